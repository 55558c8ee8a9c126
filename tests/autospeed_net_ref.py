"""AutoSpeed detector network: functional torch-CPU fp32 restatement of ``YOLO.forward`` in eval mode.

TEST INFRASTRUCTURE ONLY.  Pinned at distance 0.0 against the reference's own ``nn.Module`` (AutoSpeedNetwork().build_model('n', 4)) by
``tools/pin_autospeed_net.py`` where the reference tree is importable; the vectors are ``tests/golden/autospeed_net.npz``.

Reference (paths relative to Models/model_components):
  auto_speed/auto_speed_network.py:45-48    forward = head(fpn(net(x)))
  auto_speed/auto_speed_backbone.py:42-48   p1..p5 as AutoDrive's backbone, returns (p3, p4, p5)
  auto_speed/auto_speed_neck.py:18-24       top-down + bottom-up C3K2 path
  auto_speed/auto_speed_head.py:51-66       per-level box / cls branches, DFL, anchors, strides, sigmoid
  common_layers.py:5-14 (Conv), :20-27 (Residual), :133-146 (DFL), :149-163 (C3K), :166-180 (C3K2)
The backbone blocks (Conv, CTX, SPPF, C2PSA) are the ones oracle/autodrive.py restates; they take the key prefix.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.autodrive import STAGES, _conv_bn_act, c2psa, ctx_block, sppf

NET_H, NET_W = 512, 1024     # auto_speed_network.py:9-10
STRIDES = (8.0, 16.0, 32.0)  # auto_speed_network.py:41: image height / level height


def to_torch(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def backbone(sd, x):
    """auto_speed_backbone.py:42-48: p3 (128 x 64 x 128), p4 (128 x 32 x 64), p5 (256 x 16 x 32)."""
    y = _conv_bn_act(sd, "net.p1", x, stride=2)
    taps = {}
    for name, _, _, _, h, w in STAGES:
        y = _conv_bn_act(sd, f"net.{name}.0", y, stride=2)
        y = ctx_block(sd, f"net.{name}.1", y, h, w)
        taps[name] = y
    y = c2psa(sd, "net.p5.3", sppf(sd, "net.p5.2", y))
    return taps["p3"], taps["p4"], y


def residual(sd, p, x):
    """common_layers.py:26-27: x + conv2(conv1(x)), both Conv k3 + BN + SiLU."""
    return x + _conv_bn_act(sd, p + ".conv2", _conv_bn_act(sd, p + ".conv1", x))


def c3k(sd, p, x):
    """common_layers.py:160-163."""
    y = residual(sd, p + ".res_m.1", residual(sd, p + ".res_m.0", _conv_bn_act(sd, p + ".conv1", x)))
    return _conv_bn_act(sd, p + ".conv3", torch.cat((y, _conv_bn_act(sd, p + ".conv2", x)), dim=1))


def c3k2(sd, p, x, csp):
    """common_layers.py:177-180 with n = 1."""
    y = list(_conv_bn_act(sd, p + ".conv1", x).chunk(2, 1))
    y.append((c3k if csp else residual)(sd, p + ".res_m.0", y[-1]))
    return _conv_bn_act(sd, p + ".conv2", torch.cat(y, dim=1))


def neck(sd, p3, p4, p5):
    """auto_speed_neck.py:18-24 (Upsample(scale_factor=2): nearest)."""
    up = lambda t: F.interpolate(t, scale_factor=2.0, mode="nearest")   # noqa: E731
    p4 = c3k2(sd, "fpn.h1", torch.cat([up(p5), p4], dim=1), False)
    p3 = c3k2(sd, "fpn.h2", torch.cat([up(p4), p3], dim=1), False)
    p4 = c3k2(sd, "fpn.h4", torch.cat([_conv_bn_act(sd, "fpn.h3", p3, stride=2), p4], dim=1), False)
    p5 = c3k2(sd, "fpn.h6", torch.cat([_conv_bn_act(sd, "fpn.h5", p4, stride=2), p5], dim=1), True)
    return p3, p4, p5


def head_levels(sd, feats):
    """auto_speed_head.py:39-53: per level cat(box(x), cls(x)) = 64 + nc channels."""
    out = []
    for i, x in enumerate(feats):
        b = _conv_bn_act(sd, f"head.box.{i}.1", _conv_bn_act(sd, f"head.box.{i}.0", x))
        b = F.conv2d(b, sd[f"head.box.{i}.2.weight"], sd[f"head.box.{i}.2.bias"])
        c = _conv_bn_act(sd, f"head.cls.{i}.0", x, groups=x.shape[1])
        c = _conv_bn_act(sd, f"head.cls.{i}.1", c)
        c = _conv_bn_act(sd, f"head.cls.{i}.2", c, groups=c.shape[1])
        c = _conv_bn_act(sd, f"head.cls.{i}.3", c)
        c = F.conv2d(c, sd[f"head.cls.{i}.4.weight"], sd[f"head.cls.{i}.4.bias"])
        out.append(torch.cat((b, c), dim=1))
    return out


def dfl(sd, box):
    """common_layers.py:143-146: [b, 64, a] -> softmax over the 16 bins of each side -> 1x1 conv with the constant 0..15."""
    b, _, a = box.shape
    return F.conv2d(box.view(b, 4, 16, a).transpose(2, 1).softmax(1), sd["head.dfl.conv.weight"]).view(b, 4, a)


def decode(sd, levels, dtype=None):
    """auto_speed_head.py:57-66 + make_anchors (:8-21, offset 0.5)."""
    nc = levels[0].shape[1] - 64
    anchors, strides = [], []
    for lv, s in zip(levels, STRIDES):
        h, w = lv.shape[-2:]
        sy, sx = torch.meshgrid(torch.arange(h, dtype=lv.dtype) + 0.5, torch.arange(w, dtype=lv.dtype) + 0.5, indexing="ij")
        anchors.append(torch.stack((sx, sy), -1).view(-1, 2))
        strides.append(torch.full((h * w, 1), s, dtype=lv.dtype))
    anchors, strides = torch.cat(anchors).transpose(0, 1), torch.cat(strides).transpose(0, 1)
    x = torch.cat([lv.view(lv.shape[0], 64 + nc, -1) for lv in levels], dim=2)
    box, cls = x.split((64, nc), dim=1)
    a, b = dfl(sd, box).chunk(2, 1)
    a = anchors.unsqueeze(0) - a
    b = anchors.unsqueeze(0) + b
    box = torch.cat(((a + b) / 2, b - a), dim=1)
    return torch.cat((box * strides, cls.sigmoid()), dim=1)


def forward(sd, x):
    """sd: numpy state dict (synthetic.make_autospeed_state_dict keys), x: [1, 3, 512, 1024] float32 in [0, 1].
    Returns raw [4 + nc, 10752] and the neck's (P3, P4, P5) as numpy CHW arrays."""
    tsd = to_torch(sd)
    with torch.no_grad():
        feats = neck(tsd, *backbone(tsd, torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).reshape(1, 3, NET_H, NET_W)))
        raw = decode(tsd, head_levels(tsd, list(feats)))
    return raw[0].numpy(), tuple(f[0].numpy() for f in feats)
