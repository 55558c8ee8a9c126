"""AutoSteer 2.0 lane-perception network: functional torch-CPU fp32 restatement of ``YOLO.forward`` of auto_steer_network.py in eval mode.

TEST INFRASTRUCTURE ONLY.  Pinned at distance 0.0 against the reference's own ``nn.Module`` (AutoSteerNetwork().build_model('n')) by
``tools/pin_autosteer_net.py`` where the reference tree is importable; the vectors are ``tests/golden/autosteer_net.npz``.

Reference (paths relative to Models/model_components):
  auto_steer/auto_steer_network.py:39-43     forward = head(fpn(net(x)))
  auto_steer/auto_steer_backbone.py:42-48    p1..p5 as AutoDrive's backbone, returns (p2, p3, p4, p5)
  auto_steer/auto_steer_neck.py:15-19        top-down C3K2 path, returns (p2, p3')
  auto_steer/auto_steer_percept_head.py:45-85  v1 / v2 row-pair convolutions, features, lane expectation, height rows
  Models/inference/auto_steer_infer.py:19-23,37-45  BGR -> RGB, to_tensor (u8 / 255), 512 x 1024 only
The backbone blocks are the ones oracle/autodrive.py restates, C3K2 the one tests/autospeed_net_ref.py restates; they take the key prefix.
"""
import numpy as np
import torch
import torch.nn.functional as F

from autospeed_net_ref import c3k2, to_torch
from oracle.autodrive import STAGES, _conv_bn_act, c2psa, ctx_block, sppf

NET_H, NET_W = 512, 1024     # auto_steer_network.py:9-10
ROWS, COLS = 64, 256         # the head's feature map


def preprocess(frame_u8, bgr=True):
    """auto_steer_infer.py:19-23: HxWx3 uint8 (BGR as OpenCV gives it) -> [3][H][W] float32 RGB planes of u8 / 255 (one IEEE division)."""
    f = np.asarray(frame_u8)
    if f.shape != (NET_H, NET_W, 3):
        raise ValueError("Incorrect input size - input image must have height of 512px and width of 1024px")
    f = f[:, :, ::-1] if bgr else f
    return (f.transpose(2, 0, 1).astype(np.float32) / np.float32(255)).astype(np.float32)


def backbone(sd, x):
    """auto_steer_backbone.py:42-48: p2 (64 x 128 x 256), p3 (128 x 64 x 128), p4 (128 x 32 x 64), p5 (256 x 16 x 32)."""
    y = _conv_bn_act(sd, "net.p1", x, stride=2)
    taps = {}
    for name, _, _, _, h, w in STAGES:
        y = _conv_bn_act(sd, f"net.{name}.0", y, stride=2)
        y = ctx_block(sd, f"net.{name}.1", y, h, w)
        taps[name] = y
    y = c2psa(sd, "net.p5.3", sppf(sd, "net.p5.2", y))
    return taps["p2"], taps["p3"], taps["p4"], y


def neck(sd, p2, p3, p4, p5):
    """auto_steer_neck.py:15-19 (Upsample(scale_factor=2): nearest): returns (p2, p3') and p4' beside them."""
    up = lambda t: F.interpolate(t, scale_factor=2.0, mode="nearest")   # noqa: E731
    p4 = c3k2(sd, "fpn.h1", torch.cat([up(p5), p4], dim=1), False)
    p3 = c3k2(sd, "fpn.h2", torch.cat([up(p4), p3], dim=1), False)
    return p2, p3, p4


def features(sd, p2, p3):
    """auto_steer_percept_head.py:48-55."""
    a = F.silu(F.conv2d(p2, sd["head.v1.weight"], sd["head.v1.bias"], stride=(2, 1)))
    b = F.silu(F.conv2d(p3, sd["head.v2.weight"], sd["head.v2.bias"], stride=(2, 1)))
    return torch.cat([F.interpolate(b, scale_factor=2.0, mode="nearest"), a], dim=1)


def lane_rows(feat, c1, c2, h1_w, h1_b, h2_w, h2_b):
    """auto_steer_percept_head.py:58-85 behind `features`; c1 / c2: callables features -> [b, 1, H, W] (Conv + BN + SiLU)."""
    lanes = F.silu(c1(feat)).softmax(dim=-1)
    w = lanes.shape[-1]
    pos = torch.arange(w, dtype=torch.int).view(1, 1, 1, w)
    xp = torch.sum(lanes * pos, dim=-1, keepdim=True) / w
    hgt = F.silu(c2(feat))
    hgt = F.silu(F.conv2d(hgt, h1_w, h1_b, stride=(1, 16)))
    hgt = F.silu(F.conv2d(hgt, h2_w, h2_b, stride=(1, 16)))
    return xp, hgt


def head(sd, feat):
    return lane_rows(feat, lambda t: _conv_bn_act(sd, "head.c1", t), lambda t: _conv_bn_act(sd, "head.c2", t), sd["head.h1.weight"], sd["head.h1.bias"],
                     sd["head.h2.weight"], sd["head.h2.bias"])


def forward(sd, x):
    """sd: numpy state dict (synthetic.make_autosteer_state_dict keys), x: [3, 512, 1024] float32 in [0, 1].
    Returns (xp [64], h_vector [64]) and the taps {"fpn.h1.conv2", "fpn.h2.conv2", "features"} as numpy CHW arrays."""
    tsd = to_torch(sd)
    with torch.no_grad():
        p2, p3, p4 = neck(tsd, *backbone(tsd, torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).reshape(1, 3, NET_H, NET_W)))
        feat = features(tsd, p2, p3)
        xp, hgt = head(tsd, feat)
    return (xp.reshape(-1).numpy(), hgt.reshape(-1).numpy()), {"fpn.h1.conv2": p4[0].numpy(), "fpn.h2.conv2": p3[0].numpy(), "features": feat[0].numpy()}
