"""Synthetic data of the reference's shapes: seeded random-init weights in the reference ``state_dict`` key layout and
seeded camera frames.  No dataset or checkpoint is reachable from the build / benchmark boxes, so ``bench.py``, the
profiling tools and the tests all draw their inputs from here (BASELINE.json: "synthetic data of that shape, random-init
weights of that architecture").  Pure data generation -- no network arithmetic lives in this module; the CPU oracle
(``oracle/``, test infrastructure) re-exports these generators so checker and engine always see identical tensors.

The key layout is the reference's ``state_dict`` key layout, so the same dict can be ``load_state_dict``-ed into the
reference's own modules (oracle/pin_against_reference.py) and exported to the engine's weight blob (weights.py).

Key prefixes:
  SceneSeg  : Backbone.encoder.* SceneContext.* SceneNeck.* SceneSegHead.*
              (Models/model_components/scene_seg_network.py:11-21)
  Scene3D   : PreTrainedBackbone.pretrainedBackBone.encoder.* DepthContext.* DepthNeck.* SuperDepthHead.*
              (scene_3d_network.py:13-22, pre_trained_backbone.py:10)
  DomainSeg : DomainSegUpstream.{pretrainedBackBone.encoder,pretrainedContext,pretrainedNeck}.* DomainSegHead.*
              (domain_seg_network.py:11-14, domain_seg_upstream.py:10-20)
  EgoLanes  : BEVBackbone.encoder.* AutoSteerContext.* EgopathNeck.* EgoLanesHead.*
              (ego_lanes_network.py:14-26)
  AutoDrive : backbone.p1..p5.* head.*  (autodrive/autodrive_network.py, autodrive_backbone.py:8-48, autodrive_head.py:70-87)

Init is NOT PyTorch's default: with default init the decoder contracts the signal ~0.6x/layer and argmax collapses to
one class (SURVEY.md 8(d) init note), which would make every parity check vacuous.  A variance-preserving init is used.
"""
import numpy as np

# torchvision efficientnet_b0 inverted-residual setting (published architecture):
# (expand_ratio, kernel, stride, in_ch, out_ch, num_layers)
B0_STAGES = [
    (1, 3, 1, 32, 16, 1),
    (6, 3, 2, 16, 24, 2),
    (6, 5, 2, 24, 40, 2),
    (6, 3, 2, 40, 80, 3),
    (6, 5, 1, 80, 112, 3),
    (6, 5, 2, 112, 192, 4),
    (6, 3, 1, 192, 320, 1),
]
B0_STEM_OUT = 32
B0_LAST_OUT = 1280
BN_EPS = 1e-5

MODEL_KINDS = ("sceneseg", "scene3d", "domainseg", "egolanes")

PREFIX = {
    "sceneseg": dict(backbone="Backbone.encoder.", context="SceneContext.",
                     neck="SceneNeck.", head="SceneSegHead."),
    "scene3d": dict(backbone="PreTrainedBackbone.pretrainedBackBone.encoder.", context="DepthContext.",
                    neck="DepthNeck.", head="SuperDepthHead."),
    "domainseg": dict(backbone="DomainSegUpstream.pretrainedBackBone.encoder.",
                      context="DomainSegUpstream.pretrainedContext.",
                      neck="DomainSegUpstream.pretrainedNeck.", head="DomainSegHead."),
    "egolanes": dict(backbone="BEVBackbone.encoder.", context="AutoSteerContext.",
                     neck="EgopathNeck.", head="EgoLanesHead."),
}


def _bn(p, c):
    return [(p + ".weight", (c,), "bn_w"), (p + ".bias", (c,), "bn_b"),
            (p + ".running_mean", (c,), "bn_mean"), (p + ".running_var", (c,), "bn_var")]


def backbone_spec(prefix):
    """(key, shape, kind) for every tensor of torchvision efficientnet_b0().features."""
    s = [(prefix + "0.0.weight", (B0_STEM_OUT, 3, 3, 3), "conv")]
    s += _bn(prefix + "0.1", B0_STEM_OUT)
    for si, (e, k, st, cin, cout, n) in enumerate(B0_STAGES, start=1):
        for bi in range(n):
            ci = cin if bi == 0 else cout
            cexp = ci * e
            p = f"{prefix}{si}.{bi}.block."
            j = 0
            if e != 1:
                s.append((p + f"{j}.0.weight", (cexp, ci, 1, 1), "conv"))
                s += _bn(p + f"{j}.1", cexp)
                j += 1
            s.append((p + f"{j}.0.weight", (cexp, 1, k, k), "conv"))  # depthwise
            s += _bn(p + f"{j}.1", cexp)
            j += 1
            sq = max(1, ci // 4)
            s += [(p + f"{j}.fc1.weight", (sq, cexp, 1, 1), "conv"), (p + f"{j}.fc1.bias", (sq,), "bias"),
                  (p + f"{j}.fc2.weight", (cexp, sq, 1, 1), "conv"), (p + f"{j}.fc2.bias", (cexp,), "bias")]
            j += 1
            s.append((p + f"{j}.0.weight", (cout, cexp, 1, 1), "conv"))
            s += _bn(p + f"{j}.1", cout)
    s.append((prefix + "8.0.weight", (B0_LAST_OUT, 320, 1, 1), "conv"))
    s += _bn(prefix + "8.1", B0_LAST_OUT)
    return s


def _conv(p, cout, cin, k):
    return [(p + ".weight", (cout, cin, k, k), "conv"), (p + ".bias", (cout,), "bias")]


def _convT(p, cin, cout):
    return [(p + ".weight", (cin, cout, 2, 2), "convT"), (p + ".bias", (cout,), "bias")]


def _lin(p, cout, cin):
    return [(p + ".weight", (cout, cin), "linear"), (p + ".bias", (cout,), "bias")]


def context_spec(prefix, cin):
    """scene_context.py:14-22 / depth_context.py:14-22 (cin=1280); auto_steer_context.py:15-23 (cin=1456)."""
    return (_lin(prefix + "context_layer_0", 800, cin) + _lin(prefix + "context_layer_1", 800, 800)
            + _lin(prefix + "context_layer_2", 200, 800)
            + _conv(prefix + "context_layer_3", 128, 1, 3) + _conv(prefix + "context_layer_4", 256, 128, 3)
            + _conv(prefix + "context_layer_5", 512, 256, 3) + _conv(prefix + "context_layer_6", cin, 512, 3))


def neck_spec(prefix, cin):
    """scene_neck.py:11-24 / scene_3d_neck.py:11-24 (cin=1280); ego_path_neck.py:11-24 (cin=1456)."""
    return (_convT(prefix + "upsample_layer_0", cin, cin) + _conv(prefix + "skip_link_layer_0", cin, 80, 1)
            + _conv(prefix + "decode_layer_0", 768, cin, 3) + _conv(prefix + "decode_layer_1", 768, 768, 3)
            + _convT(prefix + "upsample_layer_1", 768, 768) + _conv(prefix + "skip_link_layer_1", 768, 40, 1)
            + _conv(prefix + "decode_layer_2", 512, 768, 3) + _conv(prefix + "decode_layer_3", 512, 512, 3)
            + _convT(prefix + "upsample_layer_2", 512, 512) + _conv(prefix + "skip_link_layer_2", 512, 24, 1)
            + _conv(prefix + "decode_layer_4", 512, 512, 3) + _conv(prefix + "decode_layer_5", 256, 512, 3))


def head_spec(kind, prefix):
    """scene_seg_head.py:11-19, scene_3d_head.py:13-21, domain_seg_head.py:11-19, ego_lanes_head.py:11-13."""
    if kind == "egolanes":
        return (_conv(prefix + "decode_layer_6", 256, 256, 3) + _conv(prefix + "decode_layer_7", 128, 256, 3)
                + _conv(prefix + "decode_layer_8", 3, 128, 3))
    c9, cout = {"sceneseg": (64, 3), "scene3d": (128, 1), "domainseg": (64, 1)}[kind]
    return (_convT(prefix + "upsample_layer_3", 256, 256) + _conv(prefix + "skip_link_layer_3", 256, 32, 1)
            + _conv(prefix + "decode_layer_6", 256, 256, 3) + _conv(prefix + "decode_layer_7", 128, 256, 3)
            + _convT(prefix + "upsample_layer_4", 128, 128)
            + _conv(prefix + "decode_layer_8", 128, 128, 3) + _conv(prefix + "decode_layer_9", c9, 128, 3)
            + _conv(prefix + "decode_layer_10", cout, c9, 3))


def context_channels(kind):
    return 1456 if kind == "egolanes" else 1280


def model_spec(kind):
    p = PREFIX[kind]
    c = context_channels(kind)
    return (backbone_spec(p["backbone"]) + context_spec(p["context"], c)
            + neck_spec(p["neck"], c) + head_spec(kind, p["head"]))


def _init(rng, shape, kind):
    f32 = np.float32
    if kind == "conv":
        fan_in = shape[1] * shape[2] * shape[3]
        return (rng.standard_normal(shape, dtype=f32) * f32(np.sqrt(2.0 / fan_in))).astype(f32)
    if kind == "linear":
        return (rng.standard_normal(shape, dtype=f32) * f32(np.sqrt(2.0 / shape[1]))).astype(f32)
    if kind == "convT":  # k2 s2: each output pixel sees exactly one tap -> fan_in = Cin
        return (rng.standard_normal(shape, dtype=f32) * f32(np.sqrt(1.0 / shape[0]))).astype(f32)
    if kind in ("bias", "bn_b", "bn_mean"):
        return (rng.standard_normal(shape, dtype=f32) * f32(0.1)).astype(f32)
    if kind in ("bn_w", "bn_var"):
        return rng.uniform(0.5, 1.5, size=shape).astype(f32)
    raise ValueError(kind)


def make_state_dict(kind, seed, spec=None):
    """Deterministic name->np.float32 array dict for ``kind`` (numpy PCG64, one stream, spec order)."""
    rng = np.random.default_rng(seed)
    return {k: _init(rng, shape, kd) for (k, shape, kd) in (spec or model_spec(kind))}


def share_backbone(dst_sd, dst_kind, src_sd, src_kind, also_context_neck=False):
    """Graft ``src``'s backbone (and optionally context+neck) tensors into ``dst`` under dst's key
    prefixes -- what Scene3DNetwork(pretrained) / DomainSegNetwork(pretrained) do by object sharing
    (pre_trained_backbone.py:10, domain_seg_upstream.py:10-20)."""
    parts = ["backbone"] + (["context", "neck"] if also_context_neck else [])
    for part in parts:
        sp, dp = PREFIX[src_kind][part], PREFIX[dst_kind][part]
        for k, v in src_sd.items():
            if k.startswith(sp):
                dst_sd[dp + k[len(sp):]] = v
    return dst_sd


def param_count(kind):
    return sum(int(np.prod(s)) for (_, s, kd) in model_spec(kind) if kd not in ("bn_mean", "bn_var"))


# ------------------------------------------------------------------------------------------------ AutoDrive
AD_BN_EPS = 1e-3                      # common_layers.py:10
AD_NET_H, AD_NET_W = 512, 1024        # autodrive_network.py:8-9
# (stage, cin of the strided conv, cout of the strided conv, CTX out, CTX map h, w)   autodrive_backbone.py:13-40
AD_STAGES = [("p2", 16, 32, 64, 128, 256), ("p3", 64, 64, 128, 64, 128), ("p4", 128, 128, 128, 32, 64), ("p5", 128, 256, 256, 16, 32)]


def _ad_conv_bn(p, cout, cin, k, groups=1):
    return [(p + ".conv.weight", (cout, cin // groups, k, k), "conv"), (p + ".norm.weight", (cout,), "bn_w"),
            (p + ".norm.bias", (cout,), "bn_b"), (p + ".norm.running_mean", (cout,), "bn_mean"),
            (p + ".norm.running_var", (cout,), "bn_var")]


def _ad_ctx(p, cin, cout, h, w, r=2):
    return [(p + ".exp0.weight", (h * w, cin, 3), "conv1d"), (p + ".exp0.bias", (h * w,), "bias"),
            (p + ".ctx0.weight", (cin // r, 1, 3, 3), "conv"), (p + ".ctx0.bias", (cin // r,), "bias"),
            (p + ".ctx1.weight", (cin, cin // r, 3, 3), "conv"), (p + ".ctx1.bias", (cin,), "bias"),
            (p + ".ctx2.weight", (cout, cin, 3, 3), "conv"), (p + ".ctx2.bias", (cout,), "bias")]


def autodrive_spec():
    """(key, shape, init kind) in the reference ``state_dict`` order (num_batches_tracked omitted)."""
    s = _ad_conv_bn("backbone.p1", 16, 3, 3)
    for name, cin, cmid, cout, h, w in AD_STAGES:
        s += _ad_conv_bn(f"backbone.{name}.0", cmid, cin, 3)
        s += _ad_ctx(f"backbone.{name}.1", cmid, cout, h, w)
    s += _ad_conv_bn("backbone.p5.2.cv1", 128, 256, 1) + _ad_conv_bn("backbone.p5.2.cv2", 256, 512, 1)   # SPPF
    s += _ad_conv_bn("backbone.p5.3.cv1", 256, 256, 1) + _ad_conv_bn("backbone.p5.3.cv2", 256, 256, 1)   # C2PSA
    a = "backbone.p5.3.middle_block"
    s += _ad_conv_bn(a + ".conv1.qkv", 256, 128, 1) + _ad_conv_bn(a + ".conv1.conv1", 128, 128, 3, groups=128)
    s += _ad_conv_bn(a + ".conv1.conv2", 128, 128, 1) + _ad_conv_bn(a + ".conv2.0", 256, 128, 1) + _ad_conv_bn(a + ".conv2.1", 128, 256, 1)
    s += [("head.conv_1.weight", (256, 512, 3, 3), "conv"), ("head.conv_1.bias", (256,), "bias"),
          ("head.conv_2.weight", (64, 256, 3, 3), "conv"), ("head.conv_2.bias", (64,), "bias"),
          ("head.conv_3.weight", (2, 64, 3, 3), "conv"), ("head.conv_3.bias", (2,), "bias"),
          ("head.fc1.0.weight", (768, 1024), "linear"), ("head.fc1.0.bias", (768,), "bias"),
          ("head.fc2.0.weight", (512, 768), "linear"), ("head.fc2.0.bias", (512,), "bias"),
          ("head.distance_head.0.weight", (1, 512), "linear"), ("head.distance_head.0.bias", (1,), "bias"),
          ("head.curvature_head.0.weight", (1, 512), "linear"), ("head.curvature_head.0.bias", (1,), "bias"),
          ("head.flag_head.weight", (1, 512), "linear"), ("head.flag_head.bias", (1,), "bias")]
    return s


def make_autodrive_state_dict(seed):
    """Seeded init (scheme of make_state_dict above) tuned so every stage carries O(1) signal and no output saturates:
    CTX gates multiplicatively (c4*x + x, with c4 driven by mean(x)), so Kaiming gains square the scale per stage
    (measured: P5 std 2e4, all three outputs clipped -> vacuous parity).  exp0 and ctx2 weights get gain 0.5 and the
    distance head's bias +1 (pre-ReLU value ~ +0.5): per-stage std 0.9 / 0.6 / 0.4 / 0.2, P5 std ~2, outputs
    (d, curvature, flag) ~ (0.5, 0.5, -1.1) on the fixture frames."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, shape, kind in autodrive_spec():
        if kind == "conv1d":  # Conv1d on a length-1 sequence: only the centre tap ever multiplies data
            out[k] = (rng.standard_normal(shape, dtype=np.float32) * np.float32(0.5 * np.sqrt(2.0 / shape[1]))).astype(np.float32)
        else:
            out[k] = _init(rng, shape, kind)
        if k.endswith("ctx2.weight"):
            out[k] = out[k] * np.float32(0.5)
        if k == "head.distance_head.0.bias":
            out[k] = out[k] + np.float32(1.0)
    return out


def autodrive_param_count():
    return sum(int(np.prod(s)) for _, s, _ in autodrive_spec())


# ------------------------------------------------------------------------------------------------ AutoSpeed detector network
AS_NET_H, AS_NET_W = 512, 1024        # auto_speed_network.py:9-10
AS_NUM_CLASSES = 4
AS_STRIDES = (8, 16, 32)
AS_NUM_ANCHORS = sum((AS_NET_H // s) * (AS_NET_W // s) for s in AS_STRIDES)   # 10752


def _as_c3k2(p, cin, cout, csp, r=2):
    """common_layers.py:166-180 C3K2 with n = 1: conv1, conv2, then res_m.0 = Residual (:20-27) or C3K (:149-163)."""
    c = cout // r
    s = _ad_conv_bn(p + ".conv1", 2 * c, cin, 1) + _ad_conv_bn(p + ".conv2", cout, 3 * c, 1)
    m = p + ".res_m.0"
    if not csp:
        return s + _ad_conv_bn(m + ".conv1", c // 2, c, 3) + _ad_conv_bn(m + ".conv2", c, c // 2, 3)
    s += _ad_conv_bn(m + ".conv1", c // 2, c, 1) + _ad_conv_bn(m + ".conv2", c // 2, c, 1) + _ad_conv_bn(m + ".conv3", c, c, 1)
    for i in range(2):   # Residual(c / 2, e = 1.0)
        s += _ad_conv_bn(f"{m}.res_m.{i}.conv1", c // 2, c // 2, 3) + _ad_conv_bn(f"{m}.res_m.{i}.conv2", c // 2, c // 2, 3)
    return s


def autospeed_spec(num_classes=AS_NUM_CLASSES):
    """(key, shape, init kind) of AutoSpeedNetwork().build_model('n', num_classes) in the reference ``state_dict`` order, num_batches_tracked
    omitted (auto_speed_network.py:33-43, auto_speed_backbone.py:8-49, auto_speed_neck.py:8-16, auto_speed_head.py:24-49).  The backbone under
    ``net.`` is AutoDrive's under ``backbone.``, key for key."""
    s = [("net." + k[len("backbone."):], shape, kind) for k, shape, kind in autodrive_spec() if k.startswith("backbone.")]
    s += _as_c3k2("fpn.h1", 128 + 256, 128, False) + _as_c3k2("fpn.h2", 128 + 128, 64, False) + _ad_conv_bn("fpn.h3", 64, 64, 3)
    s += _as_c3k2("fpn.h4", 64 + 128, 128, False) + _ad_conv_bn("fpn.h5", 128, 128, 3) + _as_c3k2("fpn.h6", 128 + 256, 256, True)
    filters = (64, 128, 256)
    box, cls = max(64, filters[0] // 4), max(80, filters[0], num_classes)
    s += [("head.dfl.conv.weight", (1, 16, 1, 1), "dfl")]
    for i, x in enumerate(filters):
        s += _ad_conv_bn(f"head.box.{i}.0", box, x, 3) + _ad_conv_bn(f"head.box.{i}.1", box, box, 3)
        s += [(f"head.box.{i}.2.weight", (64, box, 1, 1), "conv"), (f"head.box.{i}.2.bias", (64,), "bias")]
    for i, x in enumerate(filters):
        s += _ad_conv_bn(f"head.cls.{i}.0", x, x, 3, groups=x) + _ad_conv_bn(f"head.cls.{i}.1", cls, x, 1)
        s += _ad_conv_bn(f"head.cls.{i}.2", cls, cls, 3, groups=cls) + _ad_conv_bn(f"head.cls.{i}.3", cls, cls, 1)
        s += [(f"head.cls.{i}.4.weight", (num_classes, cls, 1, 1), "conv"), (f"head.cls.{i}.4.bias", (num_classes,), "bias")]
    return s


AS_CLS_LOGIT_GAIN, AS_CLS_LOGIT_BIAS = 3.0, -4.0
AS_BOX_LOGIT_GAIN = 3.0


def make_autospeed_state_dict(seed, num_classes=AS_NUM_CLASSES):
    """Seeded init of the detector network: the backbone as make_autodrive_state_dict tunes it (exp0 / ctx2 gains), DFL's constant 0..15.
    The module's own initialisation (auto_speed_head.py:68-80) gives class scores of at most 0.0024 -- no detection at any useful threshold -- so
    the last class convolution gets gain AS_CLS_LOGIT_GAIN and bias AS_CLS_LOGIT_BIAS (scores spread over (0, 1) with a few per cent of the anchors
    above 0.25) and the last box convolution gain AS_BOX_LOGIT_GAIN (peaked bin distributions: boxes of many sizes, so NMS has work to do)."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, shape, kind in autospeed_spec(num_classes):
        if kind == "dfl":
            out[k] = np.arange(16, dtype=np.float32).reshape(shape)
        elif kind == "conv1d":   # net.pN.1.exp0.weight of the backbone's CTX blocks (_ad_ctx): gain 0.5, as make_autodrive_state_dict
            out[k] = (rng.standard_normal(shape, dtype=np.float32) * np.float32(0.5 * np.sqrt(2.0 / shape[1]))).astype(np.float32)
        else:
            out[k] = _init(rng, shape, kind)
        if k.endswith("ctx2.weight"):
            out[k] = out[k] * np.float32(0.5)
        if k.startswith("head.cls.") and k.endswith(".4.weight"):
            out[k] = out[k] * np.float32(AS_CLS_LOGIT_GAIN)
        if k.startswith("head.cls.") and k.endswith(".4.bias"):
            out[k] = out[k] + np.float32(AS_CLS_LOGIT_BIAS)
        if k.startswith("head.box.") and k.endswith(".2.weight"):
            out[k] = out[k] * np.float32(AS_BOX_LOGIT_GAIN)
    return out


def autospeed_param_count(num_classes=AS_NUM_CLASSES):
    return sum(int(np.prod(s)) for k, s, _ in autospeed_spec(num_classes) if not k.endswith(("running_mean", "running_var")))


# ------------------------------------------------------------------------------------------------ AutoSteer 2.0 lane-perception network
AST_ROWS, AST_COLS = 64, 256          # the head's feature map at 512 x 1024


def autosteer_spec():
    """(key, shape, init kind) of AutoSteerNetwork().build_model('n') in the reference ``state_dict`` order, num_batches_tracked omitted
    (auto_steer_network.py:33-43, auto_steer_backbone.py:8-40, auto_steer_neck.py:8-13, auto_steer_percept_head.py:29-43).  The backbone under ``net.`` is
    AutoDrive's under ``backbone.``, key for key; ``fpn.h1`` / ``fpn.h2`` are the detector neck's."""
    s = [("net." + k[len("backbone."):], shape, kind) for k, shape, kind in autodrive_spec() if k.startswith("backbone.")]
    s += _as_c3k2("fpn.h1", 128 + 256, 128, False) + _as_c3k2("fpn.h2", 128 + 128, 64, False)
    s += _ad_conv_bn("head.c1", 1, 64, 3) + _ad_conv_bn("head.c2", 1, 64, 3)
    for v in ("v1", "v2"):
        s += [(f"head.{v}.weight", (32, 64, 2, 1), "conv"), (f"head.{v}.bias", (32,), "bias")]
    for h in ("h1", "h2"):
        s += [(f"head.{h}.weight", (1, 1, 1, 16), "conv"), (f"head.{h}.bias", (1,), "bias")]
    return s


# With plain random head weights the row softmax is nearly uniform (every xp ~ 0.498) and h_vector sits on one side of 0.5: every test of the
# outputs would be vacuous.  Chosen over a small grid by tools/pin_autosteer_net.py so that the conditions it asserts hold on its fixture frames:
AST_C1_NORM_GAIN = 12.0                # head.c1.norm.weight: a peaked row softmax, xp spread over the rows
AST_C2_NORM_GAIN = 2.0                 # head.c2.norm.weight
AST_H1_GAIN, AST_H1_BIAS = 2.0, 0.0    # head.h1.weight / bias
AST_H2_GAIN, AST_H2_BIAS = 4.0, -0.5   # head.h2.weight / bias: h_vector on both sides of 0.5


def make_autosteer_state_dict(seed, gains=None):
    """Seeded init of the lane-perception network: the backbone as make_autodrive_state_dict tunes it (exp0 / ctx2 gains), the head with the gains
    above (``gains``: a dict overriding them by name, c1 / c2 / h1 / h1_bias / h2 / h2_bias -- the pin tool's grid search)."""
    g = {"c1": AST_C1_NORM_GAIN, "c2": AST_C2_NORM_GAIN, "h1": AST_H1_GAIN, "h1_bias": AST_H1_BIAS, "h2": AST_H2_GAIN, "h2_bias": AST_H2_BIAS}
    g.update(gains or {})
    rng = np.random.default_rng(seed)
    out = {}
    for k, shape, kind in autosteer_spec():
        if kind == "conv1d":   # net.pN.1.exp0.weight of the backbone's CTX blocks (_ad_ctx): gain 0.5, as make_autodrive_state_dict
            out[k] = (rng.standard_normal(shape, dtype=np.float32) * np.float32(0.5 * np.sqrt(2.0 / shape[1]))).astype(np.float32)
        else:
            out[k] = _init(rng, shape, kind)
        if k.endswith("ctx2.weight"):
            out[k] = out[k] * np.float32(0.5)
    out["head.c1.norm.weight"] = out["head.c1.norm.weight"] * np.float32(g["c1"])
    out["head.c2.norm.weight"] = out["head.c2.norm.weight"] * np.float32(g["c2"])
    for h in ("h1", "h2"):
        out[f"head.{h}.weight"] = out[f"head.{h}.weight"] * np.float32(g[h])
        out[f"head.{h}.bias"] = out[f"head.{h}.bias"] + np.float32(g[h + "_bias"])
    return out


def autosteer_param_count():
    return sum(int(np.prod(s)) for k, s, _ in autosteer_spec() if not k.endswith(("running_mean", "running_var")))


# ------------------------------------------------------------------------------------------------ frames
def synthetic_frame(h, w, seed, smooth=True):
    """Seeded u8 HxWx3 frame.  ``smooth`` mixes low-frequency sinusoids with noise so argmax regions are
    non-trivial."""
    rng = np.random.default_rng(seed)
    if not smooth:
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.empty((h, w, 3), dtype=np.float32)
    for c in range(3):
        fy, fx, ph = rng.uniform(1.0, 6.0), rng.uniform(1.0, 6.0), rng.uniform(0, 6.28)
        img[..., c] = 127.5 + 90.0 * np.sin(2 * np.pi * (fy * yy / h + fx * xx / w) + ph)
    img += rng.normal(0.0, 12.0, size=img.shape).astype(np.float32)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ a second weight family
_PAIRS = (("context_layer_0", "context_layer_1"), ("context_layer_4", "context_layer_5"), ("decode_layer_0", "decode_layer_1"),
          ("decode_layer_2", "decode_layer_3"), ("decode_layer_4", "decode_layer_5"), ("decode_layer_6", "decode_layer_7"),
          ("decode_layer_8", "decode_layer_9"))


def make_trained_like_state_dict(kind, seed):
    """"Trained-like" statistics beside the variance-preserving family of make_state_dict: what a checkpoint has and a
    Kaiming draw has not.
      * encoder: every convolution that feeds a BatchNorm is scaled per OUTPUT CHANNEL by s * g_c (s ~ U(0.1, 0.3) per layer, g_c log-uniform
        over three decades) and the layer's running_mean / running_var follow (x f, x f^2): gamma / sqrt(var + eps) then spreads over 10^3 across
        the channels of a layer, the smallest variances sink to the order of eps (near-dead channels), and the function stays the base
        family's up to eps -- BN folding, the per-row weight prescale and the (hi, lo) split see rows of very different magnitude;
      * context / neck / head (no normalisation layers): the 3x3 convolutions and the context MLP come in (down, up) pairs -- the first of a
        pair (weights and bias) x s, the second x 1 / s, s ~ U(0.1, 0.3) -- so every second tensor of the decoder is 3-10x SMALLER than in the
        base family (|x| well under 0.1, where the lo plane of an fp16 pair is subnormal) while the logits stay O(1) (GELU is not
        homogeneous, so the function differs from the base family's: a different network, not a re-parameterisation).
    Same key layout, deterministic in (kind, seed)."""
    f32 = np.float32
    sd = make_state_dict(kind, seed)
    rng = np.random.default_rng(seed + 7919)
    for k, shape, kd in model_spec(kind):
        if kd == "conv" and k.endswith(".0.weight") and (k[:-len("0.weight")] + "1.running_var") in sd:
            base = k[:-len("0.weight")]
            f = (rng.uniform(0.1, 0.3) * 10.0 ** rng.uniform(-1.5, 1.5, size=shape[0])).astype(f32)
            sd[k] = (sd[k] * f[:, None, None, None]).astype(f32)
            sd[base + "1.running_mean"] = (sd[base + "1.running_mean"] * f).astype(f32)
            sd[base + "1.running_var"] = (sd[base + "1.running_var"] * f * f).astype(f32)
    keys = list(sd)
    for down, up in _PAIRS:
        kd_ = [k for k in keys if k.endswith(down + ".weight")]
        ku_ = [k for k in keys if k.endswith(up + ".weight")]
        if not kd_ or not ku_:
            continue
        s = f32(rng.uniform(0.1, 0.3))
        sd[kd_[0]] = (sd[kd_[0]] * s).astype(f32)
        sd[kd_[0][:-len("weight")] + "bias"] = (sd[kd_[0][:-len("weight")] + "bias"] * s).astype(f32)
        sd[ku_[0]] = (sd[ku_[0]] / s).astype(f32)
    return sd
