"""Kernel-alone cases of the AutoSteer head's two kernels, shared by the emulated (tests/test_autosteer_net_emulated.py) and the device
(tests/test_gpu_autosteer_net.py) suites: same shapes, same bars, references in torch fp64.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch
import torch.nn.functional as F

import autosteer_net_ref as ref

X3_BAR, FP16_BAR = 2e-5, 1.5e-3      # the operator bars of tests/test_gpu_conv_op.py


def rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def pair_round(x):
    """x rounded through the (hi, lo) fp16 pair: what the engine's activations can hold, so a comparison sees the kernel's arithmetic only."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16).astype(np.float32)
    return hi + (x - hi).astype(np.float16).astype(np.float32)


def _lane_ref(feat, c1w, c1b, c2w, c2b, h1w, h1b, h2w, h2b):
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64))   # noqa: E731
    c1 = lambda t: F.silu(F.conv2d(t, d(c1w).view(1, -1, 3, 3), d([c1b]), padding=1))   # noqa: E731
    c2 = lambda t: F.silu(F.conv2d(t, d(c2w).view(1, -1, 3, 3), d([c2b]), padding=1))   # noqa: E731
    xp, h = ref.lane_rows(d(feat)[None], c1, c2, d(h1w).view(1, 1, 1, 16), d([h1b]), d(h2w).view(1, 1, 1, 16), d([h2b]))
    return np.stack([xp.reshape(-1).numpy(), h.reshape(-1).numpy()])


def lane_rows_cases():
    """(name, kwargs of lib.op_lane_rows_head, fp64 reference [2][5]) on 64 channels x 5 rows x 256 columns.
    general: random features and full 3x3 weights on both outputs -- rows 0 and 4 are the top and bottom border rows, columns 0 and 255 the side borders.
    crafted: c1 is the centre tap of channel 0 with weight 1 (its output IS that channel, exactly), so each row's lane logits are set directly:
      row 0 (top border)  one dominant column at index 0        -> xp ~ 0
      row 1               one dominant column at index 255      -> xp ~ 255 / 256
      row 2               all logits equal                      -> xp = 127.5 / 256
      row 3               logits of 120 .. 180: expf of them overflows fp32 (> 88.7), expf(v - max) does not -> finite
      row 4 (bottom border) random
    c2 / h1 / h2 stay general in both."""
    rng = np.random.default_rng(11)
    f32 = np.float32
    out = []
    h1w, h2w = rng.normal(0, 0.5, 16).astype(f32), rng.normal(0, 0.5, 16).astype(f32)
    c2w = rng.normal(0, 0.08, (64, 3, 3)).astype(f32)
    feat = pair_round(rng.normal(0, 1, (64, 5, 256)))
    c1w = rng.normal(0, 0.25, (64, 3, 3)).astype(f32)
    kw = dict(features=feat, c1_w=c1w, c1_b=f32(0.3), c2_w=c2w, c2_b=f32(-0.2), h1_w=h1w, h1_b=f32(0.1), h2_w=h2w, h2_b=f32(0.25))
    out.append(("general", kw, _lane_ref(feat, c1w, 0.3, c2w, -0.2, h1w, 0.1, h2w, 0.25)))
    feat = pair_round(rng.normal(0, 1, (64, 5, 256)))
    feat[0, 0], feat[0, 1], feat[0, 2] = 0.0, 0.0, 0.7
    feat[0, 0, 0] = 30.0
    feat[0, 1, 255] = 30.0
    feat[0, 3] = pair_round(120.0 + 60.0 * rng.random(256))
    c1w = np.zeros((64, 3, 3), f32)
    c1w[0, 1, 1] = 1.0
    kw = dict(features=feat, c1_w=c1w, c1_b=f32(0.0), c2_w=c2w, c2_b=f32(0.1), h1_w=h1w, h1_b=f32(-0.1), h2_w=h2w, h2_b=f32(0.0))
    out.append(("crafted", kw, _lane_ref(feat, c1w, 0.0, c2w, 0.1, h1w, -0.1, h2w, 0.0)))
    return out


def check_lane_rows(lib):
    for name, kw, want in lane_rows_cases():
        got = lib.op_lane_rows_head(precision="fp16x3", **kw)
        err = rel(got, want)
        print(f"lane_rows_head {name}: {err:.2e}; xp {got[0]}")
        assert got.shape == want.shape and np.isfinite(got).all(), name
        assert err <= X3_BAR, (name, err)
        if name == "crafted":
            assert abs(got[0, 0]) <= X3_BAR and abs(got[0, 1] - 255.0 / 256.0) <= X3_BAR and abs(got[0, 2] - 127.5 / 256.0) <= X3_BAR
            with np.errstate(over="ignore"):
                assert np.isinf(np.exp(kw["features"][0, 3].astype(np.float32))).all()      # the unshifted exponentials do overflow fp32


def check_rowpair(lib, precision, h, w, replicate):
    """cin 64 -> 32 on an h x w map into channels 32..63 of a 96-channel destination filled with a pattern: the slice within the bar of torch fp64, the
    four copies of a replicated pixel bit-identical, every other channel's (hi, lo) planes untouched."""
    rng = np.random.default_rng(h * 100 + w)
    f32 = np.float32
    x = rng.normal(0, 1, (64, h, w)).astype(f32)
    x = pair_round(x) if precision == "fp16x3" else x.astype(np.float16).astype(f32)
    wt = (rng.normal(0, 1, (32, 64, 2, 1)) * np.sqrt(2.0 / 128)).astype(f32)
    b = rng.normal(0, 0.1, 32).astype(f32)
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64))   # noqa: E731
    want = F.silu(F.conv2d(d(x)[None], d(wt), d(b), stride=(2, 1)))[0].numpy()
    f = 2 if replicate else 1
    ho, wo = (h // 2) * f, w * f
    init = pair_round(rng.normal(0, 1, (96, ho, wo))) if precision == "fp16x3" else rng.normal(0, 1, (96, ho, wo)).astype(np.float16).astype(f32)
    hi, lo = lib.op_rowpair_conv(x, wt, b, replicate=replicate, dst=init, dst_off=32, precision=precision)
    got = hi.astype(f32) + lo.astype(f32)
    if replicate:
        want = want.repeat(2, axis=1).repeat(2, axis=2)
        for plane in (hi, lo):
            s = plane[32:64].view(np.uint16)
            assert all(np.array_equal(s[:, 0::2, 0::2], s[:, dy::2, dx::2]) for dy in (0, 1) for dx in (0, 1))
    err = rel(got[32:64], want)
    print(f"rowpair_conv {precision} {h}x{w} replicate={replicate}: {err:.2e}")
    assert err <= (X3_BAR if precision == "fp16x3" else FP16_BAR), err
    ih = init.astype(np.float16)
    il = (init - ih.astype(f32)).astype(np.float16) if precision == "fp16x3" else np.zeros_like(ih)
    for a in (slice(0, 32), slice(64, 96)):
        assert np.array_equal(hi[a].view(np.uint16), ih[a].view(np.uint16)) and np.array_equal(lo[a].view(np.uint16), il[a].view(np.uint16))
