"""The convolution forms the AutoDrive / AutoSpeed / AutoSteer plans launch beyond what vp_op_conv2d can express, one operator at a time through
vp_op_conv2d_forms (the engine's own add_conv: production dispatch, packing and epilogue routing): A 3x3 stride 2, B the CTX gate (activation behind the
residual), C alias-slice destinations and a residual read from a slice, D the same under the activation scale, E the plan-time refusals.  Shared by the
emulated (tests/test_conv_forms_emulated.py) and the device (tests/test_gpu_conv_forms.py) suites: same shapes, same bars.  TEST INFRASTRUCTURE ONLY.

Reference: torch fp64 on the operands AS STORED -- an fp16x3 engine holds pair_round(v * 2^-s) * 2^s of a value v under exponent s (s = 0 without the
activation scale), an fp16 engine the value rounded through fp16, an fp8-storage engine the de-quantised e4m3 weights; the bias is fp32.  Error:
|got - ref| / max(1, |ref|) with got = (hi + lo) * 2^out_exp.  Bars: the operator bars of tests/test_gpu_conv_op.py (autosteer_cases.X3_BAR / FP16_BAR);
e4m3 weights on an fp16 engine: the 3e-3 of tests/test_conv_emulated.py::test_fp8_weight_storage, and the closeness to the (hi, lo) run as there."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from autosteer_cases import FP16_BAR, X3_BAR, pair_round, rel

FP8_ON_FP16_BAR = 3e-3                      # test_fp8_weight_storage
FP8_TO_PLAIN = {"fp16x3": 2e-5, "fp16": 2e-3}   # the e4m3 run against the (hi, lo) run of the same values, as test_fp8_weight_storage has it
PREC = {"fp16": 0, "fp16x3": 1}
NONE, SILU = 0, 2
RES_ADD, RES_MULADD = 1, 2
GENERIC = [(t, -1, -1) for t in range(4)]           # (tile, bk, nsplit); -1 = the dispatch rule
HALO = [(100 + t, -1, -1) for t in range(5)]
RULE = (-1, -1, -1)
f32 = np.float32
WORST = {}                                           # group -> largest error seen (printed by every check)


def _h(a):
    return np.asarray(a, f32).astype(np.float16).astype(f32)


def stored(v, precision, exp=0):
    """what the engine holds of v under exponent exp"""
    if precision == "fp16":
        assert exp == 0
        return _h(v)
    s = f32(2.0 ** -exp)
    return (pair_round(np.asarray(v, f32) * s).astype(np.float64) * 2.0 ** exp)


def planes(v, precision, exp=0):
    """the (hi, lo) bit planes of v stored under exp (lo: zeros in an fp16 engine)"""
    s = np.asarray(v, f32) * f32(2.0 ** -exp)
    hi = s.astype(np.float16)
    lo = (s - hi.astype(f32)).astype(np.float16) if precision == "fp16x3" else np.zeros_like(hi)
    return hi, lo


def bar_of(precision, fp8=False):
    if precision == "fp16x3":
        return X3_BAR
    return FP8_ON_FP16_BAR if fp8 else FP16_BAR


def q_e4m3(w):
    """oracle/autodrive.py quantize_fp8_e4m3 on one weight tensor: per-output-row symmetric OCP e4m3, returned de-quantised (fp32)."""
    from oracle import autodrive

    return autodrive.quantize_fp8_e4m3({"x.weight": w})["x.weight"]


def layer(seed, precision, cin, cout, h, w, ks, fp8=False):
    """standard-normal input, He-scaled weights, 0.1 * normal bias -- the input and the weights already what the engine will hold of them"""
    rng = np.random.default_rng(seed)
    q = pair_round if precision == "fp16x3" else _h
    x = q(rng.standard_normal((cin, h, w)))
    wt = (rng.standard_normal((cout, cin, ks, ks)) * np.sqrt(2.0 / (cin * ks * ks))).astype(f32)
    wt = q_e4m3(wt) if fp8 else q(wt)
    b = (rng.standard_normal(cout) * 0.1).astype(f32)
    return rng, x, wt, b


def reference(x, wt, b, stride=1, act=NONE, res_mode=0, res=None, post_act=NONE):
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64))   # noqa: E731
    y = F.conv2d(d(x)[None], d(wt), d(b), stride=stride, padding=wt.shape[-1] // 2)[0]
    if act == SILU:
        y = F.silu(y)
    if res_mode == RES_ADD:
        y = y + d(res)
    elif res_mode == RES_MULADD:
        y = y * d(res) + d(res)
    if post_act == SILU:
        y = F.silu(y)
    return y.numpy()


def value(hi, lo, out_exp=0):
    return (hi.astype(np.float64) + lo.astype(np.float64)) * 2.0 ** out_exp


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint16), np.ascontiguousarray(b).view(np.uint16))


def note(group, what, err, bar):
    WORST[group] = max(WORST.get(group, 0.0), err)
    print(f"conv_forms {group} {what}: {err:.2e} (bar {bar:.1e}; largest of {group} so far {WORST[group]:.2e})")


def run_cfgs(lib, group, what, precision, cfgs, want, x, wt, b, fp8=False, sl=None, **kw):
    """one layer through every (tile, bk, nsplit) of cfgs: each result (its slice sl of the destination) within the bar of `want`; returns the planes of the last"""
    bar = bar_of(precision, fp8)
    pr = PREC[precision] | (16 if fp8 else 0)
    for tile, bk, nsplit in cfgs:
        hi, lo = lib.op_conv2d_forms(x, wt, b, precision=pr, tile=tile, bk=bk, nsplit=nsplit, **kw)
        got = value(hi, lo, kw.get("out_exp", 0))
        got = got if sl is None else got[sl]
        assert got.shape == want.shape and np.isfinite(got).all(), (what, tile, bk, nsplit)
        err = rel(got, want)
        note(group, f"{what} {precision}{'+e4m3' if fp8 else ''} tile {tile} bk {bk} nsplit {nsplit}", err, bar)
        assert err <= bar, (what, precision, tile, bk, nsplit, err, np.unravel_index(np.argmax(np.abs(got - want) / np.maximum(1.0, np.abs(want))), want.shape))
    return hi, lo


# ------------------------------------------------------------------------------------------------ A: 3x3 stride 2 + SiLU
#          cin, cout, h, w: one K block and M = 128; 30 pixels, odd output width, ragged channels on both sides; M = 120; bk 64 does not divide 96, ragged channel tile
A_ROWS = [(16, 32, 16, 32), (24, 40, 10, 12), (64, 64, 12, 40), (96, 72, 8, 16)]


def a_cfgs(row):
    cfgs = [RULE] + GENERIC
    if row == (64, 64, 12, 40):   # nine taps x one (bk 64) or two (bk 32) blocks: 9 / 18 steps in 1, 2, 3 slices -- unequal ones at 9 in 2
        cfgs += [(2, bk, ns) for bk in (32, 64) for ns in (1, 2, 3)] + [(0, 64, 3), (3, 32, 2)]
    if row == (96, 72, 8, 16):
        cfgs += [(1, 64, -1), (2, 64, 2)]   # 64 does not divide the 96 padded channels: the 32-channel K block takes over
    return cfgs


def check_stride2(lib, precision, row):
    cin, cout, h, w = row
    _, x, wt, b = layer(1000 + cin + cout, precision, cin, cout, h, w, 3)
    want = reference(x, wt, b, stride=2, act=SILU)
    assert want.shape == (cout, h // 2, w // 2)
    run_cfgs(lib, "A", f"s2 {cin}->{cout} {h}x{w}", precision, a_cfgs(row), want, x, wt, b, ks=3, stride=2, act=SILU)


TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]


def check_stride2_tap(lib, ky, kx):
    """64 -> 64 on 8x40, fp16x3, integer inputs, a non-symmetric channel permutation on the single tap (ky, kx): the result IS
    x[perm][2y + ky - 1, 2x + kx - 1] (zero outside the map), to the bit -- any swap of y / x, stride / tap or Hin / Win moves a value."""
    cin = cout = 64
    x = np.arange(cin * 8 * 40, dtype=f32).reshape(cin, 8, 40) % 97 - 48.0
    perm = [(c * 7 + 3) % cin for c in range(cout)]
    wt = np.zeros((cout, cin, 3, 3), f32)
    for c in range(cout):
        wt[c, perm[c], ky, kx] = 1.0
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    want = xp[perm][:, ky:ky + 8:2, kx:kx + 40:2]
    assert want.shape == (cout, 4, 20)
    for tile in (-1, 3):
        hi, lo = lib.op_conv2d_forms(x, wt, np.zeros(cout, f32), ks=3, stride=2, precision=1, tile=tile)
        got = hi.astype(f32) + lo.astype(f32)
        assert np.array_equal(got, want), (ky, kx, tile, np.argwhere(got != want)[:4])


def check_stride2_refusals(lib):
    z = lambda *s: np.zeros(s, f32)   # noqa: E731
    with pytest.raises((lib.VpError, ValueError), match="even maps"):
        lib.op_conv2d_forms(z(32, 9, 12), z(32, 32, 3, 3), z(32), ks=3, stride=2, precision=1)
    with pytest.raises((lib.VpError, ValueError), match="strided conv: 3x3"):
        lib.op_conv2d_forms(z(32, 8, 16), z(32, 32, 1, 1), z(32), ks=1, stride=2, precision=1)


A_FP8_ROWS = [(24, 40, 10, 12), (64, 64, 12, 40)]


def check_stride2_fp8(lib, precision, row):
    cin, cout, h, w = row
    _, x, wt, b = layer(1100 + cin + cout, precision, cin, cout, h, w, 3, fp8=True)
    want = reference(x, wt, b, stride=2, act=SILU)
    hi, lo = run_cfgs(lib, "A", f"s2 {cin}->{cout} {h}x{w}", precision, [RULE], want, x, wt, b, fp8=True, ks=3, stride=2, act=SILU)
    ph, pl = lib.op_conv2d_forms(x, wt, b, ks=3, stride=2, act=SILU, precision=PREC[precision])   # the same values as (hi, lo) fp16 planes
    assert rel(value(hi, lo), value(ph, pl)) <= FP8_TO_PLAIN[precision]


# ------------------------------------------------------------------------------------------------ B: the CTX gate SiLU(SiLU(conv) * r + r)
B_ROWS = [(32, 64, 8, 16), (48, 40, 11, 21)]


def b_cfgs(row):
    cfgs = [RULE] + GENERIC
    if row == (32, 64, 8, 16):   # the other map reaches the halo kernel by rule
        cfgs += HALO
    return cfgs + [(2, -1, 1), (2, -1, 2), (103, -1, 1), (103, -1, 2)]   # two K slices: splitk_finish_kernel carries the post-activation


def gate_layer(precision, row, fp8=False):
    cin, cout, h, w = row
    rng, x, wt, b = layer(2000 + cin + cout, precision, cin, cout, h, w, 3, fp8=fp8)
    r = (pair_round if precision == "fp16x3" else _h)(rng.standard_normal((cout, h, w)))
    want = reference(x, wt, b, act=SILU, res_mode=RES_MULADD, res=r, post_act=SILU)
    plain = reference(x, wt, b, act=SILU, res_mode=RES_MULADD, res=r)
    assert rel(plain, want) > 100 * FP16_BAR     # precondition: a dropped post-activation cannot pass
    return x, wt, b, r, want, plain


def check_gate(lib, precision, row):
    x, wt, b, r, want, plain = gate_layer(precision, row)
    what = f"gate {row[0]}->{row[1]} {row[2]}x{row[3]}"
    run_cfgs(lib, "B", what, precision, b_cfgs(row), want, x, wt, b, ks=3, act=SILU, res_mode=RES_MULADD, res=r, post_act=SILU)
    run_cfgs(lib, "B", what + " post_act 0", precision, [RULE, (2, -1, 2)], plain, x, wt, b, ks=3, act=SILU, res_mode=RES_MULADD, res=r)


def check_gate_fp8(lib, precision):
    x, wt, b, r, want, _ = gate_layer(precision, B_ROWS[0], fp8=True)
    run_cfgs(lib, "B", "gate 32->64 8x16", precision, [RULE], want, x, wt, b, fp8=True, ks=3, act=SILU, res_mode=RES_MULADD, res=r, post_act=SILU)


# ------------------------------------------------------------------------------------------------ C: slice stores
def dst_pattern(rng, precision, c, h, w):
    return (pair_round if precision == "fp16x3" else _h)(rng.standard_normal((c, h, w)))


def assert_untouched(hi, lo, init, sl, precision, exp=0):
    """every channel outside sl holds the (hi, lo) bits of the pattern it started with"""
    ih, il = planes(init, precision, exp)
    keep = np.ones(init.shape[0], bool)
    keep[sl] = False
    assert same_bits(hi[keep], ih[keep]) and same_bits(lo[keep], il[keep]), np.argwhere(hi[keep].view(np.uint16) != ih[keep].view(np.uint16))[:4]


# name -> (cin, cout, h, w, ks, stride, dst_c, dst_off, res_off, [(precision, fp8, cfgs)])
C_CASES = {
    # C3K2 conv1: in fp16 by rule the register epilogue; tiles 0 - 3 compute 128 / 64 weight rows, more than the slice: padding rows must not land
    "conv1": (64, 64, 7, 19, 1, 1, 96, 0, None, [(p, False, [RULE] + GENERIC) for p in ("fp16x3", "fp16")]),
    # C3K conv2, p5.3.cv2 into head.cat: the LAST slice of the tensor
    "conv2": (64, 32, 7, 19, 1, 1, 64, 32, None, [(p, False, GENERIC + [(2, 32, 2), (1, 32, 2)]) for p in ("fp16x3", "fp16")] + [("fp16x3", True, [RULE]), ("fp16", True, [RULE])]),
    "fpn.h3": (32, 32, 16, 32, 3, 2, 96, 0, None, [(p, False, [RULE]) for p in ("fp16x3", "fp16")]),
    "residual": (32, 32, 8, 16, 3, 1, 96, 64, 32, [(p, False, [RULE, (1, -1, -1), (3, -1, -1)] + HALO + [(3, -1, 2), (102, -1, 2)]) for p in ("fp16x3", "fp16")]),
    "residual ragged": (32, 32, 11, 21, 3, 1, 96, 64, 32, [(p, False, [RULE]) for p in ("fp16x3", "fp16")]),
}
C_IDS = [(name, v) for name, c in C_CASES.items() for v in range(len(c[-1]))]


def check_slice(lib, name, variant, exps=(0, 0, 0), group="C", flagged_zero=False):
    cin, cout, h, w, ks, stride, dst_c, dst_off, res_off, variants = C_CASES[name]
    precision, fp8, cfgs = variants[variant]
    in_exp, res_exp, out_exp = exps
    rng, x, wt, b = layer(3000 + sum(ord(ch) for ch in name), precision, cin, cout, h, w, ks, fp8=fp8)
    oh, ow = h // stride, w // stride
    init = dst_pattern(rng, precision, dst_c, oh, ow)
    sl = slice(dst_off, dst_off + cout)
    kw = dict(ks=ks, stride=stride, act=SILU, dst=init, dst_off=dst_off, in_exp=in_exp, res_exp=res_exp, out_exp=out_exp)
    r = None
    if res_off is not None:   # the Residual block: x + SiLU(conv(..)), x read back from its slice of the destination (stored under the destination's exponent)
        kw.update(res_mode=RES_ADD, res_off=res_off)
        r = stored(init[res_off:res_off + cout], precision, out_exp)
    want = reference(stored(x, precision, in_exp), wt, b, stride=stride, act=SILU, res_mode=RES_ADD if r is not None else 0, res=r)
    bar = bar_of(precision, fp8)
    pr = PREC[precision] | (16 if fp8 else 0) | (64 if flagged_zero else 0)
    out = []
    for tile, bk, nsplit in cfgs:
        hi, lo = lib.op_conv2d_forms(x, wt, b, precision=pr, tile=tile, bk=bk, nsplit=nsplit, **kw)
        assert hi.shape == (dst_c, oh, ow)
        got = value(hi, lo, out_exp)
        err = rel(got[sl], want)
        note(group, f"slice {name} {precision}{'+e4m3' if fp8 else ''} exps {exps} tile {tile} bk {bk} nsplit {nsplit}", err, bar)
        assert np.isfinite(got).all() and err <= bar, (name, precision, tile, bk, nsplit, err)
        assert_untouched(hi, lo, init, sl, precision, out_exp)
        out.append((hi, lo))
    return out


# ------------------------------------------------------------------------------------------------ D: under the activation scale (fp16x3)
D_EXPS = [(3, -2, 5), (-4, 6, -3)]


def check_scaled(lib, form, exps):
    """the A, B and C-residual forms with exponents (in, res, out): (hi + lo) * 2^out_exp within X3_BAR of the same fp64 reference on the operands as stored"""
    ie, re_, oe = exps
    if form == "A":
        cin, cout, h, w = A_ROWS[2]
        _, x, wt, b = layer(4001, "fp16x3", cin, cout, h, w, 3)
        want = reference(stored(x, "fp16x3", ie), wt, b, stride=2, act=SILU)
        run_cfgs(lib, "D", "s2 64->64 12x40", "fp16x3", [RULE, (2, 32, 2)], want, x, wt, b, ks=3, stride=2, act=SILU, in_exp=ie, res_exp=re_, out_exp=oe)
    elif form == "B":
        cin, cout, h, w = B_ROWS[0]
        rng, x, wt, b = layer(4002, "fp16x3", cin, cout, h, w, 3)
        r = pair_round(rng.standard_normal((cout, h, w)))
        want = reference(stored(x, "fp16x3", ie), wt, b, act=SILU, res_mode=RES_MULADD, res=stored(r, "fp16x3", re_), post_act=SILU)
        run_cfgs(lib, "D", "gate 32->64 8x16", "fp16x3", [RULE, (2, -1, 2), (103, -1, 1), (103, -1, 2)], want, x, wt, b, ks=3, act=SILU, res_mode=RES_MULADD, res=r,
                 post_act=SILU, in_exp=ie, res_exp=re_, out_exp=oe)
    else:
        check_slice(lib, "residual", 0, exps=exps, group="D")


def check_scaled_zero_exponents(lib):
    """a flagged engine (VP_ACT_SCALE in the precision argument) with every exponent 0 stores the unflagged engine's bits, in each of the three forms"""
    cin, cout, h, w = A_ROWS[2]
    _, x, wt, b = layer(4001, "fp16x3", cin, cout, h, w, 3)
    kw = dict(ks=3, stride=2, act=SILU)
    p, f = lib.op_conv2d_forms(x, wt, b, precision=1, **kw), lib.op_conv2d_forms(x, wt, b, precision=1 | 64, **kw)
    assert same_bits(p[0], f[0]) and same_bits(p[1], f[1])
    cin, cout, h, w = B_ROWS[0]
    rng, x, wt, b = layer(4002, "fp16x3", cin, cout, h, w, 3)
    r = pair_round(rng.standard_normal((cout, h, w)))
    for tile, ns in ((-1, -1), (2, 2)):
        kw = dict(ks=3, act=SILU, res_mode=RES_MULADD, res=r, post_act=SILU, tile=tile, nsplit=ns)
        p, f = lib.op_conv2d_forms(x, wt, b, precision=1, **kw), lib.op_conv2d_forms(x, wt, b, precision=1 | 64, **kw)
        assert same_bits(p[0], f[0]) and same_bits(p[1], f[1])
    plain = check_slice(lib, "residual", 0, group="D")
    flagged = check_slice(lib, "residual", 0, group="D", flagged_zero=True)
    for (ph, pl), (fh, fl) in zip(plain, flagged):
        assert same_bits(ph, fh) and same_bits(pl, fl)


# ------------------------------------------------------------------------------------------------ E: refusals, when the plan is built
def check_refusals(lib):
    z = lambda *s: np.zeros(s, f32)   # noqa: E731
    x, wt, b = z(32, 8, 16), z(32, 32, 3, 3), z(32)
    with pytest.raises((lib.VpError, ValueError), match="residual needs the destination's row pitch and map size"):     # a fresh residual (pitch 32) with a slice destination (pitch 96)
        lib.op_conv2d_forms(x, wt, b, ks=3, act=SILU, res_mode=RES_ADD, res=z(32, 8, 16), dst=z(96, 8, 16), dst_off=64, precision=1)
    with pytest.raises((lib.VpError, ValueError), match="residual needs the destination's row pitch and map size"):     # a residual of another map size
        lib.op_conv2d_forms(x, wt, b, ks=3, act=SILU, res_mode=RES_ADD, res=z(32, 4, 8), precision=1)
    with pytest.raises((lib.VpError, ValueError), match="input cannot be a slice"):
        lib.op_conv2d_forms(x, wt, b, ks=3, act=SILU, in_c=64, in_off=32, precision=1)
    lib.op_conv2d_forms(x, wt, b, ks=3, act=SILU, res_mode=RES_ADD, res=z(32, 8, 16), precision=1)                        # the well-formed neighbours build and run
    lib.op_conv2d_forms(x, wt, b, ks=3, act=SILU, res_mode=RES_ADD, res_off=32, dst=z(96, 8, 16), dst_off=64, precision=1)
