"""The quantisation rule of the e4m3 MFMA layers (include/vp_hip.h "FP8 MFMA ENGINES") restated in numpy, and the cases the three suites share
(tests/test_f8_host.py, tests/test_f8_emulated.py, tests/test_gpu_f8.py).  Nothing here looks at the library's code: the encoder searches the decoded
table of all 256 codes."""
import numpy as np

EXPS = (-8, 0, 3, 8)
# (cin, cout, h, w) of the operator cases; the device suite adds the last two (three chunks x three row tiles; two channel tiles)
SHAPES = ((64, 64, 8, 16), (128, 64, 9, 17), (64, 128, 16, 32))
SHAPES_GPU = SHAPES + ((192, 64, 24, 16), (128, 128, 16, 32))


def e4m3_decode(codes):
    """OCP e4m3fn codes -> float64 (0x7f / 0xff: NaN)"""
    c = np.asarray(codes).astype(np.int64)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e - 10.0))
    mag = np.where((c & 0x7f) == 0x7f, np.nan, mag)
    return np.where(c & 0x80, -mag, mag)


_GRID = e4m3_decode(np.arange(0x7f))          # the 127 finite magnitudes, ascending: code == index


def e4m3_encode(v):
    """float64 values -> codes: nearest grid value, ties to the even code, beyond 448 (the infinities included) +-448, NaN -> 0x7f | sign, signed zeros"""
    v = np.asarray(v, np.float64)
    a = np.abs(v)
    hi = np.clip(np.searchsorted(_GRID, a, side="left"), 1, 126)      # first grid value >= a
    lo = hi - 1
    dl, dh = a - _GRID[lo], _GRID[hi] - a
    code = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(a >= 448.0, 126, code)
    code = np.where(np.isnan(v), 0x7f, code)
    return (code | np.where(np.signbit(v), 0x80, 0)).astype(np.uint8)


def quantize_act(f16, qexp):
    """the activation rule: fp16 values -> e4m3(x * 2^-qexp) codes (the scaling is exact in float64)"""
    with np.errstate(invalid="ignore"):
        return e4m3_encode(np.asarray(f16, np.float16).astype(np.float64) * 2.0 ** -qexp)


def encode_weight_rows(w):
    """[rows][per_row] fp32 -> (codes, fp32 row scales S_n = amax_n / 448): the rule of vp_fp8_encode_rows in float32 arithmetic"""
    w = np.asarray(w, np.float32)
    amax = np.abs(w).max(axis=1)
    s = np.where(amax > 0, amax / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    return e4m3_encode((w / s[:, None]).astype(np.float32)), s


def gelu(x):
    from math import erf

    return 0.5 * x * (1.0 + np.vectorize(erf)(x / np.sqrt(2.0)))


def layer_ref(x, weight, bias, act, qexp):
    """the layer: quantised operands, float64 sum, y_n = fl32(acc_n * fl32(S_n * 2^qexp)) + bias_n, activation -- as float64, BEFORE the fp16 store
    (acc is exact in float64 here; the kernel's is an fp32 accumulator, which the callers' bounds allow for)"""
    cout, cin = weight.shape[:2]
    xq = e4m3_decode(quantize_act(np.asarray(x, np.float32).astype(np.float16), qexp))
    codes, s = encode_weight_rows(np.asarray(weight, np.float32).reshape(cout, -1))
    wq = e4m3_decode(codes).reshape(weight.shape)
    h, w = x.shape[1:]
    xp = np.zeros((cin, h + 2, w + 2))
    xp[:, 1:-1, 1:-1] = xq
    acc = np.zeros((cout, h, w))
    for ky in range(3):
        for kx in range(3):
            acc += np.einsum("oc,chw->ohw", wq[:, :, ky, kx], xp[:, ky:ky + h, kx:kx + w])
    scale = (s * np.float32(2.0 ** qexp)).astype(np.float32)
    y = (acc.astype(np.float32) * scale[:, None, None]).astype(np.float32).astype(np.float64) + np.asarray(bias, np.float32).astype(np.float64)[:, None, None]
    return gelu(y) if act else y


def exact_case(cin, cout, h, w, seed=0):
    """(a): integer activations in [-4, 4], integer weights in [-7, 7] with +-7 in every row (S_n = 2^-6, every code exact), integer bias -- every partial
    sum is an integer below 2^24, so any summation order gives the same fp32 accumulator.  Asymmetric in channel and in position: the values come from a
    seeded generator, plus a ramp over the input channels on the weights' centre tap and one over x on the activations."""
    rng = np.random.default_rng(1000 + seed)
    x = rng.integers(-4, 5, (cin, h, w)).astype(np.float32)
    x[:, :, 0] = np.clip(np.arange(cin) % 9 - 4, -4, 4)[:, None]
    x[0, 0, :] = np.arange(w) % 5
    wt = rng.integers(-7, 8, (cout, cin, 3, 3)).astype(np.float32)
    wt[:, :, 1, 1] = (np.arange(cin)[None, :] + 3 * np.arange(cout)[:, None]) % 15 - 7
    wt[:, 0, 0, 0] = np.where(np.arange(cout) % 2 == 0, 7, -7)
    b = rng.integers(-20, 21, cout).astype(np.float32)
    return x, wt, b


def random_case(cin, cout, h, w, seed=0):
    """(b): Gaussian activations of a few units, kaiming-sized weights, a bias of the output's size"""
    rng = np.random.default_rng(2000 + seed)
    x = (rng.standard_normal((cin, h, w)) * 2.0).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9.0 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    return x, wt, b


def check_exact(op, shape, seed=0):
    x, wt, b = exact_case(*shape, seed=seed)
    ref = layer_ref(x, wt, b, 0, 0)
    assert np.abs(ref).max() < 65504 and np.array_equal(ref, np.round(ref))
    got = op(x, wt, b, act=0, qexp=0)
    assert got.dtype == np.float16
    assert np.array_equal(got.view(np.uint16), ref.astype(np.float16).view(np.uint16)), (shape, int((got != ref.astype(np.float16)).sum()))


def check_random(op, shape, qexp, act, seed=0):
    """within 1.5e-3 * max(1, |ref|) of the restatement: one fp16 output rounding plus accumulation order (tests/test_gpu_conv_op.py's VP_FP16 bound)"""
    x, wt, b = random_case(*shape, seed=seed)
    ref = layer_ref(x, wt, b, act, qexp)
    got = op(x, wt, b, act=act, qexp=qexp).astype(np.float64)
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print(f"conv3x3_f8 {shape} qexp {qexp} act {act}: max err {err.max():.3e} (bound 1.5e-3)")
    assert (err <= 1.5e-3).all(), (shape, qexp, act, float(err.max()))


def check_refusals(op):
    import pytest

    for cin, cout in ((64, 96), (32, 64)):
        x, wt, b = random_case(cin, cout, 8, 16)
        with pytest.raises(ValueError, match="halo tile 13"):
            op(x, wt, b)
