"""Shared by tests/test_range_hist_emulated.py and tests/test_gpu_range_survey.py: the operator cases of act_exp_hist_kernel (vp_op_exp_hist) and the numpy
oracle of the range survey.  The oracle is floor(log2 |float32(hi) + float32(lo)|) through np.frexp; every comparison is exact (integer counters)."""
import numpy as np

BINS, EXP_MIN = 40, -24

# (c, c_pitch, h, w): pad exclusion and count == c*h*w at 1x1 and 5x7; a channel count that is no multiple of 8 octets' pitch; a pixel count that is
# neither a block (256 threads) nor a wave (64) multiple, on six blocks
SHAPES = ((3, 32, 1, 1), (3, 32, 5, 7), (40, 64, 3, 50), (32, 32, 17, 19))


def oracle(hi, lo, c):
    """-> (bins int64 [40], zeros, nonfinite, count, absmax float32) of the stored values of channels [0, c)"""
    x = hi[..., :c].astype(np.float32)
    if lo is not None:
        x = x + lo[..., :c].astype(np.float32)
    return stats(x)


def stats(x):
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    fin = np.isfinite(x)
    a = np.abs(x[fin])
    nz = a[a != 0]
    e = np.frexp(nz)[1].astype(np.int64) - 1            # |x| = m * 2^e', m in [0.5, 1): floor(log2 |x|) = e' - 1
    assert e.size == 0 or (e.min() >= EXP_MIN and e.max() <= EXP_MIN + BINS - 1), (e.min(), e.max())
    bins = np.bincount(e - EXP_MIN, minlength=BINS).astype(np.int64)
    return bins, int(a.size - nz.size), int(x.size - a.size), int(x.size), np.float32(a.max() if a.size else 0.0)


def planes(c, pitch, h, w, two, seed, one_bin=False):
    """Seeded (hi, lo) fp16 planes [h][w][pitch]; lo is None for a single-plane tensor.  Values spread over every fp16 binade, with the special values
    below written over the first real elements in a seeded order; the pad channels hold values that would show up if they were counted.
    one_bin: every real value in [1, 2) -- the contention case (one counter takes every element)."""
    rng = np.random.default_rng(seed)
    n = h * w * c
    if one_bin:
        v = rng.uniform(1.0, 1.999, n).astype(np.float32)
    else:
        v = (rng.uniform(0.5, 1.0, n) * np.exp2(rng.integers(-25, 17, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)   # 2^-26 .. 2^16: under- and overflow of fp16 included
        v = np.clip(v, -65504.0, 65504.0)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16) if two else None
    if not one_bin:
        f16 = np.float16
        special = [(f16(0.0), f16(0.0)), (f16(-0.0), f16(-0.0)), (f16(2.0 ** -24), f16(0.0)), (f16(-2.0 ** -20), f16(0.0)), (f16(65504.0), f16(0.0)),
                   (f16(np.inf), f16(0.0)), (f16(-np.inf), f16(0.0)), (f16(np.nan), f16(0.0)), (f16(-65504.0), f16(0.0)), (f16(2.0 ** -15), f16(0.0))]
        if two:
            special += [(f16(1.0), f16(-2.0 ** -12)),       # the sum lies below 1: exponent -1, not hi's exponent 0
                        (f16(-4.0), f16(2.0 ** -9)), (f16(2.0 ** -14), f16(-2.0 ** -24)), (f16(0.5), f16(2.0 ** -24))]
        order = rng.permutation(len(special))
        where = rng.permutation(n)[: len(special)]
        for k, pos in enumerate(where):
            s = special[order[k]]
            hi[pos] = s[0]
            if two:
                lo[pos] = s[1]
    hp = np.full((h, w, pitch), np.float16(60000.0), np.float16)
    hp[..., c + (pitch - c) // 2:] = np.float16(np.inf)
    hp[..., :c] = hi.reshape(h, w, c)
    lp = None
    if two:
        lp = np.full((h, w, pitch), np.float16(-3.0), np.float16)
        lp[..., :c] = lo.reshape(h, w, c)
    return hp, lp


def operator_cases():
    """-> [(id, hi, lo, c)]"""
    out = []
    for si, (c, pitch, h, w) in enumerate(SHAPES):
        for two in (False, True):
            hi, lo = planes(c, pitch, h, w, two, 100 + 2 * si + two)
            out.append((f"c{c}p{pitch}_{h}x{w}_{'x2' if two else 'x1'}", hi, lo, c))
    for (c, pitch, h, w), two in (((32, 32, 17, 19), True), ((40, 64, 3, 50), False)):
        hi, lo = planes(c, pitch, h, w, two, 7, one_bin=True)
        out.append((f"one_bin_c{c}_{h}x{w}_{'x2' if two else 'x1'}", hi, lo, c))
    return out


def check_operator(lib, hi, lo, c):
    bins, zeros, nonfinite, count, _ = oracle(hi, lo, c)
    got = lib.op_exp_hist(hi, lo, c)
    print("bins", got[0].tolist(), "zeros", got[1], "count", got[2], "| oracle", bins.tolist(), zeros, count, "non-finite", nonfinite)
    assert np.array_equal(got[0], bins) and got[1] == zeros and got[2] == count == c * hi.shape[0] * hi.shape[1]
    assert int(bins.sum()) + zeros + nonfinite == count
    again = lib.op_exp_hist(hi, lo, c)
    assert np.array_equal(again[0], got[0]) and again[1:] == got[1:]
