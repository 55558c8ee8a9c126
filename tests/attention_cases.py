"""The C2PSA / SPPF kernel family of kernels_autodrive.hip (attention_kernel, attention_block_kernel<4>, sppf_pool_kernel, maxpool5_kernel, chan_copy_kernel,
dwconv_plain_kernel) at the token counts the plans launch, at the kernels' limits and at the value edges of the softmax -- one kernel at a time through the entry
points of tests/emul/harness_entries.hpp.  Shared by the emulated (tests/test_attention_emulated.py) and the device (tests/test_gpu_attention.py) suites: the
bodies take a backend of tests/emul/backends.py; same shapes, same bars.  TEST INFRASTRUCTURE ONLY.

ATTENTION.  Reference: fp64 numpy, out = softmax(q k^T * float(scale)) v per head, q, k, v the values the planes HOLD (hi + lo, or hi alone).  Every case's
reference must be finite (checked in reference()).  Bar, per case, from the reference and the inputs only:

    bar = 4 * err32 + storage

  * err32: the largest difference between the same formula evaluated in fp32 numpy and the fp64 result;
  * storage: what the output format cannot hold -- two planes: max(2^-22 * |out|max, 2^-25) (the second term is half the quantum 2^-24 of a subnormal lo
    plane: it takes over when |out| < 2^-3); one plane: 2^-11 * |out|max;
  * the factor 4: the kernel sums the value pass as 32 interleaved slices (fma chains) added in slice order and the logits as one fma chain; numpy sums
    in its own blocked order -- the two fp32 results differ from fp64 by amounts of the same size, not by the same amount.
Under the activation scale (a tensor t stored as t * 2^-s, the launch given scale * 2^(2s)) the reference is taken from the stored planes times 2^s, the result
compared as out * 2^s, and the storage term -- a property of the stored numbers -- is scaled by 2^s with it.
Measured (table() prints every row): both kernels, on the emulation and on the device alike, at 0.08 - 0.79 of the bar on (hi, lo) planes -- largest at gain 2^-6
and exponent 6, where the subnormal lo plane is the whole error -- and at 0.35 - 0.81 on a single plane, where the fp16 rounding of the output is.
The copy of v (vout) must equal v within 1e-6 (tests/test_kernels_emulated.py::test_maxpool5_and_attention_kernels); rows behind T and channels behind
heads * dv of the output arrays, which the launch does not own, must keep their bits.  out and vout share ONE row pitch (launch_attention refuses anything else).

SPPF / MAX-POOL.  Bit-exact on the values (hi + lo) against three chained F.max_pool2d(5, 1, 2) of the stored values: a maximum of stored numbers is a
stored number.  No bar."""
import ctypes as ct

import numpy as np
import torch
import torch.nn.functional as F

f32, f64, f16 = np.float32, np.float64, np.float16
NAN16 = 0x7E01          # canary of the read side: a NaN in every half the launch must not read
CANARY = 0x5A5A         # canary of the write side (fp16 203.25)
RESULTS = {}            # row -> {backend: (error, bar)}, the worst error / bar of the row; printed when a module is done (table())
_REF = {}               # case key -> reference, computed once


# ------------------------------------------------------------------------------------------------ common
def split16(x):
    x = np.asarray(x, f32)
    hi = x.astype(f16)
    return np.ascontiguousarray(hi), np.ascontiguousarray((x - hi.astype(f32)).astype(f16))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def filled(shape, pattern):
    return np.full(shape, pattern, np.uint16).view(f16)


def note(row, be, err, bar):
    got = RESULTS.setdefault(row, {})
    if be.name not in got or err / bar > got[be.name][0] / got[be.name][1]:
        got[be.name] = (err, bar)
    print(f"attention_cases {be.name} {row}: {err:.3e} / bar {bar:.3e} = {err / bar:.2f}")


def table():
    if not RESULTS:
        return
    print("\nlargest measured error / bar per row (attention: |got - fp64|max against 4 * err32 + storage):")
    for row, got in RESULTS.items():
        print("  %-34s %s" % (row, "   ".join(f"{k}: {e:.2e} / {b:.2e} = {e / b:.2f}" for k, (e, b) in sorted(got.items()))))


def prepare(be):
    p, i = ct.c_void_p, ct.c_int
    be.emu_attention_pitched.argtypes = [p, p, i, i, i, i, i, ct.c_float, p, p, p, p, i, i, i, i]
    be.emu_attention.argtypes = [p, p, i, i, i, i, i, ct.c_float, p, p, p, p, i]
    return be


# ------------------------------------------------------------------------------------------------ attention: reference and bar
def storage(out_abs_max, planes):
    return max(2.0 ** -22 * out_abs_max, 2.0 ** -25) if planes == 2 else 2.0 ** -11 * out_abs_max


def reference(key, x64, x32, heads, dk, dv, scale):
    """(fp64 result [T][heads * dv], err32, the stored v [T][heads * dv] in fp64) of the stored qkv values x64 (x32: the same values in fp32), once per key"""
    if key in _REF:
        return _REF[key]
    per, s64, s32 = 2 * dk + dv, float(f32(scale)), f32(scale)
    out, v_all, err32 = [], [], 0.0
    for h in range(heads):
        q, k, v = (x64[:, h * per + a:h * per + b] for a, b in ((0, dk), (dk, 2 * dk), (2 * dk, per)))
        s = (q @ k.T) * s64
        e = np.exp(s - s.max(axis=1, keepdims=True))
        o = (e @ v) / e.sum(axis=1, keepdims=True)
        q3, k3, v3 = (x32[:, h * per + a:h * per + b] for a, b in ((0, dk), (dk, 2 * dk), (2 * dk, per)))
        s3 = (q3 @ k3.T) * s32
        e3 = np.exp(s3 - s3.max(axis=1, keepdims=True))
        o3 = (e3 @ v3) * (f32(1.0) / e3.sum(axis=1, keepdims=True, dtype=f32))
        assert o3.dtype == f32
        err32 = max(err32, float(np.abs(o3.astype(f64) - o).max()))
        out.append(o)
        v_all.append(v)
    out, v_all = np.concatenate(out, axis=1), np.concatenate(v_all, axis=1)
    assert np.isfinite(out).all(), key          # the reference-only precondition of every case
    _REF[key] = (out, err32, v_all)
    return _REF[key]


def launch(be, hi, lo, H, W, heads, dk, dv, scale, qblock, planes, pads=(8, 16, 3)):
    """one launch on arrays wider (qkv by pads[0] channels, out and vout by pads[1]) and longer (pads[2] rows: a last block of four queries reaches at most three
    rows behind T) than the views: NaNs where the launch must not read, canaries where it must not write.  Returns (rc, out, vout) -- the values (hi + lo,
    fp64) of the views; the canaries are checked here."""
    prepare(be)
    T, per, two = H * W, 2 * dk + dv, planes == 2
    QP, OP, R = heads * per + pads[0], heads * dv + pads[1], T + pads[2]
    q = [filled((R, QP), NAN16) for _ in range(planes)]
    q[0][:T, :heads * per] = hi
    if two:
        q[1][:T, :heads * per] = lo
    before = [a.copy() for a in q]
    o = [filled((R, OP), CANARY) for _ in range(2 * planes)]     # out hi [, lo], vout hi [, lo]
    ol, vh, vl = (o[1], o[2], o[3]) if two else (None, o[1], None)
    rc = be.emu_attention_pitched(q[0], q[1] if two else None, H, W, heads, dk, dv, scale, o[0], ol, vh, vl, qblock, QP, OP, OP)
    if rc:
        assert all((bits(a) == CANARY).all() for a in o), "a refused launch wrote"
        return rc, None, None
    for a, b in zip(q, before):
        assert np.array_equal(bits(a), bits(b)), "qkv was written"
    for a in o:
        assert (bits(a[T:]) == CANARY).all(), "rows behind T were written"
        assert (bits(a[:T, heads * dv:]) == CANARY).all(), "channels behind heads * dv were written"
    val = lambda h_, l_: h_[:T, :heads * dv].astype(f64) + (l_[:T, :heads * dv].astype(f64) if l_ is not None else 0.0)   # noqa: E731
    return 0, val(o[0], ol), val(vh, vl)


def stored(x, planes):
    """(hi, lo, fp64 values, fp32 values) the planes hold of x"""
    hi, lo = split16(x)
    if planes == 1:
        return hi, None, hi.astype(f64), hi.astype(f32)
    return hi, lo, hi.astype(f64) + lo.astype(f64), hi.astype(f32) + lo.astype(f32)


def run(be, row, key, x, H, W, heads, dk, dv, kernels=(4, 0), planes_list=(2, 1), scale=None, exp=0):
    """x (the values before storage, [T][heads * (2 dk + dv)]) through each kernel and plane form against the fp64 reference within the bar; exp: the
    activation-scale exponent s (x * 2^-s is stored, the launch gets scale * 2^(2s)).  Returns {(qblock, planes): (out, vout, reference)}."""
    scale = dk ** -0.5 if scale is None else scale
    res, m = {}, 2.0 ** exp
    for planes in planes_list:
        hi, lo, x64, x32 = stored(np.asarray(x, f32) * f32(1.0 / m), planes)
        want, err32, v = reference((key, planes), x64 * m, x32 * f32(m), heads, dk, dv, scale)
        bar = 4.0 * err32 + storage(float(np.abs(want).max()) / m, planes) * m
        for qblock in kernels:
            rc, out, vout = launch(be, hi, lo, H, W, heads, dk, dv, f32(scale) * f32(m * m), qblock, planes)
            assert rc == 0, (row, qblock, planes, rc)
            out, vout = out * m, vout * m
            assert np.isfinite(out).all(), (row, qblock, planes)
            err = float(np.abs(out - want).max())
            note(f"{row} q{qblock} {'hi+lo' if planes == 2 else 'hi'}", be, err, bar)
            assert err <= bar, (row, qblock, planes, err, bar, np.unravel_index(np.argmax(np.abs(out - want)), want.shape))
            assert np.abs(vout - v).max() <= 1e-6, (row, qblock, planes)
            res[qblock, planes] = (out, vout, want, bar)
    return res


def normal(seed, T, heads, dk, dv):
    return np.random.default_rng(seed).standard_normal((T, heads * (2 * dk + dv))).astype(f32)


# ------------------------------------------------------------------------------------------------ 1: the shapes the plans launch
def plan_shapes(lib):
    """(H, W, heads) of the attention launch of each network that has one, read from the engines' tensors (the attention output has heads * 64 channels)"""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    shapes = {}
    for kind, make in (("autodrive", synthetic.make_autodrive_state_dict), ("autospeed", synthetic.make_autospeed_state_dict), ("autosteer", synthetic.make_autosteer_state_dict)):
        eng = lib.Engine(kind, vw.pack_state_dict(make(0)), precision="fp16x3")
        try:
            found = [(h, w, c // 64) for n, c, h, w in eng.tensors() if n.endswith(".conv1.attn")]
        finally:
            eng.close()
        assert len(found) == 1 and found[0][2] >= 1, (kind, found)
        shapes[kind] = found[0]
    return shapes


def check_plan_shapes(be, lib):
    """every engine that has the block takes a 1024 x 512 input, so the three plans launch 16x32 with c_ / 64 = 2 heads; the 20x20 map is P5 of the detector's
    own 640 x 640 letterbox (vp_detect's default net size), which no engine plans today -- it is run as a shape of its own, with the plans' head count"""
    shapes = plan_shapes(lib)
    assert shapes["autodrive"] == (16, 32, 2) and set(shapes) == {"autodrive", "autospeed", "autosteer"}, shapes
    for H, W, heads in sorted(set(shapes.values()) | {(20, 20, shapes["autospeed"][2])}):
        run(be, f"plan {H}x{W}x{heads}", ("plan", H, W, heads), normal(100 + H, H * W, heads, 32, 64), H, W, heads, 32, 64)


# ------------------------------------------------------------------------------------------------ 2, 3: token counts and the block kernel's limit
#        T: 1, 3, 255, 256, 257, 258 (the only T = 2 mod 4 of the list: a last block of two queries), 323, 511, 513, 1760 (65536 bytes of LDS: the largest the block kernel takes)
EDGE_MAPS = [(1, 1), (1, 3), (15, 17), (16, 16), (1, 257), (6, 43), (17, 19), (7, 73), (27, 19), (40, 44)]
REFUSED_MAPS = [(41, 43), (32, 64)]     # 1763 and 2048 tokens


def check_token_edge(be, H, W):
    T = H * W
    res = run(be, f"edge T={T}", ("edge", T), normal(200 + T, T, 1, 32, 64), H, W, 1, 32, 64, planes_list=(2,) if T != 323 else (2, 1))
    if T == 1:      # one key: the probability is 1 and the output is v, to the bit
        for out, vout, _, _ in res.values():
            assert np.array_equal(out, vout)


def check_block_limit(be, H, W):
    """above 1760 tokens the block kernel is refused by return code and the per-query kernel computes the map"""
    T = H * W
    x = normal(300 + T, T, 1, 32, 64)
    hi, lo, _, _ = stored(x, 2)
    rc, _, _ = launch(be, hi, lo, H, W, 1, 32, 64, f32(32 ** -0.5), 4, 2)
    assert rc != 0
    run(be, f"limit T={T}", ("limit", T), x, H, W, 1, 32, 64, kernels=(0,), planes_list=(2,))


# ------------------------------------------------------------------------------------------------ 4: value edges at T = 323
VALUE_EDGES = ["gain 2^-6", "gain 4", "gain 8", "aligned key", "equal keys", "equal keys T=512", "common logit", "negative v"]


def check_value_edge(be, name):
    H, W, heads, dk, dv = (16, 32, 2, 32, 64) if name.endswith("T=512") else (17, 19, 2, 32, 64)
    T, per = H * W, 128
    x = normal(400, T, heads, dk, dv)
    kw = {}
    if name.startswith("gain"):       # |logit| up to ~5 * gain^2: gain 8 leaves a handful of keys per row above the underflow of expf
        x = x * f32({"gain 2^-6": 2.0 ** -6, "gain 4": 4.0, "gain 8": 8.0}[name])
    elif name == "aligned key":       # q[0] doubled so that the planted logit (16 |q0|^2 / sqrt(32) ~ 90) leaves the other keys below 2^-64 of the row
        for h in range(heads):
            x[0, h * per:h * per + dk] *= 2
            x[T - 1, h * per + dk:h * per + 2 * dk] = 4 * x[0, h * per:h * per + dk]
    elif name.startswith("equal keys"):
        for h in range(heads):
            x[:, h * per + dk:h * per + 2 * dk] = x[0, h * per + dk:h * per + 2 * dk]
    elif name == "common logit":      # every logit 32 * 16 / sqrt(32) = 90.5 > 88.7 = log(FLT_MAX): finite only through the row-maximum subtraction
        for h in range(heads):
            x[:, h * per:h * per + 2 * dk] = 4.0
    elif name == "negative v":
        for h in range(heads):
            x[:, h * per + 2 * dk:(h + 1) * per] = -np.abs(x[:, h * per + 2 * dk:(h + 1) * per]) - f32(0.5)
    res = run(be, name, ("value", name), x, H, W, heads, dk, dv, **kw)
    for (qblock, planes), (out, vout, want, bar) in res.items():
        if name == "aligned key":     # one-hot row: the output IS v[T - 1]
            assert np.abs(want[0] - vout[T - 1]).max() <= 2.0 ** -40                      # (reference only)
            assert np.abs(out[0] - vout[T - 1]).max() <= bar, (qblock, planes)
        if name.startswith("equal keys") or name == "common logit":   # uniform rows: the output is the mean of v
            mean = vout.mean(axis=0)
            assert np.abs(want - mean).max() <= 1e-12                                     # (reference only)
            assert np.abs(out - mean).max() <= bar, (qblock, planes)
        if name == "negative v":
            assert (out < 0).all()


# ------------------------------------------------------------------------------------------------ 5: the activation-scale form
ACT_EXPS = [-3, 3, 6]


def check_act_scale(be, s):
    run(be, f"act scale s={s}", ("scale", s), normal(500, 323, 2, 32, 64), 17, 19, 2, 32, 64, exp=s)


# ------------------------------------------------------------------------------------------------ 6: other head sizes (the per-query kernel)
HEAD_SIZES = [(16, 32), (8, 16)]


def check_head_size(be, dk, dv):
    x = normal(600 + dk, 323, 2, dk, dv)
    run(be, f"dk={dk} dv={dv}", ("heads", dk), x, 17, 19, 2, dk, dv, kernels=(0,))
    hi, lo, _, _ = stored(x, 2)
    rc, _, _ = launch(be, hi, lo, 17, 19, 2, dk, dv, f32(dk ** -0.5), 4, 2)
    assert rc != 0          # the block kernel is dk = 32, dv = 64 only


def check_pitch_refusal(be):
    """out and vout are indexed with ONE row pitch by both kernels: views of different pitches are refused, not written with the wrong one"""
    prepare(be)
    T, heads, dk, dv = 42, 1, 32, 64
    hi, lo, _, _ = stored(normal(650, T, heads, dk, dv), 2)
    for qblock in (4, 0):
        o = [filled((T, 72), CANARY) for _ in range(2)] + [filled((T, 80), CANARY) for _ in range(2)]
        assert be.emu_attention_pitched(hi, lo, 6, 7, heads, dk, dv, f32(0.18), o[0], o[1], o[2], o[3], qblock, 128, 72, 80) != 0
        assert all((bits(a) == CANARY).all() for a in o)


# ------------------------------------------------------------------------------------------------ 7: determinism
def check_determinism(be):
    prepare(be)
    H, W, heads, dk, dv = 16, 32, 2, 32, 64
    hi, lo, _, _ = stored(normal(700, H * W, heads, dk, dv), 2)
    for qblock in (4, 0):
        runs = []
        for _ in range(3):
            o = [np.zeros((H * W, heads * dv), f16) for _ in range(4)]
            assert be.emu_attention(hi, lo, H, W, heads, dk, dv, f32(dk ** -0.5), o[0], o[1], o[2], o[3], qblock) == 0
            runs.append(o)
        for o in runs[1:]:
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(o, runs[0])), qblock


# ------------------------------------------------------------------------------------------------ SPPF and max-pool
SPPF_MAPS = [(16, 32), (20, 20), (1, 1), (2, 3), (1, 512), (512, 1), (3, 170), (5, 13), (23, 22)]
SPPF_INPUTS = ["x1", "x2^-12", "x2^8", "shifted -50", "ties"]
NCH, SRC_C, DST_C = 64, 72, 4 * 64 + 8


def sppf_input(name, H, W):
    rng = np.random.default_rng(800 + H * 7 + W)
    if name == "ties":              # integers in [-3, 3]: most windows hold their maximum several times
        return rng.integers(-3, 4, (H, W, SRC_C)).astype(f32)
    x = rng.standard_normal((H, W, SRC_C)).astype(f32)
    if name == "shifted -50":       # every value negative: a maximum that starts from zero shows
        assert (x - 50 < 0).all()
        return x - f32(50)
    return x * f32({"x1": 1.0, "x2^-12": 2.0 ** -12, "x2^8": 2.0 ** 8}[name])


def pyramid(v):
    """[x, mp5(x), mp5(mp5(x)), mp5^3(x)] of the fp32 values v [H][W][C], each [H][W][C]"""
    t = [torch.from_numpy(np.ascontiguousarray(v.transpose(2, 0, 1)))[None]]
    for _ in range(3):
        t.append(F.max_pool2d(t[-1], 5, 1, 2))
    return [a[0].numpy().transpose(1, 2, 0) for a in t]


def sppf_operands(name, H, W, planes):
    hi, lo = split16(sppf_input(name, H, W))
    src = [hi, lo][:planes]
    dst = [filled((H, W, DST_C), CANARY) for _ in range(planes)]
    vals = hi.astype(f32) + (lo.astype(f32) if planes == 2 else f32(0))
    return src, dst, vals


def two(a):
    return (a[0], a[1] if len(a) == 2 else None)


def value(planes_):
    return planes_[0].astype(f32) + (planes_[1].astype(f32) if len(planes_) == 2 else f32(0))


def check_sppf(be, H, W):
    for name in SPPF_INPUTS:
        for planes in (2, 1):
            src, dst, vals = sppf_operands(name, H, W, planes)
            assert be.emu_sppf_pool(*two(src), H, W, SRC_C, *two(dst), DST_C, NCH) == 0, (name, planes)
            got = value(dst)
            for i, want in enumerate(pyramid(vals[..., :NCH])):
                assert np.array_equal(got[..., i * NCH:(i + 1) * NCH], want), (name, planes, i)
            assert all((bits(d[..., 4 * NCH:]) == CANARY).all() for d in dst), (name, planes)


def check_sppf_refusals(be):
    def rc(H=16, W=32, nch=NCH, dst_c=DST_C, src_lo=True, dst_lo=True):
        s = [np.zeros((H, W, SRC_C), f16) for _ in range(2)]
        d = [filled((H, W, dst_c), CANARY) for _ in range(2)]
        r = be.emu_sppf_pool(s[0], s[1] if src_lo else None, H, W, SRC_C, d[0], d[1] if dst_lo else None, dst_c, nch)
        assert r == 0 or all((bits(a) == CANARY).all() for a in d)
        return r

    assert rc() == 0                                         # the well-formed neighbour
    assert rc(W=33) != 0                                     # 528 pixels: one workgroup holds 512
    assert rc(nch=60) != 0                                   # not whole octets (4 * 60 would fit)
    assert rc(dst_c=4 * NCH - 8) != 0                        # four slices do not fit the destination
    assert rc(src_lo=True, dst_lo=False) != 0 and rc(src_lo=False, dst_lo=True) != 0   # mixed planes


def chain(be, src, dst, H, W):
    """the plan's form above 512 pixels: slice copy, then three max-pools IN PLACE, slice i -> slice i + 1 of the concat tensor"""
    assert be.emu_chan_copy(*two(src), H, W, SRC_C, 0, *two(dst), DST_C, 0, NCH) == 0
    for i in range(3):
        assert be.emu_maxpool5_planes(*two(dst), H, W, DST_C, i * NCH, *two(dst), DST_C, (i + 1) * NCH, NCH) == 0


def check_chain_equals_sppf(be):
    H, W = 16, 32
    for name in ("x1", "shifted -50", "ties"):
        for planes in (2, 1):
            src, one, _ = sppf_operands(name, H, W, planes)
            _, many, _ = sppf_operands(name, H, W, planes)
            assert be.emu_sppf_pool(*two(src), H, W, SRC_C, *two(one), DST_C, NCH) == 0
            chain(be, src, many, H, W)
            assert np.array_equal(value(one)[..., :4 * NCH], value(many)[..., :4 * NCH]), (name, planes)
            # the planes' bits too, canary tail included -- but for slice 0, which the chain COPIES and sppf_pool splits again from the value: a pair whose lo is
            # exactly half an ulp of its hi (a residual that rounded up to it) has a second spelling with the same value, and the split picks the even hi
            assert all(np.array_equal(bits(a[..., NCH:]), bits(b[..., NCH:])) for a, b in zip(one, many)), (name, planes)
            if planes == 1:
                assert np.array_equal(bits(one[0]), bits(many[0])), name


def check_chain_large_map(be):
    H, W = 24, 40
    for name in ("x1", "shifted -50", "ties"):
        for planes in (2, 1):
            src, dst, vals = sppf_operands(name, H, W, planes)
            assert be.emu_sppf_pool(*two(src), H, W, SRC_C, *two(dst), DST_C, NCH) != 0     # 960 pixels: only the chain is accepted
            assert all((bits(d) == CANARY).all() for d in dst)
            chain(be, src, dst, H, W)
            got = value(dst)
            for i, want in enumerate(pyramid(vals[..., :NCH])):
                assert np.array_equal(got[..., i * NCH:(i + 1) * NCH], want), (name, planes, i)
            assert all((bits(d[..., 4 * NCH:]) == CANARY).all() for d in dst)


# ------------------------------------------------------------------------------------------------ the block as the plan runs it
def check_block_as_planned(be):
    """16x32, c_ = 128, two heads: chan_copy split of the 256-channel [a | y] tensor, attention on a qkv tensor handed in, dwconv_plain(v) + att.
    Reference: att + depthwise3x3(v) + b in fp64; bar: the attention bar + err32 of the depthwise sum + the storage of the result."""
    prepare(be)
    H, W, c_, heads, dk, dv = 16, 32, 128, 2, 32, 64
    T = H * W
    rng = np.random.default_rng(900)
    th, tl = split16(rng.standard_normal((T, 2 * c_)))
    yh, yl = filled((T, c_), CANARY), filled((T, c_), CANARY)
    assert be.emu_chan_copy(th, tl, H, W, 2 * c_, c_, yh, yl, c_, 0, c_) == 0
    assert np.array_equal(bits(yh), bits(th[:, c_:])) and np.array_equal(bits(yl), bits(tl[:, c_:]))
    hi, lo, x64, x32 = stored(rng.standard_normal((T, heads * (2 * dk + dv))), 2)
    att64, err_att, v64 = reference(("block",), x64, x32, heads, dk, dv, dk ** -0.5)
    bar_att = 4.0 * err_att + storage(float(np.abs(att64).max()), 2)
    w9, b = (rng.standard_normal((9, c_)) * 0.3).astype(f32), (rng.standard_normal(c_) * 0.1).astype(f32)

    def depthwise(v, w, bias):
        vp = np.pad(v.reshape(H, W, c_), ((1, 1), (1, 1), (0, 0)))
        acc = np.broadcast_to(bias, (H, W, c_)).astype(v.dtype)
        for ky in range(3):
            for kx in range(3):
                acc = acc + vp[ky:ky + H, kx:kx + W] * w[ky * 3 + kx]
        return acc.reshape(T, c_)

    pe64 = depthwise(v64, w9.astype(f64), b.astype(f64))
    pe32 = depthwise(v64.astype(f32), w9, b)
    assert pe32.dtype == f32
    want = att64 + pe64
    bar = bar_att + float(np.abs(pe32.astype(f64) - pe64).max()) + storage(float(np.abs(want).max()), 2)
    for qblock in (4, 0):
        a, v, o = ([np.zeros((T, c_), f16) for _ in range(2)] for _ in range(3))
        assert be.emu_attention(hi, lo, H, W, heads, dk, dv, f32(dk ** -0.5), a[0], a[1], v[0], v[1], qblock) == 0
        assert be.emu_dwconv_plain(v[0], v[1], a[0], a[1], o[0], o[1], H, W, c_, w9, b) == 0
        got = o[0].astype(f64) + o[1].astype(f64)
        err = float(np.abs(got - want).max())
        note(f"block 16x32x128 q{qblock}", be, err, bar)
        assert err <= bar, (qblock, err, bar)
