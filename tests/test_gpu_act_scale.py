"""VP_ACT_SCALE on the device: the abs-max kernel, the scaled convolution epilogue, and the flagged AutoDrive engine -- bit-identity while every exponent
is 0, the all-0 -> all-255 pair the unflagged engine refuses (tests/golden/autodrive_range.npz, tools/pin_act_scale.py), the shipped table, stability of
the replayed graph, refusals.  The figures of the ordinary pair go to profiles/act_scale.txt by tools/bench_act_scale.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "autodrive_range.npz"))
TARGET = 12


def _frames(name):
    from oracle import pre_post

    if name == "range":
        return np.zeros((1080, 1920, 3), dtype=np.uint8), np.full((1080, 1920, 3), 255, dtype=np.uint8)
    i = {"a": 0, "b": 3}[name]
    return tuple(pre_post.synthetic_frame(1080, 1920, 200 + k, smooth=(k % 3 != 2)) for k in (i, i + 1))


@pytest.fixture(scope="module")
def pairs():
    return {n: _frames(n) for n in ("range", "a", "b")}


@pytest.fixture(scope="module")
def blob():
    from autoware_vision_pilot_amd import weights as vw
    from oracle import autodrive

    return vw.pack_state_dict(autodrive.make_state_dict(int(GOLD["weight_seed"])))


def _engine(blob, **kw):
    from autoware_vision_pilot_amd import lib

    return lib.Engine("autodrive", blob, precision="fp16x3", **kw)


def _run(eng, pair):
    eng.infer_pair(*pair)
    return eng.logits().reshape(3).copy()


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def _split(v):
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(np.float32)).astype(np.float16)


# ---------------------------------------------------------------------------------------------------------------- test 1
@pytest.mark.parametrize("c,h,w,pitch", [(8, 3, 5, 8), (40, 17, 33, 64), (64, 1, 1, 64), (64, 256, 512, 64)])   # the last: 4 passes of the kernel's grid-stride loop
def test_absmax_equals_numpy(c, h, w, pitch):
    from autoware_vision_pilot_amd import lib

    rng = np.random.default_rng(c * 1000 + h)
    hi, lo = _split((rng.standard_normal((h, w, pitch)) * 50).astype(np.float32))
    if pitch > c:   # garbage in the padding: larger than anything real, and non-finite
        hi[..., c:] = np.float16(60000.0)
        hi[0, 0, c] = np.float16(np.inf)

    def check(hi, lo):
        val = hi[..., :c].astype(np.float32) + (0 if lo is None else lo[..., :c].astype(np.float32))
        fin = np.isfinite(val)
        want = (np.float32(np.abs(val[fin]).max()) if fin.any() else np.float32(0), int((~fin).sum()))
        got = lib.op_absmax(hi, lo, c)
        assert got == lib.op_absmax(hi, lo, c), "two launches disagree"
        assert _bits(got[0]) == _bits(want[0]) and got[1] == want[1], (got, want)

    check(hi, lo)
    check(hi, None)
    p = hi.copy(), lo.copy()
    p[0][0, 0, 0], p[1][0, 0, 0] = np.float16(np.inf), 0
    p[0][h - 1, w - 1, c - 1] = np.float16(-np.inf)
    p[0][h // 2, w // 2, c // 2] = np.float16(np.nan)
    check(*p)
    p = hi.copy(), lo.copy()
    p[0][h - 1, 0, c - 1], p[1][h - 1, 0, c - 1] = np.float16(-65504.0), 0
    check(*p)
    p = np.zeros_like(hi), np.zeros_like(lo)
    p[1][0, 0, 1] = np.float16(-3e-6)   # a subnormal low plane under a zero high plane
    check(*p)
    check(np.zeros_like(hi), np.zeros_like(lo))


# ---------------------------------------------------------------------------------------------------------------- test 2
@pytest.mark.parametrize("ks", [3, 1])
@pytest.mark.parametrize("cin", [32, 64])
@pytest.mark.parametrize("res_mode", [0, 1, 2])
def test_conv2d_scaled(ks, cin, res_mode):
    """Input ~3e5 (beyond fp16 unscaled) stored with in_exp = 6, residual with res_exp = -3, true output ~1e6 stored near 2^12: 2e-5 * max(1, |ref|) against
    torch fp64, the bar of the project's fp32-FMA kernel tests.  That bar has an ABSOLUTE floor (2e-5 where |ref| < 1) which fp32 accumulation of terms of
    size 1e6 cannot meet where they cancel (one fp32 rounding of 1e6 is 0.06), so the operands are chosen without cancellation: positive input, and weight
    rows and biases of one sign per output channel -- even channels come out near +1e6 (SiLU's linear side), odd ones saturate SiLU's other side (-0, so
    the gate stores r and the residual sum stores r: small values beside the large ones).  How small they may be is the storage format's limit, not the
    kernel's: below 2^-14 stored the low plane is subnormal with quantum 2^-24, i.e. 2^(out_exp - 25) = 3e-5 in true units here, so the gate's r is 8 .. 24
    (the bar there is 2e-5 * r >= 1.6e-4) and its convolution is scaled down to keep the product near 1e6.  A wrong or missing power of two anywhere is a
    factor >= 2."""
    from autoware_vision_pilot_amd import lib

    rng = np.random.default_rng(100 * cin + 10 * ks + res_mode)
    cout, h, w = 32, 8, 16
    sign = np.where(np.arange(cout) % 2 == 0, 1.0, -1.0)
    x = rng.uniform(1e5, 5e5, (cin, h, w)).astype(np.float32)
    wt = (np.abs(rng.standard_normal((cout, cin, ks, ks))) * (4.0 / (ks * ks * cin)) * sign[:, None, None, None]).astype(np.float32)
    b = (np.abs(rng.standard_normal(cout)) * 1e5 * sign).astype(np.float32)
    res = None
    if res_mode == 1:
        res = (rng.standard_normal((cout, h, w)) * 1e3).astype(np.float32)
    if res_mode == 2:
        res = rng.uniform(8.0, 24.0, (cout, h, w)).astype(np.float32)
        wt, b = wt / 16, b / 16
    y = torch.nn.functional.silu(torch.nn.functional.conv2d(torch.from_numpy(x).double()[None], torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=ks // 2))[0]
    if res_mode:
        r = torch.from_numpy(res).double()
        y = y + r if res_mode == 1 else y * r + r
    ref = y.numpy()
    out_exp = int(np.ceil(np.log2(np.abs(ref).max()))) - TARGET
    hi, lo = lib.op_conv2d_scaled(x, wt, b, ks=ks, act=2, res=res, res_mode=res_mode, in_exp=6, res_exp=-3, out_exp=out_exp)
    stored = hi.astype(np.float32) + lo.astype(np.float32)
    assert np.isfinite(stored).all() and 2.0 ** (TARGET - 1) <= np.abs(stored).max() <= 2.0 ** TARGET
    got = stored.astype(np.float64) * 2.0 ** out_exp
    rel = float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
    print(f"conv2d_scaled ks={ks} cin={cin} res_mode={res_mode}: |ref| max {np.abs(ref).max():.3e}, rel err {rel:.3e}")
    assert rel <= 2e-5, rel
    # all three exponents 0: the unflagged launch.  op_conv2d returns fp32(hi) + fp32(lo) of the planes it stored (exact), so equal sums <=> equal planes
    # up to the one ambiguity a re-split of the sum has (a lo of exactly half an ulp of hi): the sums are compared, bit for bit
    xs, bs = (x / 3e5).astype(np.float32), (b / 1e5).astype(np.float32)
    rs = None if res is None else (res / (1e3 if res_mode == 1 else 1.0)).astype(np.float32)
    h0, l0 = lib.op_conv2d_scaled(xs, wt, bs, ks=ks, act=2, res=rs, res_mode=res_mode)
    plain = lib.op_conv2d(xs, wt, bs, ks=ks, act=2, res=rs, res_mode=res_mode, precision=lib.VP_FP16X3)
    assert np.array_equal(_bits(h0.astype(np.float32) + l0.astype(np.float32)), _bits(plain))


# ---------------------------------------------------------------------------------------------------------------- test 3
@pytest.mark.parametrize("latency", [False, True])
def test_uncalibrated_flagged_engine_is_bit_identical(blob, pairs, latency):
    plain, flagged = _engine(blob, plan_latency=latency), _engine(blob, plan_latency=latency, act_scale=True)
    try:
        assert flagged.plan_hash() == plain.plan_hash() and not flagged.act_scales().any()
        assert np.array_equal(_bits(_run(flagged, pairs["a"])), _bits(_run(plain, pairs["a"])))
    finally:
        plain.close()
        flagged.close()


# ---------------------------------------------------------------------------------------------------------------- test 4
def _judge_range(got, prefix=""):
    """1e-3 * max(1, |ref_fp32|), the parity bar; an output whose fp32 reference is itself farther than 4e-4 from fp64 is judged by engine_vs_fp64 <=
    2.5 * fp32_vs_fp64 instead.  tools/pin_act_scale.py measured fp32_vs_fp64 <= 2.6e-6 on every output of this pair: the first rule."""
    ref32, ref64 = GOLD[prefix + "range_fp32"].astype(np.float64), GOLD[prefix + "range_fp64"]
    assert np.isfinite(got).all(), got
    for k in range(3):
        f32_vs_64 = abs(ref32[k] - ref64[k]) / max(1.0, abs(ref64[k]))
        e32 = abs(float(got[k]) - ref32[k]) / max(1.0, abs(ref32[k]))
        e64 = abs(float(got[k]) - ref64[k]) / max(1.0, abs(ref64[k]))
        print(f"range case {prefix or 'fp32-weights '}output {k}: engine {got[k]!r} fp32 {ref32[k]!r}; vs fp32 {e32:.3e}, vs fp64 {e64:.3e}, fp32 vs fp64 {f32_vs_64:.3e}")
        if f32_vs_64 > 4e-4:
            assert e64 <= 2.5 * f32_vs_64, (k, e64, f32_vs_64)
        else:
            assert e32 <= 1e-3, (k, e32)


def test_range_case(blob, pairs):
    from autoware_vision_pilot_amd import lib

    plain, flagged = _engine(blob), _engine(blob, act_scale=True)
    try:
        with pytest.raises(lib.VpRangeError):      # the precondition: without the flag the frame is refused
            plain.infer_pair(*pairs["range"])
        with pytest.raises(lib.VpRangeError):      # ... and so it is while every exponent is 0
            flagged.infer_pair(*pairs["range"])
        flagged.calibrate_range()                   # over the pair that is resident
        _judge_range(_run(flagged, pairs["range"]))
    finally:
        plain.close()
        flagged.close()


# ---------------------------------------------------------------------------------------------------------------- test 5
def test_ordinary_pair_after_calibration_on_another(blob, pairs):
    plain, flagged = _engine(blob), _engine(blob, act_scale=True)
    try:
        flagged.infer_pair(*pairs["a"])
        flagged.calibrate_range()
        got, base = _run(flagged, pairs["b"]), _run(plain, pairs["b"])
        ref32, ref64 = GOLD["b_fp32"].astype(np.float64), GOLD["b_fp64"]
        assert (np.abs(got - ref32) <= 1e-3 * np.maximum(1.0, np.abs(ref32))).all(), (got, ref32)
        e = lambda v: float((np.abs(v - ref64) / np.maximum(1.0, np.abs(ref64))).max())
        print(f"pair b, error against fp64: flagged (calibrated on pair a) {e(got):.3e}, unflagged {e(base):.3e}")
    finally:
        plain.close()
        flagged.close()


# ---------------------------------------------------------------------------------------------------------------- tests 6 and 7
# tensors that share storage or are copies / max-pools / convex combinations of each other carry ONE exponent
TIE_GROUPS = (("head.cat", "backbone.p5.3.cv2"), ("backbone.p5.2.cv1", "backbone.p5.2.cat"),
              ("backbone.p5.3.cv1", "backbone.p5.3.y", "backbone.p5.3.middle_block.conv2.1"),
              ("backbone.p5.3.middle_block.conv1.qkv", "backbone.p5.3.middle_block.conv1.attn", "backbone.p5.3.middle_block.conv1.v"))


def _check_band(names, exps, stored, target=TARGET):
    """Every untied tensor's stored abs-max lies in [2^(target - 1), 2^target) or the tensor is zero; the members of a tie group share one exponent, each
    stays below 2^target, and the group's largest member lies in the band (the smaller ones cannot: that is what sharing an exponent means)."""
    lo, hi = 2.0 ** (target - 1), 2.0 ** target
    tied = {n for g in TIE_GROUPS for n in g}
    assert tied <= set(names), tied - set(names)
    for g in TIE_GROUPS:
        idx = [names.index(n) for n in g]
        assert len({int(exps[i]) for i in idx}) == 1, (g, [int(exps[i]) for i in idx])
        assert all(stored[i] < hi for i in idx) and lo <= max(stored[i] for i in idx), (g, [stored[i] for i in idx])
    for i, n in enumerate(names):
        if n not in tied:
            assert stored[i] == 0 or lo <= stored[i] < hi, (n, int(exps[i]), stored[i])


def test_table_round_trip_reset_and_stability(blob, pairs):
    a, b, plain = _engine(blob, act_scale=True), _engine(blob, act_scale=True), _engine(blob)
    try:
        first = _run(a, pairs["a"])
        assert np.array_equal(_bits(first), _bits(_run(plain, pairs["a"])))
        h0 = a.plan_hash()
        a.infer_pair(pairs["a"][1], pairs["a"][1])     # one frame as both halves: every tensor's band is this frame's
        a.calibrate_range()
        exps = a.act_scales()
        assert a.plan_hash() == h0, "exponents are data, not plan"
        assert (exps != 0).any() and (exps < 0).any(), exps
        a.infer_pair(pairs["a"][1], pairs["a"][1])
        names = [t[0] for t in a.tensors()]
        stored = np.array([float(np.abs(a.tensor_read(i)).max()) * 2.0 ** -int(exps[i]) for i in range(len(names))])
        _check_band(names, exps, stored)
        # test 7: replay after calibration is bit-stable (the stream form: pass k + 1 reuses pass k's features, so the SAME pair is given each time)
        outs = [_run(a, pairs["b"]) for _ in range(3)]
        assert all(np.array_equal(_bits(o), _bits(outs[0])) for o in outs)
        # test 6: the shipped table
        b.set_act_scales(exps)
        assert np.array_equal(b.act_scales(), exps)
        for p in ("b", "a"):
            assert np.array_equal(_bits(_run(b, pairs[p])), _bits(_run(a, pairs[p]))), p
        with pytest.raises(ValueError):
            b.set_act_scales(exps[:-1])
        bad = exps.copy()
        bad[names.index("backbone.p5.3.cv2")] = bad[names.index("head.cat")] + 1
        with pytest.raises(ValueError, match="tied"):
            b.set_act_scales(bad)
        a.reset_range()
        assert not a.act_scales().any()
        assert np.array_equal(_bits(_run(a, pairs["a"])), _bits(first))
    finally:
        a.close()
        b.close()
        plain.close()


# ---------------------------------------------------------------------------------------------------------------- test 8
def test_refusals(blob):
    from autoware_vision_pilot_amd import lib, weights as vw
    from oracle import weights

    seg = vw.pack_state_dict(weights.make_state_dict("sceneseg", 0))
    with pytest.raises(ValueError, match="VP_ACT_SCALE"):
        lib.Engine("sceneseg", seg, precision="fp16x3", act_scale=True)
    with pytest.raises(ValueError, match="VP_ACT_SCALE"):
        lib.Engine("autodrive", blob, precision="fp16", act_scale=True)
    base = lib.Engine("sceneseg", seg, precision="fp16x3")
    try:
        with pytest.raises(ValueError, match="VP_ACT_SCALE"):
            lib.Engine("sceneseg", seg, precision="fp16x3", base=base, act_scale=True)
        with pytest.raises(ValueError, match="VP_ACT_SCALE"):
            lib.Engine("sceneseg", seg, precision="fp16x3", frames=2, act_scale=True)
    finally:
        base.close()


@pytest.mark.parametrize("latency", [False, True])
def test_range_case_with_fp8_weights(blob, pairs, latency):
    from autoware_vision_pilot_amd import lib

    plain, flagged = _engine(blob, weights_fp8=True, plan_latency=latency), _engine(blob, weights_fp8=True, plan_latency=latency, act_scale=True)
    try:
        with pytest.raises(lib.VpRangeError):
            plain.infer_pair(*pairs["range"])
        with pytest.raises(lib.VpRangeError):
            flagged.infer_pair(*pairs["range"])
        flagged.calibrate_range()
        _judge_range(_run(flagged, pairs["range"]), "fp8_")
    finally:
        plain.close()
        flagged.close()


def test_autodrive_infer_calibrates_on_its_first_pair(blob, pairs, tmp_path):
    """AutoDriveInfer(act_scale=True): forward() answers the pair the unflagged wrapper refuses; step() calibrates on its second frame and streams on."""
    from autoware_vision_pilot_amd import infer, lib

    path = tmp_path / "autodrive.vpw"
    path.write_bytes(bytes(blob))
    with pytest.raises(lib.VpRangeError):
        infer.AutoDriveInfer(str(path), precision="fp16x3").forward(*pairs["range"])
    m = infer.AutoDriveInfer(str(path), precision="fp16x3", act_scale=True)
    _judge_range(np.array(m.forward(*pairs["range"]), dtype=np.float32))
    s = infer.AutoDriveInfer(str(path), precision="fp16x3", act_scale=True)
    s.step(pairs["b"][0])
    assert not s.model.act_scales().any()
    got = np.array(s.step(pairs["b"][1]), dtype=np.float64)
    assert s.model.act_scales().any()
    ref = GOLD["b_fp32"].astype(np.float64)
    assert (np.abs(got - ref) <= 1e-3 * np.maximum(1.0, np.abs(ref))).all(), (got, ref)
    again = np.array(s.step(pairs["b"][1]), dtype=np.float64)      # the stream continues: this frame pairs with itself
    assert np.isfinite(again).all()
