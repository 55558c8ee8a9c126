"""Device-only cases of the encoder, context and fusion kernels (the bodies of tests/test_kernels_emulated.py, device backend of
tests/emul/backends.py: the product's own gfx950 kernel objects): every encoder launch of the SceneSeg plan at the 320x640 input with
the shapes taken from B0_STAGES and the replica count of the engine's rule, at the bars the emulated tests use; three launches of every
kernel that accumulates with atomics, bit-identical; value edges (inputs, biases and residuals x 2^-12, where the lo plane is subnormal,
and x 2^8, large pool sums), judged relative to the tensor's scale with the output format's own storage error added; the real sizes of
the squeeze-excite gate, the context path and EgoLanes' feature fusion."""
import os
import sys

import numpy as np
import pytest

from autoware_vision_pilot_amd.synthetic import B0_STAGES, B0_STEM_OUT
from test_kernels_emulated import (check_ctx_conv1, check_depthwise_pool, check_fusion, check_mbconv_back, check_mbconv_front, check_pool_fc,
                                   check_squeeze_excite, check_stem)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))

pytestmark = pytest.mark.gpu

NET_H, NET_W = 320, 640
K_SE_MAX_REPLICAS = 64      # kernels.hpp kSeMaxReplicas


def se_replicas(hw):
    """engine.cpp build_backbone: replica rows of the pool atomics, ~4 per row of 32 pixels, 8 ... kSeMaxReplicas"""
    r = 8
    while r < K_SE_MAX_REPLICAS and r * 4 * 32 <= hw:
        r *= 2
    return r


def _plan():
    """(depthwise + pool launches, mbconv_front launches, mbconv_back launches) of the SceneSeg encoder at NET_H x NET_W, one entry per
    distinct geometry"""
    dws, fronts, backs = [], [], []
    H, W, cprev = NET_H // 2, NET_W // 2, B0_STEM_OUT
    for e, k, s, cin0, cout, n in B0_STAGES:
        assert cin0 == cprev
        for bi in range(n):
            cin, stride = (cin0, s) if bi == 0 else (cout, 1)
            cexp, OH, OW = cin * e, H // stride, W // stride
            rep, sq = se_replicas(OH * OW), max(1, cin // 4)
            if e == 1:
                dws.append((cexp, k, stride, H, W, rep))
            else:
                fronts.append((cin, cexp, k, stride, H, W, rep))
            backs.append((cexp, cout, sq, OH, OW, stride == 1 and cin == cout, rep))
            H, W = OH, OW
        cprev = cout
    dedup = lambda xs: list(dict.fromkeys(xs))
    return dedup(dws), dedup(fronts), dedup(backs)


DWS, FRONTS, BACKS = _plan()
SCALES = [1.0, 2.0 ** -12, 2.0 ** 8]
_errs = {}


@pytest.fixture(scope="module")
def dev():
    import backends

    return backends.load("device")


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    if _errs:
        print("\nlargest measured error per kernel (relative to the tensor's largest magnitude) / its bar:")
        for name, (err, bar) in sorted(_errs.items()):
            print(f"  {name:<44} {err:.3e} / {bar:.3e}")


def _note(name, r):
    err, bar = _errs.get(name, (0.0, 0.0))
    _errs[name] = (max(err, r["err"]), max(bar, r["bar"]))
    return r


def _same(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b) if x is not None)


def test_plan_covers_the_encoder():
    # stage 1 (expansion 1): depthwise + pool alone; stages 2-7: one front per distinct geometry; every block a back half
    assert len(DWS) == 1 and DWS[0][:5] == (32, 3, 1, NET_H // 2, NET_W // 2)
    assert {f[2:4] for f in FRONTS} == {(3, 2), (3, 1), (5, 2), (5, 1)}
    assert {b[-1] for b in BACKS} == {8, 32, 64} and max(f[4] for f in FRONTS) == NET_H // 2


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("split", [True, False])
def test_stem_production(dev, split, scale):
    r = check_stem(dev, NET_H, NET_W, split, seed=31, scale=scale)
    if split:
        _note("stem", r)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("C,k,stride,H,W,rep", DWS)
def test_depthwise_pool_production(dev, C, k, stride, H, W, rep, scale):
    _note("dwconv_pool", check_depthwise_pool(dev, C, k, stride, H, W, replicas=rep, seed=C + 1, scale=scale))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("cin,cexp,k,stride,H,W,rep", FRONTS)
def test_mbconv_front_production(dev, cin, cexp, k, stride, H, W, rep, scale):
    _note("mbconv_front", check_mbconv_front(dev, cin, cexp, k, stride, H, W, replicas=rep, seed=cin + cexp + H, scale=scale, fp16=scale == 1.0))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("cexp,cout,sq,H,W,residual,rep", BACKS)
def test_mbconv_back_production(dev, cexp, cout, sq, H, W, residual, rep, scale):
    _note("mbconv_back", check_mbconv_back(dev, cexp, cout, sq, H, W, residual, replicas=rep, seed=cexp + cout + H, scale=scale, fp16=scale == 1.0))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("cexp,cout,sq,H,W,residual,rep", BACKS)
def test_squeeze_excite_production(dev, cexp, cout, sq, H, W, residual, rep, scale):
    """the unfused path's gate (se_gate_scale): projection rows = Cout, the block's expanded channels, pool over the block's map"""
    C, rows = (cexp + 31) // 32 * 32, (cout + 31) // 32 * 32
    _note("se_gate_scale", check_squeeze_excite(dev, C, cexp, sq, rows, H * W, rep, seed=cexp + H, scale=scale))


def test_atomics_are_deterministic(dev):
    """three launches on the same inputs: outputs, per-channel sums and squeeze sums bit-identical (the 2^24 fixed-point pool sums are
    integer atomics: any order gives the same bits -- under real scheduling, on the biggest map and the most replicas of the plan)"""
    C, k, stride, H, W, rep = DWS[0]
    runs = [check_depthwise_pool(dev, C, k, stride, H, W, replicas=rep, seed=5) for _ in range(3)]
    for r in runs[1:]:
        assert _same(r["out"], runs[0]["out"]) and _same(r["out16"], runs[0]["out16"])
    for cin, cexp, k, stride, H, W, rep in (FRONTS[0], FRONTS[-1]):
        runs = [check_mbconv_front(dev, cin, cexp, k, stride, H, W, replicas=rep, seed=6) for _ in range(3)]
        for r in runs[1:]:
            assert _same(r["out"], runs[0]["out"]) and _same(r["engine_form"], runs[0]["engine_form"]) and _same(r["out16"], runs[0]["out16"])
    for cexp, cout, sq, H, W, residual, rep in (BACKS[1], BACKS[-1]):
        runs = [check_mbconv_back(dev, cexp, cout, sq, H, W, residual, replicas=rep, seed=7) for _ in range(3)]
        for r in runs[1:]:
            assert _same(r["out"], runs[0]["out"]) and _same(r["zs_form"], runs[0]["zs_form"]) and np.array_equal(r["out16"], runs[0]["out16"])


def test_batched_production_equals_per_frame(dev):
    """the batched depthwise + pool and squeeze-excite instantiations at stage 1's real map (three frames): per frame, bit-identical to
    single-frame launches"""
    from test_kernels_emulated import split16

    C, k, stride, H, W, rep = DWS[0]
    frames, sq, rows = 3, 8, 32
    rng = np.random.default_rng(41)
    xh, xl = split16(rng.standard_normal((frames, H, W, C)).astype(np.float32))
    wk = (rng.standard_normal((k * k, C)) * 0.3).astype(np.float32)
    b = (rng.standard_normal(C) * 0.1).astype(np.float32)
    w1, b1 = (rng.standard_normal((sq, C)) * 0.2).astype(np.float32), (rng.standard_normal(sq) * 0.1).astype(np.float32)
    w2, b2 = (rng.standard_normal((C, sq)) * 0.5).astype(np.float32), (rng.standard_normal(C) * 0.2).astype(np.float32)
    pw = rng.standard_normal((rows, C)).astype(np.float32)
    OH, OW = H // stride, W // stride
    oh, ol = np.zeros((frames, OH, OW, C), np.float16), np.zeros((frames, OH, OW, C), np.float16)
    sums = np.zeros((frames, rep, C), np.uint64)
    assert dev.emu_dwconv_batched(xh, xl, H, W, C, oh, ol, OH, OW, wk, b, k, stride, sums, rep, frames) == 0
    ph, pl = np.zeros((frames, rows, C), np.float16), np.zeros((frames, rows, C), np.float16)
    assert dev.emu_se_gate_scale(sums, rep, C, C, sq, 1.0 / (OH * OW), w1, b1, pw, ph, pl, rows, w2, b2, frames) == 0
    for f in range(frames):
        o1, o2, sm = np.zeros((OH, OW, C), np.float16), np.zeros((OH, OW, C), np.float16), np.zeros((rep, C), np.uint64)
        assert dev.emu_dwconv(np.ascontiguousarray(xh[f]), np.ascontiguousarray(xl[f]), H, W, C, o1, o2, OH, OW, wk, b, k, stride, sm, rep) == 0
        assert np.array_equal(oh[f], o1) and np.array_equal(ol[f], o2) and np.array_equal(sums[f], sm), f
        q1, q2 = np.zeros((rows, C), np.float16), np.zeros((rows, C), np.float16)
        assert dev.emu_se_gate_scale(sm, rep, C, C, sq, 1.0 / (OH * OW), w1, b1, pw, q1, q2, rows, w2, b2, 1) == 0
        assert np.array_equal(ph[f], q1) and np.array_equal(pl[f], q2), f


@pytest.mark.parametrize("kind,cin", [("sceneseg", 1280), ("egolanes", 1456)])
def test_context_path_production(dev, kind, cin):
    """scene_context.py / auto_steer_context.py at the 10x20 map: the pool over cin channels -> context_layer_0 (800 outputs, GELU);
    context_layer_3 (1 -> 128 channels, GELU)"""
    rng = np.random.default_rng(cin)
    _note("pool_partial + fc_pooled", check_pool_fc(dev, NET_H // 32, NET_W // 32, cin, (cin + 31) // 32 * 32, 4, 800, rng))
    _note("ctx_conv1", check_ctx_conv1(dev, NET_H // 32, NET_W // 32, 128, rng))


def test_feature_fusion_production(dev):
    """EgoLanes' fusion at the 320x640 input: taps 160x320x32, 80x160x24, 40x80x40, 20x40x80, 10x20x1280 -> 10x20x1456, both kernels"""
    rng = np.random.default_rng(43)
    _note("fusion", check_fusion(dev, NET_H // 32, NET_W // 32, [32, 24, 40, 80, 1280], [32, 32, 64, 96, 1280], 1472, (0, 1), rng))
