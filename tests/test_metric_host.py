"""vp_metric without a GPU: the ABI, the properties of the restatements every metric test uses as its oracle (tests/metric_cases.py), and -- on the
HIP-on-CPU emulation of the real kernels and accumulator code (tests/emul) -- every case the MI355X runs: the select bit for bit, the segmentation
counts, depth exact and general, the reference's NaN answers and the accumulator's behaviour."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
import abi  # noqa: E402
import metric_cases as mc  # noqa: E402


@pytest.fixture(scope="module")
def emu_lib():
    import build as emul_build

    from autoware_vision_pilot_amd import lib

    if not os.path.exists(emul_build.CLANG):
        pytest.skip("host clang++ of the ROCm toolchain not found")
    so = ct.CDLL(emul_build.build(), mode=os.RTLD_LOCAL | os.RTLD_NOW)     # never RTLD_GLOBAL: same symbol names as libvp_hip.so
    for name, (res, args) in lib._SIGS.items():
        fn = getattr(so, name)
        fn.restype, fn.argtypes = res, args
    saved = lib._lib
    lib._lib = so
    yield lib
    lib._lib = saved


# ---- the ABI
def test_new_symbols_are_declared_exported_and_bound_and_the_structs_match():
    from autoware_vision_pilot_amd import lib

    src = abi.header_source()
    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in mc.NEW_SYMBOLS:
        assert s in declared and s in exported and s in lib.EXPORTED_SYMBOLS, s
    assert all(s.startswith("vp_") for s in exported)
    assert "enum vp_gt_form { VP_GT_LABEL = 0, VP_GT_BITS = 1 };" in src and (lib.VP_GT_LABEL, lib.VP_GT_BITS) == (0, 1)
    assert "uint32_t I[3], P[3], G[3];" in src and "float q_lo, q_hi, q, mae, mel;" in src
    assert "double sceneseg_iou[3], sceneseg_iou_full, domainseg_iou, mae, mel;" in src
    # vp_metric_frame: an int, twelve u32, five floats; the numpy record is the same layout
    F, D = lib.MetricFrame, lib.METRIC_FRAME_DTYPE
    assert ct.sizeof(F) == 72 == D.itemsize
    for name, off in (("kind", 0), ("I", 4), ("P", 16), ("G", 28), ("nonfinite", 40), ("n", 44), ("kept", 48), ("q_lo", 52), ("q_hi", 56), ("q", 60), ("mae", 64), ("mel", 68)):
        assert getattr(F, name).offset == off == D.fields[name][1], name
    # vp_metric_summary: six ints, seven doubles
    S = lib.MetricSummary
    assert ct.sizeof(S) == 80 and S.nan_frames.offset == 16 and S.sceneseg_iou.offset == 24 and S.sceneseg_iou_full.offset == 48 and S.mel.offset == 72


# ---- the restatements' own properties
def test_cascade_is_the_first_maximum_on_finite_logits_ties_included():
    rng = np.random.default_rng(0)
    lg = (rng.integers(-2, 3, (3, 64, 64)) / 2.0).astype(np.float32)          # five values: every tie pattern many times over
    lg[:, 0, :4] = np.array([[np.inf, 1, -np.inf, np.inf], [np.inf, -np.inf, -np.inf, 0], [0, -np.inf, -np.inf, np.inf]], np.float32)
    pred = mc.cascade(lg)
    assert np.array_equal(pred, np.argmax(lg, axis=0))
    ties = (lg[0] == lg[1]).sum(), (lg[0] == lg[2]).sum(), (lg[1] == lg[2]).sum(), ((lg[0] == lg[1]) & (lg[1] == lg[2])).sum()
    assert min(ties) > 100
    for c in range(3):                                                           # a NaN in any plane: no class
        bad = lg.copy()
        bad[c, 5, 5] = np.nan
        assert mc.cascade(bad)[5, 5] == 3
    one = np.array([[[0.0, -0.0, 1e-45, np.nan, np.inf, -1.0]]], np.float32)
    assert mc.predict(one).tolist() == [[3, 3, 0, 3, 0, 3]]


def test_quantile_ranks_and_lerp_are_torch_quantile():
    """q formed from the two order statistics and the fp32 weight equals torch.quantile bit for bit, also where 0.9 (n - 1) rounds to an integer in
    fp32 (n = 1961: the weight is 0 and q is the lower statistic)"""
    rng = np.random.default_rng(1)
    assert mc.quantile_ranks(1961) == (1764, 1765, np.float32(0)) and mc.quantile_ranks(11) == (9, 10, np.float32(0))
    for n in (64, 65, 135, 1961, 12800, 204800, 11):
        a = np.abs(rng.standard_normal(n)).astype(np.float32)
        lo, hi, w = mc.quantile_ranks(n)
        s = np.sort(a)
        q = torch.quantile(torch.from_numpy(a), 0.9, interpolation="linear").item()
        assert mc.same_f32(mc.lerp32(s[lo], s[hi], w), q), n


def test_kept_set_rule_of_the_quantile():
    """b > a and w > 0: the kept set is {A <= a}, lo + 1 elements; a == b: {A < a}, elements equal to q excluded"""
    n = 64
    lo, hi, w = mc.quantile_ranks(n)
    assert (lo, hi) == (56, 57) and w > 0
    g = np.zeros((8, 8), np.float32)
    g.reshape(-1)[:] = np.arange(n) * 4
    p = g.copy()
    p.reshape(-1)[1:-1] += (np.arange(n - 2) % 7 - 3)          # min and max stay: both normalisers stay
    r = mc.depth_torch32(p, g)
    assert r["q_hi"] > r["q_lo"] and r["q_lo"] < r["q"] <= r["q_hi"] and r["kept"] == lo + 1
    for shape in mc.EXACT_SEEDS:
        p, g, r = mc.exact_case(shape)
        A = np.abs(p / 2 - g / 2).reshape(-1)                   # the pair's normalisers are 2 and its minima 0
        a = np.sort(A)[mc.quantile_ranks(A.size)[0]]
        assert r["q_lo"] == r["q_hi"] == r["q"] == a and r["kept"] == int((A < a).sum()) < int((A <= a).sum())


def test_nan_answers_of_the_restatement():
    p, g = mc.general_pair(8, 8)
    same = mc.depth_torch32(g, g)
    assert np.isnan(same["mae"]) and same["mel"] == 0.0 and same["kept"] == 0
    const = mc.depth_torch32(np.full((8, 8), 1.5, np.float32), g)
    assert np.isnan(const["mae"]) and np.isnan(const["mel"])
    with pytest.raises(RuntimeError):                            # the reference's pooling refuses planes below 8 x 8
        mc.depth_torch32(p[:7], g[:7])


def test_general_cases_torch_fp32_sits_close_to_fp64():
    for shape in mc.GENERAL_SHAPES:
        _, _, r32, r64 = mc.general_case(shape)
        assert r32["q_hi"] > r32["q_lo"]
        for k in ("mae", "mel"):
            assert abs(r32[k] - r64[k]) <= 2.0 ** -21 * r64["S"]


# ---- the emulated library
@pytest.mark.parametrize("n", mc.SELECT_SIZES)
def test_select_bit_for_bit_emulated(emu_lib, n):
    mc.check_select(emu_lib, n)


def test_select_refusals_emulated(emu_lib):
    mc.check_select_refusals(emu_lib)


@pytest.mark.parametrize("shape", mc.SEG_SHAPES, ids=["x".join(map(str, s)) for s in mc.SEG_SHAPES])
def test_seg_counts_bit_for_bit_emulated(emu_lib, shape):
    mc.check_seg(emu_lib, shape)


def test_seg_absent_class_scores_one_emulated(emu_lib):
    mc.check_seg_absent_class(emu_lib)


@pytest.mark.parametrize("shape", tuple(mc.EXACT_SEEDS), ids=["x".join(map(str, s)) for s in mc.EXACT_SEEDS])
def test_depth_exact_emulated(emu_lib, shape):
    mc.check_depth_exact(emu_lib, shape)


@pytest.mark.parametrize("shape", mc.GENERAL_SHAPES, ids=["x".join(map(str, s)) for s in mc.GENERAL_SHAPES])
def test_depth_general_emulated(emu_lib, shape):
    mc.check_depth_general(emu_lib, shape)


def test_depth_nan_answers_emulated(emu_lib):
    mc.check_depth_nan_answers(emu_lib)


def test_accumulator_emulated(emu_lib):
    mc.check_accumulator(emu_lib, emu_lib.VpError)


def test_refusals_emulated(emu_lib):
    mc.check_refusals(emu_lib)
