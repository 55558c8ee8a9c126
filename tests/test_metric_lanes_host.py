"""vp_metric's lane part without a GPU: the ABI, the restatements against the pinned reference results (tests/golden/metric_lanes.npz), and -- on the
HIP-on-CPU emulation of the real kernels and accumulator code (tests/emul) -- every case the MI355X runs: lane masks edge-exact and general, the three
ground-truth forms, the NaN answers, the accumulator, the refusals, the lane rows, and the host AP against compute_vector_ap."""
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
import metric_lanes_cases as lc  # noqa: E402


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


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


# ---- the ABI
def test_new_symbols_are_declared_exported_and_bound_and_the_structs_match():
    from autoware_vision_pilot_amd import lib

    src = abi.header_source()
    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in lc.NEW_SYMBOLS:
        assert s in declared and s in exported and s in lib.EXPORTED_SYMBOLS, s
    assert all(s.startswith("vp_") for s in exported)
    assert "enum vp_lanes_gt_form { VP_LANES_GT_PLANES = 0, VP_LANES_GT_BITS = 1, VP_LANES_GT_BITS_4X = 2 };" in src
    assert (lib.VP_LANES_GT_PLANES, lib.VP_LANES_GT_BITS, lib.VP_LANES_GT_BITS_4X) == (0, 1, 2)
    assert "float bce[3], edge[3][5], loss[3], score;" in src and "double precision, recall, mean_ap, ap[VP_ROWS_MAX_THR], map50;" in src
    assert "#define VP_ROWS_MAX_THR 8" in src and lib.VP_ROWS_MAX_THR == 8
    # vp_metric_lanes_frame: 22 floats, two u32; vp_metric_rows_line: two floats, three u32; the numpy records are the same layouts
    F, D = lib.MetricLanesFrame, lib.METRIC_LANES_FRAME_DTYPE
    assert ct.sizeof(F) == 96 == D.itemsize
    for name, off in (("bce", 0), ("edge", 12), ("loss", 72), ("score", 84), ("n", 88), ("nonfinite", 92)):
        assert getattr(F, name).offset == off == D.fields[name][1], name
    R, E = lib.MetricRowsLine, lib.METRIC_ROWS_LINE_DTYPE
    assert ct.sizeof(R) == 20 == E.itemsize
    for name, off in (("dist", 0), ("conf", 4), ("tp", 8), ("valid", 12), ("target_valid", 16)):
        assert getattr(R, name).offset == off == E.fields[name][1], name
    S, T = lib.MetricLanesSummary, lib.MetricRowsSummary
    assert ct.sizeof(S) == 88 and S.score.offset == 8 and S.edge.offset == 64
    assert ct.sizeof(T) == 104 and T.precision.offset == 8 and T.ap.offset == 32 and T.map50.offset == 96
    # the older records and entries are as they were
    assert ct.sizeof(lib.MetricFrame) == 72 and ct.sizeof(lib.MetricSummary) == 80


# ---- the restatements
PINNED = [(lc.exact_case, s) for s in lc.EXACT_SHAPES] + [(lc.general_case, s) for s in lc.GENERAL_SHAPES]


@pytest.mark.parametrize("case,shape", PINNED, ids=[c.__name__ + "-" + lc.key(s) for c, s in PINNED])
def test_restatement_equals_the_pinned_reference(case, shape):
    """the torch restatement of tests/metric_lanes_cases.py against the trainer's own methods, in both precisions (exact_case also asserts its property)"""
    lg, bits, r32, r64 = case(shape)
    planes = lc.planes_of_bits(bits)
    assert np.allclose(lc.pack(lc.lanes_ref(lg, planes, torch.float64)), lc.pack(r64), rtol=1e-12, atol=0)
    assert np.allclose(lc.pack(lc.lanes_ref(lg, planes, torch.float32)), lc.pack(r32), rtol=2.0 ** -20, atol=0)


def test_threshold_trap():
    """Threshold(0, 1) of relu: 1.0 where the value is not above 0 -- zero, negative zero and every negative logit -- and the value itself elsewhere"""
    t = lc.threshold_plane(np.array([0.0, -0.0, 1e-45, 2.0], np.float32)).numpy()
    assert t.view(np.uint32).tolist() == np.array([1.0, 1.0, 1e-45, 2.0], np.float32).view(np.uint32).tolist()
    assert lc.threshold_plane(np.array([-3.0], np.float32)).item() == 1.0
    assert torch.equal(lc.threshold_plane(torch.tensor([0.0, -0.0, 1e-45, 2.0, -3.0])), torch.nn.Threshold(0.0, 1.0)(torch.relu(torch.tensor([0.0, -0.0, 1e-45, 2.0, -3.0]))))


def test_general_cases_sit_where_the_issue_measured_them():
    """the reference's fp32 run within 4e-6 of its fp64 run on scores of 12 to 15: the bars of the general cases rest on that distance"""
    for shape in lc.GENERAL_SHAPES:
        _, _, r32, r64 = lc.general_case(shape)
        assert 12.0 < r64["score"] < 15.0 and abs(r32["score"] - r64["score"]) < 4e-6


def test_rows_generators_and_restatement():
    for case in lc.ROWS_GENERAL:
        lc.rows_general(*case)                                   # asserts the distance from every threshold
    xp, hv, txp, thv = lc.rows_dyadic(2, 64, 0)
    want = lc.rows_ref(xp, hv, txp, thv)
    for k in range(2):
        d32, c32 = lc.rows_torch32(xp[k], hv[k], txp[k], thv[k])
        assert d32 == want["dist"][k] and c32 == want["conf"][k]   # exact sums: torch's fp32 mean and the fp64 mean coincide


@pytest.mark.parametrize("name", lc.AP_CASES)
def test_vector_ap_restatement_equals_the_pinned_reference(name):
    tp, conf = lc.ap_inputs(name)
    g = lc.golden()
    assert np.array_equal(tp, g["ap_" + name + "_tp"]) and np.array_equal(conf, g["ap_" + name + "_conf"])
    got = lc.vector_ap(tp, conf)
    assert np.allclose([got[k] for k in ("precision", "recall", "mean_ap", "map50")], g["ap_" + name], rtol=0, atol=1e-12)


# ---- the host AP entry (no device: the library's own host code)
@pytest.mark.parametrize("name", lc.AP_CASES)
def test_host_ap_against_compute_vector_ap(emu_lib, name):
    tp, conf = lc.ap_inputs(name)
    s = emu_lib.rows_ap(tp, conf)
    want = lc.golden()["ap_" + name]
    assert s["lines"] == tp.size and s["n_thr"] == 3
    for k, v in zip(("precision", "recall", "mean_ap", "map50"), want):
        assert abs(s[k] - v) <= 1e-12, (k, s[k], v)
    assert np.allclose(s["ap"], lc.vector_ap(tp, conf)["ap"], rtol=0, atol=1e-12)
    if name == "tie":                                            # the tie rule decides: the other order of the tied lines scores differently
        swapped = tp.copy()
        swapped[[2, 5]] = swapped[[5, 2]]
        assert abs(emu_lib.rows_ap(swapped, conf)["mean_ap"] - want[2]) > 1e-6
    assert np.isnan(emu_lib.rows_ap(tp, conf, thr=[0.02, 0.1, 0.3])["map50"])
    none = emu_lib.rows_ap(np.zeros(0, np.uint32), np.zeros(0, np.float32))
    assert (none["lines"], none["precision"], none["recall"], none["mean_ap"], none["map50"]) == (0, 0.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        emu_lib.rows_ap(tp, conf, thr=np.zeros(9))


# ---- the emulated library
@pytest.mark.parametrize("shape", lc.EXACT_SHAPES, ids=ids(lc.EXACT_SHAPES))
def test_lanes_edge_exact_emulated(emu_lib, shape):
    lc.check_lanes_exact(emu_lib, shape)


@pytest.mark.parametrize("shape", lc.GENERAL_SHAPES, ids=ids(lc.GENERAL_SHAPES))
def test_lanes_general_emulated(emu_lib, shape):
    lc.check_lanes_general(emu_lib, shape)


def test_lanes_gt_forms_emulated(emu_lib):
    lc.check_lanes_gt_forms(emu_lib)


def test_lanes_nan_answers_emulated(emu_lib):
    lc.check_lanes_nan_answers(emu_lib)


def test_lanes_accumulator_emulated(emu_lib):
    lc.check_lanes_accumulator(emu_lib, emu_lib.VpError)


def test_lanes_and_rows_refusals_emulated(emu_lib):
    lc.check_lanes_refusals(emu_lib)


@pytest.mark.parametrize("case", lc.ROWS_DYADIC, ids=["%dx%d" % c[:2] for c in lc.ROWS_DYADIC])
def test_rows_dyadic_bit_for_bit_emulated(emu_lib, case):
    lc.check_rows_dyadic(emu_lib, case)


@pytest.mark.parametrize("case", lc.ROWS_GENERAL, ids=["%dx%d" % c[:2] for c in lc.ROWS_GENERAL])
def test_rows_general_emulated(emu_lib, case):
    lc.check_rows_general(emu_lib, case)


def test_rows_special_values_emulated(emu_lib):
    lc.check_rows_special(emu_lib)
