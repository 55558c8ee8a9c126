"""The range survey without a GPU: the C ABI, and act_exp_hist_kernel (vp_op_exp_hist) on the CPU-emulated library (tests/emul: the real kernel and
engine sources on the HIP-on-CPU shim) against the numpy oracle of tests/range_hist_cases.py, exactly -- the GPU twin is tests/test_gpu_range_survey.py."""
import ctypes as ct
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emul"))
sys.path.insert(0, HERE)

import abi  # noqa: E402
import range_hist_cases as cases  # noqa: E402

NEW_SYMBOLS = ("vp_range_survey", "vp_op_exp_hist")
CASES = cases.operator_cases()


def test_abi_exports_the_range_survey_symbols():
    from autoware_vision_pilot_amd import lib

    header = open(abi.HEADER).read()
    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in lib.EXPORTED_SYMBOLS and s in exported, s
    for name, value, oracle_value in (("VP_RANGE_BINS", lib.VP_RANGE_BINS, cases.BINS), ("VP_RANGE_EXP_MIN", lib.VP_RANGE_EXP_MIN, cases.EXP_MIN)):
        m = re.search(r"#define %s \(?(-?\d+)\)?" % name, header)
        assert m and int(m.group(1)) == value == oracle_value, name
    # vp_range_stats as ctypes lays it out is the header's struct: two 4-byte fields, then 3 + VP_RANGE_BINS 8-byte counters
    assert ct.sizeof(lib.RangeStats) == 8 + 8 * (3 + lib.VP_RANGE_BINS) and lib.RangeStats.bins.offset == 32


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


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_exp_hist_kernel_on_cpu(emu_lib, case):
    _, hi, lo, c = case
    cases.check_operator(emu_lib, hi, lo, c)


def test_exp_hist_refuses_bad_geometry(emu_lib):
    hi = np.zeros((2, 2, 32), np.float16)
    with pytest.raises(ValueError):
        emu_lib.op_exp_hist(hi, None, 40)          # more channels than the pitch holds
    with pytest.raises(ValueError):
        emu_lib.op_exp_hist(hi[..., :12], None, 8)  # a pitch that is no multiple of 8


def test_range_summary_reads_a_record():
    from autoware_vision_pilot_amd import lib

    bins = np.zeros(lib.VP_RANGE_BINS, np.int64)
    bins[-24 - lib.VP_RANGE_EXP_MIN] = 1     # 2^-24: below both marks
    bins[-4 - lib.VP_RANGE_EXP_MIN] = 1      # [2^-4, 2^-3): below 0.125 only
    bins[-3 - lib.VP_RANGE_EXP_MIN] = 1      # [0.125, 0.25): above both
    bins[9 - lib.VP_RANGE_EXP_MIN] = 1
    s = lib.range_summary({"bins": bins, "absmax": np.float32(1000.0)})
    assert s == {"headroom": 6, "below_lo_normal": 0.5, "below_hi_normal": 0.25}
    assert lib.range_summary({"bins": bins * 0, "absmax": np.float32(0.0)}) == {"headroom": None, "below_lo_normal": 0.0, "below_hi_normal": 0.0}
    assert lib.range_summary({"bins": bins, "absmax": np.float32(65504.0)})["headroom"] == 0
