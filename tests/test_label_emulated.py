"""vp_metric's label kernels and accumulator code on the HIP-on-CPU emulation (tests/emul), as they stand: the small cases of tests/label_cases.py through
vp_op_label_gt / vp_op_label_depth_gt and the operator forms of the accumulator, bit for bit against the numpy reference."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
import label_cases as lc  # noqa: E402


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


@pytest.mark.parametrize("name", lc.EMULATED_COLOUR)
def test_colour_labels_emulated(emu_lib, name):
    lc.check_colour(emu_lib, name)


@pytest.mark.parametrize("name", lc.EMULATED_MASK)
def test_mask_labels_emulated(emu_lib, name):
    lc.check_mask(emu_lib, name)


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=("f32", "f64"))
@pytest.mark.parametrize("name", lc.EMULATED_DEPTH)
def test_depth_labels_emulated(emu_lib, name, dtype):
    lc.check_depth(emu_lib, name, dtype)


def test_fused_records_emulated(emu_lib):
    lc.check_fused(emu_lib)


def test_one_host_buffer_emulated(emu_lib):
    lc.check_one_buffer(emu_lib)


def test_refusals_emulated(emu_lib):
    lc.check_refusals(emu_lib)
