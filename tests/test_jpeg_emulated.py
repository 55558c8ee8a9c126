"""The canvas's JPEG encoder on the HIP-on-CPU emulation of the real kernels and host class (tests/emul): vp_op_jpeg_encode_bgr8 on the cases up to
48 x 64 and the canvas entries byte for byte against the numpy twin (tests/jpeg_ref.py), and every refusal."""
import ctypes as ct
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
import jpeg_cases as jc  # noqa: E402


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


@pytest.mark.parametrize("case", jc.SMALL_CASES, ids=jc.case_id)
def test_operator_equals_the_twin_emulated(emu_lib, case):
    jc.check_operator(emu_lib, case)


def test_operator_refusals_emulated(emu_lib):
    jc.check_operator_refusals(emu_lib)


def test_host_entries_emulated(emu_lib):
    jc.check_host_entries(emu_lib)


def test_canvas_fetch_jpeg_emulated(emu_lib):
    jc.check_canvas(emu_lib)


def test_canvas_refusals_emulated(emu_lib):
    jc.check_canvas_refusals(emu_lib)
