"""The convolution forms beyond vp_op_conv2d's (3x3 stride 2, the CTX gate, alias-slice destinations, a residual read from a slice, all of them under
the activation scale, and the plan-time refusals) on the CPU: the bodies of tests/conv_forms_cases.py through vp_op_conv2d_forms of the HIP-on-CPU
emulation (tests/emul: the real kernel and engine sources).  The device twin is tests/test_gpu_conv_forms.py."""
import ctypes as ct
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))

import abi   # noqa: E402
import conv_forms_cases as cases   # noqa: E402

NEW_SYMBOLS = ("vp_op_conv2d_forms",)
PRECISIONS = ["fp16x3", "fp16"]


def test_abi_exports_the_forms_entry():
    from autoware_vision_pilot_amd import lib

    header = open(abi.HEADER).read()
    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in lib.EXPORTED_SYMBOLS and s in exported, s
    fields = re.search(r"typedef struct vp_conv_form \{(.*?)\} vp_conv_form;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.replace("int ", "", 1).split(",")]
    assert tuple(names) == lib._CONV_FORM_FIELDS      # the wrapper fills the struct as an int array in the header's order


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


# ---- A
@pytest.mark.parametrize("row", cases.A_ROWS, ids=lambda r: "%d-%d_%dx%d" % r)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_stride2_against_fp64(emu_lib, precision, row):
    cases.check_stride2(emu_lib, precision, row)


@pytest.mark.parametrize("ky,kx", cases.TAPS)
def test_stride2_single_tap_is_exact(emu_lib, ky, kx):
    cases.check_stride2_tap(emu_lib, ky, kx)


def test_stride2_refusals(emu_lib):
    cases.check_stride2_refusals(emu_lib)


@pytest.mark.parametrize("row", cases.A_FP8_ROWS, ids=lambda r: "%d-%d_%dx%d" % r)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_stride2_fp8_storage(emu_lib, precision, row):
    cases.check_stride2_fp8(emu_lib, precision, row)


# ---- B
@pytest.mark.parametrize("row", cases.B_ROWS, ids=lambda r: "%d-%d_%dx%d" % r)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ctx_gate_against_fp64(emu_lib, precision, row):
    cases.check_gate(emu_lib, precision, row)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ctx_gate_fp8_storage(emu_lib, precision):
    cases.check_gate_fp8(emu_lib, precision)


# ---- C
@pytest.mark.parametrize("name,variant", cases.C_IDS, ids=lambda v: str(v).replace(" ", "_"))
def test_slice_store_leaves_the_neighbours(emu_lib, name, variant):
    cases.check_slice(emu_lib, name, variant)


# ---- D
@pytest.mark.parametrize("exps", cases.D_EXPS, ids=lambda e: "%d_%d_%d" % e)
@pytest.mark.parametrize("form", ["A", "B", "C"])
def test_forms_under_the_activation_scale(emu_lib, form, exps):
    cases.check_scaled(emu_lib, form, exps)


def test_flagged_engine_with_zero_exponents_is_the_unflagged_one(emu_lib):
    cases.check_scaled_zero_exponents(emu_lib)


# ---- E
def test_refusals_at_plan_time(emu_lib):
    cases.check_refusals(emu_lib)
