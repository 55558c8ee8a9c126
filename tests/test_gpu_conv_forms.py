"""The convolution forms beyond vp_op_conv2d's on the device: the bodies of tests/conv_forms_cases.py (3x3 stride 2, the CTX gate, alias-slice
destinations, a residual read from a slice, all of them under the activation scale, the plan-time refusals) through the product library's
vp_op_conv2d_forms -- same shapes and bars as tests/test_conv_forms_emulated.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_forms_cases as cases   # noqa: E402

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp16x3", "fp16"]


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib as vp_lib

    return vp_lib


# ---- A
@pytest.mark.parametrize("row", cases.A_ROWS, ids=lambda r: "%d-%d_%dx%d" % r)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_stride2_against_fp64(lib, precision, row):
    cases.check_stride2(lib, precision, row)


@pytest.mark.parametrize("ky,kx", cases.TAPS)
def test_stride2_single_tap_is_exact(lib, ky, kx):
    cases.check_stride2_tap(lib, ky, kx)


def test_stride2_refusals(lib):
    cases.check_stride2_refusals(lib)


@pytest.mark.parametrize("row", cases.A_FP8_ROWS, ids=lambda r: "%d-%d_%dx%d" % r)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_stride2_fp8_storage(lib, precision, row):
    cases.check_stride2_fp8(lib, precision, row)


# ---- B
@pytest.mark.parametrize("row", cases.B_ROWS, ids=lambda r: "%d-%d_%dx%d" % r)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ctx_gate_against_fp64(lib, precision, row):
    cases.check_gate(lib, precision, row)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ctx_gate_fp8_storage(lib, precision):
    cases.check_gate_fp8(lib, precision)


# ---- C
@pytest.mark.parametrize("name,variant", cases.C_IDS, ids=lambda v: str(v).replace(" ", "_"))
def test_slice_store_leaves_the_neighbours(lib, name, variant):
    cases.check_slice(lib, name, variant)


# ---- D
@pytest.mark.parametrize("exps", cases.D_EXPS, ids=lambda e: "%d_%d_%d" % e)
@pytest.mark.parametrize("form", ["A", "B", "C"])
def test_forms_under_the_activation_scale(lib, form, exps):
    cases.check_scaled(lib, form, exps)


def test_flagged_engine_with_zero_exponents_is_the_unflagged_one(lib):
    cases.check_scaled_zero_exponents(lib)


# ---- E: refused when the plan is built, before any launch
def test_refusals_at_plan_time(lib):
    cases.check_refusals(lib)
