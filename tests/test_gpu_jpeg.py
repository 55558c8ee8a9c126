"""The canvas's JPEG encoder on the MI355X: vp_op_jpeg_encode_bgr8 on every case of tests/jpeg_cases.py and the canvas entries (vp_canvas_fetch_jpeg,
vp_canvas_fetch_jpeg_resized) byte for byte against the numpy twin of the rules in include/vp_hip.h (tests/jpeg_ref.py), and every refusal."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_cases as jc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib as _lib

    return _lib


@pytest.mark.parametrize("case", jc.CASES, ids=jc.case_id)
def test_operator_equals_the_twin(lib, case):
    jc.check_operator(lib, case)


def test_canvas_fetch_jpeg(lib):
    """behind begin + blend_mask_u8 + draw_points with no sync of the caller's: equal to the operator entry on fetch(BGR8) and to the twin fed fetch(I420)
    under (BT.601, full, mean); unchanged by set_color; the canvas unchanged; equal on every call; the resized form; a second begin at another geometry"""
    jc.check_canvas(lib)


def test_production_display_size(lib):
    """fetch_jpeg_resized(90, 160), a 1/8 of the production display's 1280 x 720, from a larger canvas equals the operator entry on fetch_resized(BGR8)"""
    import canvas_cases as cc

    with cc.OnCanvas(lib, jc.picture("frame", 176, 320)) as oc:
        jc.drawn_canvas(lib, oc)
        small = oc.canvas.fetch("bgr8", size=(90, 160))
        got = oc.canvas.fetch_jpeg(90, 0, size=(90, 160))
        assert got == lib.jpeg_encode(small, 90, 0) == jc.ref.encode(small, 90, 0)


def test_operator_refusals(lib):
    jc.check_operator_refusals(lib)


def test_canvas_refusals(lib):
    jc.check_canvas_refusals(lib)
