"""vp_frame rectification on the MI355X: frame_remap_kernel through vp_op_remap_bgr8 and through the frame path (undistort + warp to the standard pose
behind the upload).  Cases and the numpy restatement of the definition: tests/rectify_cases.py.  Every comparison is bit for bit."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rectify_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib as _lib

    return _lib


@pytest.fixture(scope="module")
def seg(lib, state_dicts):
    """two SceneSeg fp16 engines on the same weights (the kind tests/test_gpu_frame.py feeds from a frame)"""
    from autoware_vision_pilot_amd import weights as vw

    blob = vw.pack_state_dict(state_dicts("sceneseg"))
    engs = [lib.Engine("sceneseg", blob, precision="fp16") for _ in range(2)]
    yield engs
    for e in engs:
        e.close()


# ---- 1. the kernel through vp_op_remap_bgr8
@pytest.mark.parametrize("which,dist_name", rc.MAP_CASES, ids=["-".join(c) for c in rc.MAP_CASES])
def test_kernel_case(lib, which, dist_name):
    rc.check_kernel_case(lib, which, dist_name)


def test_kernel_table(lib):
    rc.check_kernel_table(lib)


def test_kernel_edges(lib):
    rc.check_kernel_edges(lib)


def test_kernel_widths_and_padding(lib):
    rc.check_kernel_widths_and_padding(lib)


def test_kernel_wide(lib):
    rc.check_kernel_wide(lib)


def test_op_refusals(lib):
    rc.check_op_refusals(lib)


# ---- 2. the frame path
@pytest.mark.parametrize("mode", ["two_pass", "one_pass"])
@pytest.mark.parametrize("fmt", rc.FRAME_FORMATS)
def test_frame_rectified(lib, fmt, mode):
    rc.check_frame_rectified(lib, fmt, mode)


def test_frame_single_passes(lib):
    rc.check_frame_single_passes(lib)


@pytest.mark.parametrize("fmt", rc.FRAME_FORMATS)
def test_frame_identity_setting_is_todays_picture(lib, fmt):
    rc.check_frame_identity_setting(lib, fmt)


def test_setting_applies_to_later_uploads(lib):
    rc.check_setting_applies_to_later_uploads(lib)


def test_geometry_change_rebuilds_the_maps(lib):
    rc.check_geometry_change_rebuilds_the_maps(lib)


def test_consumer_of_rectified_frame_equals_host_path(lib, seg):
    rc.check_consumer_of_rectified_frame(lib, seg[0])


def test_canvas_has_out_geometry(lib):
    rc.check_canvas_has_out_geometry(lib)


def test_reupload_keeps_the_ordering(lib, seg):
    """the first round captures the engines' graphs for the geometry, the second replays them: no host wait is left between the uploads"""
    rc.check_reupload_keeps_the_ordering(lib, seg[0], seg[1], rc.BIG_HW, rc.BIG_OUT_HW, rc.BIG_K, rc.FRAME_DIST, rc.BIG_H)
