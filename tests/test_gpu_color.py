"""Colour standards (BT.601 / BT.709, limited / full range), the I420 / YV12 / NV21 layouts and the mean chroma rule of vp_frame / vp_canvas on the MI355X.
Cases and the numpy oracle: tests/color_cases.py (the constants are rederived, and BT.601 full range compared with Pillow, in tests/test_color_host.py).
Everything here is bit for bit, on frames of a few dozen pixels or the 450 x 512 table."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import color_cases as kc  # noqa: E402

pytestmark = pytest.mark.gpu
STD_IDS = [kc.std_id(s) for s in kc.STANDARDS]
NEW_STD_IDS = [kc.std_id(s) for s in kc.NEW_STANDARDS]


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib as _lib

    return _lib


# ---- 1. upload, bit for bit through vp_frame_fetch_bgr8
@pytest.mark.parametrize("std", kc.STANDARDS, ids=STD_IDS)
@pytest.mark.parametrize("fmt,h,w,strides", kc.NEW_CONVERSION_CASES, ids=[c[0] for c in kc.NEW_CONVERSION_CASES])
def test_new_formats_bit_for_bit(lib, std, fmt, h, w, strides):
    kc.check_conversion(lib, std, fmt, h, w, strides)


@pytest.mark.parametrize("std", kc.NEW_STANDARDS, ids=NEW_STD_IDS)
@pytest.mark.parametrize("fmt,h,w,strides", kc.OLD_CONVERSION_CASES, ids=[c[0] for c in kc.OLD_CONVERSION_CASES])
def test_old_formats_under_new_standards(lib, std, fmt, h, w, strides):
    kc.check_conversion(lib, std, fmt, h, w, strides)


@pytest.mark.parametrize("std", kc.STANDARDS, ids=STD_IDS)
def test_table_frames(lib, std):
    """every YUV format under the new standards; under the default the new formats (the old ones: tests/test_gpu_frame.py)"""
    for fmt in kc.NEW_FORMATS if std == kc.DEFAULT else kc.ALL_YUV:
        kc.check_table(lib, std, fmt)


def test_more_than_one_workgroup_and_registered_pool(lib):
    """w % 4 == 2 over several workgroups, and one DMA per plane -- three of them -- out of a vp_register_frames pool"""
    for fmt, strides in (("i420", (491, 250, 243)), ("nv21", (488, 485))):
        kc.check_conversion(lib, ("bt709", "limited"), fmt, 270, 482, strides, seed=5)
    pool = np.random.default_rng(6).integers(0, 256, size=(3, 40, 96), dtype=np.uint8)
    lib.register_frames(pool)
    f = lib.Frame()
    try:
        f.set_color("bt601", "full")
        planes = [pool[0][:, :90], pool[1][:20, :45], pool[2][:20, :45]]
        f.upload(planes, "yv12", hw=(40, 90))
        assert np.array_equal(f.fetch_bgr8(), kc.to_bgr(("bt601", "full"), "yv12", planes, 40, 90))
    finally:
        f.close()
        lib.unregister_frames(pool)


@pytest.mark.parametrize("fmt", kc.NEW_FORMATS)
def test_flat_buffer_upload(lib, fmt):
    kc.check_flat_upload(lib, fmt)


# ---- 2. fetch, bit for bit
@pytest.mark.parametrize("std", kc.STANDARDS, ids=STD_IDS)
@pytest.mark.parametrize("fmt", kc.ALL_YUV + ("gray8",))
def test_fetch_bit_for_bit(lib, std, fmt):
    kc.check_fetch(lib, std, fmt)


def test_fetch_more_than_one_workgroup(lib):
    """66 x 130: w % 4 == 2, an odd number of four-pixel blocks a row (the planar chroma rows end inside a word), several workgroups"""
    import canvas_cases as cc

    bgr = cc.random_bgr(66, 130, 8)
    for fmt in kc.NEW_FORMATS:
        want = kc.from_bgr(("bt709", "full"), "mean", fmt, bgr)
        got = kc.fetch_planes(lib, ("bt709", "full"), "mean", fmt, bgr)
        assert len(got) == len(want) and all(np.array_equal(g, x) for g, x in zip(got, want)), fmt


def test_layout3(lib):
    kc.check_layout3(lib)


# ---- 3. round trip
@pytest.mark.parametrize("std", kc.STANDARDS, ids=STD_IDS)
def test_round_trip(lib, std):
    kc.check_roundtrip(lib, std)


# ---- 4. a consumer equals the host path
def test_sceneseg_consumer_from_an_i420_bt709_region(lib, state_dicts):
    from autoware_vision_pilot_amd import weights as vw

    eng = lib.Engine("sceneseg", vw.pack_state_dict(state_dicts("sceneseg")), precision="fp16")
    try:
        kc.check_consumer_equals_host(lib, eng, ("bt709", "limited"), "i420", 48, 64, (5, 7, 41, 29), (69, 35, 37))
    finally:
        eng.close()


# ---- 5. device upload
def test_device_upload_i420_from_a_torch_stream(lib):
    """three planes produced by torch on a side stream, handed over with that stream's handle: the bits of the host upload"""
    std, fmt, h, w = ("bt709", "limited"), "i420", 30, 46
    planes = kc.random_planes(fmt, h, w, (50, 27, 24), 40)
    parents = [p.base for p in planes]
    side = torch.cuda.Stream()
    f = lib.Frame()
    try:
        f.set_color(*std)
        with torch.cuda.stream(side):
            half = [torch.from_numpy(np.ascontiguousarray(p // 2)).cuda() for p in parents]
            rest = [torch.from_numpy(np.ascontiguousarray(p - p // 2)).cuda() for p in parents]
            dev = [a + b for a, b in zip(half, rest)]        # produced on the side stream
            handle = torch.cuda.current_stream().cuda_stream
            assert handle != 0
            f.upload_device([t.data_ptr() for t in dev], [t.stride(0) for t in dev], fmt, h, w, producer_stream=handle)
        got = f.fetch_bgr8()
        side.synchronize()
    finally:
        f.close()
    assert np.array_equal(got, kc.to_bgr(std, fmt, planes, h, w))


# ---- 6. refusals and state
def test_refusals_and_state(lib):
    kc.check_refusals_and_state(lib)
