"""Colour standards and the I420 / YV12 / NV21 layouts of vp_frame / vp_canvas without a GPU: the constants of include/vp_hip.h rederived from (Kr, Kb),
the numpy restatement that every conversion test uses as its oracle (anchors, grey, monotone, the default equals the existing restatements; BT.601 full
range against Pillow), and -- on the HIP-on-CPU emulation of the real kernel and engine code (tests/emul) -- uploads, fetches, the round trip, one
consumer and the refusals.  Cases: tests/color_cases.py."""
import ctypes as ct
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
import abi  # noqa: E402
import canvas_cases as cc  # noqa: E402
import color_cases as kc  # noqa: E402
import frame_cases as fc  # noqa: E402

NEW_SYMBOLS = ("vp_frame_set_color", "vp_frame_get_color", "vp_canvas_set_color", "vp_canvas_get_color", "vp_canvas_layout3")
STD_IDS = [kc.std_id(s) for s in kc.STANDARDS]
NEW_STD_IDS = [kc.std_id(s) for s in kc.NEW_STANDARDS]


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
def test_new_symbols_and_codes_are_declared_exported_and_bound():
    from autoware_vision_pilot_amd import lib

    src = abi.header_source()
    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in exported and s in lib.EXPORTED_SYMBOLS, s
    for name, code in kc.CODES.items():
        assert lib.FRAME_FORMATS[name] == code and f"VP_FRAME_{name.upper()} = {code}" in src
    assert not set(lib.FRAME_FORMATS.values()) & set(range(8, 16))          # 8 .. 15 stay unknown
    for text in ("VP_COLOR_BT601 = 0, VP_COLOR_BT709 = 1", "VP_COLOR_RANGE_LIMITED = 0, VP_COLOR_RANGE_FULL = 1", "VP_CHROMA_EVEN = 0, VP_CHROMA_MEAN = 1"):
        assert text in src
    assert (lib.VP_COLOR_BT709, lib.VP_COLOR_RANGE_FULL, lib.VP_CHROMA_MEAN) == (1, 1, 1)


def test_header_states_every_constant():
    """both tables of include/vp_hip.h, row by row, are the ones the oracle uses"""
    text = open(abi.HEADER).read()
    rows = {}
    for m in re.finditer(r"\*\s+BT\.(601|709) (limited|full)\s+((?:-?\d+\s+)+)", text):
        rows.setdefault(("bt" + m.group(1), m.group(2)), []).append(tuple(int(v) for v in m.group(3).split()))
    for std in kc.STANDARDS:
        off, yk, uk, vk = kc.FORWARD[std]
        assert sorted(rows[std], key=len) == [kc.INVERSE[std], (off,) + yk + uk + vk], std


# ---- the constants and the restatement (pure numpy)
@pytest.mark.parametrize("std", kc.NEW_STANDARDS, ids=NEW_STD_IDS)
def test_constants_rederived_from_kr_kb(std):
    inv, fwd = kc.derive(*std)
    assert inv == kc.INVERSE[std]
    assert fwd == kc.FORWARD[std]


def test_default_constants_are_opencvs_not_the_derived_ones():
    """the BT.601 limited row stays what it was: within 1e-3 relative of the derived constants, but not equal to them"""
    inv, fwd = kc.derive(*kc.DEFAULT)
    assert inv != kc.INVERSE[kc.DEFAULT] and fwd != kc.FORWARD[kc.DEFAULT]
    for a, b in zip(inv[1:], kc.INVERSE[kc.DEFAULT][1:]):
        assert abs(a - b) <= 2e-3 * abs(a)


@pytest.mark.parametrize("std", kc.STANDARDS, ids=STD_IDS)
def test_restatement_anchors_grey_monotone_and_headroom(std):
    off = kc.INVERSE[std][0]
    white = 235 if off else 255
    assert kc.yuv_to_bgr(std, off, 128, 128).tolist() == [0, 0, 0]
    assert kc.yuv_to_bgr(std, white, 128, 128).tolist() == [255, 255, 255]
    assert [int(c) for c in kc.bgr_to_yuv(std, np.array([0, 0, 0]))] == [off, 128, 128]
    assert [int(c) for c in kc.bgr_to_yuv(std, np.array([255, 255, 255]))] == [white, 128, 128]
    lv = np.arange(256)
    y, u, v = kc.bgr_raw(std, lv, lv, lv)                        # grey: exactly (128, 128) at all 256 levels
    assert (u == 128).all() and (v == 128).all() and (np.diff(y) >= 0).all()
    for ch in range(3):                                          # Y monotone in each channel, the other two at either end
        for rest in (0, 255):
            rgb = [np.full(256, rest)] * 3
            rgb[ch] = lv
            assert (np.diff(kc.bgr_raw(std, *rgb)[0]) >= 0).all(), (std, ch, rest)
    for uu in fc.UV_GRID:                                        # and the inverse monotone in Y, flat below `off`
        for vv in fc.UV_GRID:
            px = kc.yuv_to_bgr(std, lv, np.full(256, uu), np.full(256, vv)).astype(np.int64)
            assert (np.diff(px, axis=0) >= 0).all() and (px[:off + 1] == px[0]).all()
    # 32-bit arithmetic has room: |pre-shift| < 2^30 means |result| < 2^10 for every byte input
    Y, U, V = np.meshgrid(lv, lv, lv, indexing="ij", sparse=True)
    for c in kc.yuv_raw(std, Y, U, V) + kc.bgr_raw(std, Y, U, V):
        assert -(1 << 10) < int(c.min()) and int(c.max()) < (1 << 10)
    if off == 0:                                                 # full range: pure blue / pure red reach 256, the clamp decides
        assert int(kc.bgr_raw(std, 0, 0, 255)[1]) == 256 and int(kc.bgr_raw(std, 255, 0, 0)[2]) == 256
    else:
        _, u, v = kc.bgr_raw(std, Y, U, V)
        assert 0 <= int(min(u.min(), v.min())) and int(max(u.max(), v.max())) <= 255


def test_default_restatement_equals_the_existing_ones_on_the_table():
    planes, h, w = fc.table_planes("nv12")
    Y = planes[0]
    uv = planes[1].reshape(h // 2, w // 2, 2).repeat(2, axis=0).repeat(2, axis=1)
    assert np.array_equal(kc.yuv_to_bgr(kc.DEFAULT, Y, uv[..., 0], uv[..., 1]), fc.yuv_to_bgr(Y, uv[..., 0], uv[..., 1]))
    for fmt in fc.YUV:
        p, hh, ww = fc.table_planes(fmt)
        assert np.array_equal(kc.to_bgr(kc.DEFAULT, fmt, p, hh, ww), fc.to_bgr(fmt, p, hh, ww)), fmt
    bgr = fc.to_bgr("nv12", planes, h, w)
    for a, b in zip(kc.bgr_to_yuv(kc.DEFAULT, bgr), cc.bgr_to_yuv(bgr)):
        assert np.array_equal(a, b)
    for fmt in ("gray8",) + fc.YUV:
        for a, b in zip(kc.from_bgr(kc.DEFAULT, "even", fmt, bgr), cc.from_bgr(fmt, bgr)):
            assert np.array_equal(a, b), fmt


def test_bt601_full_range_against_pillow():
    """Pillow's convert("YCbCr") is JFIF: BT.601 full range, its own fixed point.  On the grid {0, 5, .., 255}^3 every channel within 1, both directions."""
    from PIL import Image

    std = ("bt601", "full")
    g = np.arange(0, 256, 5, dtype=np.uint8)
    a, b, c = (x.reshape(-1, 1) for x in np.meshgrid(g, g, g, indexing="ij"))
    rgb = np.concatenate([a, b, c], axis=1).reshape(-1, 52, 3)
    size = (rgb.shape[1], rgb.shape[0])
    ycc = np.asarray(Image.frombytes("RGB", size, rgb.tobytes()).convert("YCbCr")).astype(np.int64)
    ours = np.stack(kc.bgr_to_yuv(std, rgb[..., ::-1]), axis=-1).astype(np.int64)
    d = np.abs(ours - ycc).max()
    print("forward max |ours - Pillow| =", d)
    assert d <= 1
    back = np.asarray(Image.frombytes("YCbCr", size, rgb.tobytes()).convert("RGB")).astype(np.int64)       # the same grid read as (Y, Cb, Cr)
    ours = kc.yuv_to_bgr(std, rgb[..., 0], rgb[..., 1], rgb[..., 2])[..., ::-1].astype(np.int64)
    d = np.abs(ours - back).max()
    print("inverse max |ours - Pillow| =", d)
    assert d <= 1


# ---- the emulated library
@pytest.mark.parametrize("std", kc.STANDARDS, ids=STD_IDS)
@pytest.mark.parametrize("fmt,h,w,strides", kc.NEW_CONVERSION_CASES, ids=[c[0] for c in kc.NEW_CONVERSION_CASES])
def test_new_formats_bit_for_bit_emulated(emu_lib, std, fmt, h, w, strides):
    kc.check_conversion(emu_lib, std, fmt, h, w, strides)


@pytest.mark.parametrize("std", kc.NEW_STANDARDS, ids=NEW_STD_IDS)
@pytest.mark.parametrize("fmt,h,w,strides", kc.OLD_CONVERSION_CASES, ids=[c[0] for c in kc.OLD_CONVERSION_CASES])
def test_old_formats_under_new_standards_emulated(emu_lib, std, fmt, h, w, strides):
    kc.check_conversion(emu_lib, std, fmt, h, w, strides)


@pytest.mark.parametrize("std", kc.STANDARDS, ids=STD_IDS)
def test_table_frames_emulated(emu_lib, std):
    """every YUV format under the new standards; under the default the new formats (the old ones: tests/test_frame_host.py)"""
    for fmt in kc.NEW_FORMATS if std == kc.DEFAULT else kc.ALL_YUV:
        kc.check_table(emu_lib, std, fmt)


@pytest.mark.parametrize("fmt", kc.NEW_FORMATS)
def test_flat_buffer_upload_emulated(emu_lib, fmt):
    kc.check_flat_upload(emu_lib, fmt)


@pytest.mark.parametrize("std", kc.STANDARDS, ids=STD_IDS)
@pytest.mark.parametrize("fmt", kc.ALL_YUV + ("gray8",))
def test_fetch_bit_for_bit_emulated(emu_lib, std, fmt):
    kc.check_fetch(emu_lib, std, fmt)


def test_more_than_one_workgroup_emulated(emu_lib):
    """w % 4 == 2 over several workgroups; 66 x 130: an odd number of four-pixel blocks a row (the planar chroma rows of the fetch end inside a word)"""
    for fmt, strides in (("i420", (491, 250, 243)), ("nv21", (488, 485))):
        kc.check_conversion(emu_lib, ("bt709", "limited"), fmt, 270, 482, strides, seed=5)
    bgr = cc.random_bgr(66, 130, 8)
    for fmt in kc.NEW_FORMATS:
        want = kc.from_bgr(("bt709", "full"), "mean", fmt, bgr)
        got = kc.fetch_planes(emu_lib, ("bt709", "full"), "mean", fmt, bgr)
        assert len(got) == len(want) and all(np.array_equal(g, x) for g, x in zip(got, want)), fmt


def test_layout3_emulated(emu_lib):
    kc.check_layout3(emu_lib)


@pytest.mark.parametrize("std", kc.STANDARDS, ids=STD_IDS)
def test_round_trip_emulated(emu_lib, std):
    kc.check_roundtrip(emu_lib, std)


def test_consumer_equals_host_path_emulated(emu_lib):
    """AutoDrive (fp16), odd offset and odd size out of an I420 BT.709 limited-range frame"""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    eng = emu_lib.Engine("autodrive", vw.pack_state_dict(synthetic.make_autodrive_state_dict(0)), precision="fp16")
    try:
        kc.check_consumer_equals_host(emu_lib, eng, ("bt709", "limited"), "i420", 48, 64, (5, 7, 41, 29), (69, 35, 37))
    finally:
        eng.close()


def test_refusals_and_state_emulated(emu_lib):
    kc.check_refusals_and_state(emu_lib)
