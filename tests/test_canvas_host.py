"""vp_canvas without a GPU: the ABI (header, shared library, binding), vp_canvas_layout (host only), the anchors of the two restated definitions (boxes,
forward YUV) and -- on the HIP-on-CPU emulation of the real kernel and engine code (tests/emul) -- the operator entry, the boxes, every fetch format and
one engine pass whose overlay equals vp_visualize_mask_bgr8."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
import abi  # noqa: E402
import canvas_cases as cc  # noqa: E402

NEW_SYMBOLS = ("vp_canvas_create", "vp_canvas_destroy", "vp_canvas_last_error", "vp_canvas_begin", "vp_canvas_blend_mask", "vp_canvas_blend_mask_u8",
               "vp_canvas_paste_depth", "vp_canvas_draw_detections", "vp_canvas_sync", "vp_canvas_dims", "vp_canvas_device", "vp_canvas_layout", "vp_canvas_fetch")


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


def test_new_symbols_are_declared_exported_and_bound():
    from autoware_vision_pilot_amd import lib

    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in exported, s
        assert s in lib.EXPORTED_SYMBOLS, s
    for m in ("begin", "blend_mask", "blend_mask_u8", "paste_depth", "draw_detections", "fetch", "device", "sync", "hw"):
        assert callable(getattr(lib.Canvas, m)), m


@pytest.mark.parametrize("fmt", cc.FORMATS)
def test_layout_against_the_case_table(fmt):
    """host only: no device, no emulation -- the shipped library answers"""
    from autoware_vision_pilot_amd import lib

    for h, w in cc.LAYOUT_SIZES:
        want = cc.layout(fmt, h, w)
        if want is None:
            with pytest.raises(ValueError):
                lib.canvas_layout(fmt, h, w)
        else:
            assert lib.canvas_layout(fmt, h, w) == want, (fmt, h, w)


def test_layout_refuses_unknown_formats_and_null_outputs():
    from autoware_vision_pilot_amd import lib

    so = lib.load()
    n, rb, rows = ct.c_int(), (ct.c_int * 2)(), (ct.c_int * 2)()
    for f in (-1, 8, 99):
        assert so.vp_canvas_layout(f, 4, 4, ct.byref(n), rb, rows) == -1
    assert so.vp_canvas_layout(0, 4, 4, None, rb, rows) == -1
    assert so.vp_canvas_layout(0, 4, 4, ct.byref(n), rb, rows) == 0 and (n.value, rb[0], rows[0]) == (1, 12, 4)


def test_forward_yuv_anchors():
    px = lambda b, g, r: tuple(int(c) for c in cc.bgr_to_yuv(np.array([b, g, r], np.uint8)))   # noqa: E731
    assert px(0, 0, 0) == (16, 128, 128)
    assert px(255, 255, 255) == (235, 128, 128)
    assert px(0, 0, 255)[2] == 240           # pure red: V
    assert px(255, 0, 0)[1] == 240           # pure blue: U
    for g in range(256):                     # grey stays grey
        assert px(g, g, g)[1:] == (128, 128)


def test_forward_yuv_y_is_monotone_in_each_channel():
    v = np.arange(256)
    for a in (0, 1, 127, 128, 254, 255):
        for b in (0, 77, 255):
            A, B = np.full(256, a), np.full(256, b)
            for rgb in ((v, A, B), (A, v, B), (A, B, v)):
                assert (np.diff(cc.yuv_raw(*rgb)[0]) >= 0).all()


def test_forward_yuv_range_and_clamps():
    """Over the byte grid the limited range is reached exactly and never left -- Y 16 .. 235, U and V 16 .. 240 -- so for byte input the clamp decides
    nothing; it is live for the arithmetic all the same: both ends of every component are reached just outside the byte grid, and clipped."""
    R, G, B = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij", sparse=True)
    for c, lo, hi in zip(cc.yuv_raw(R, G, B), (16, 16, 16), (235, 240, 240)):
        c = np.broadcast_to(c, (256, 256, 256))
        assert (int(c.min()), int(c.max())) == (lo, hi)
    wide = np.arange(-600, 900, 25)
    R, G, B = np.meshgrid(wide, wide, wide, indexing="ij", sparse=True)
    for c in cc.yuv_raw(R, G, B):
        c = np.broadcast_to(c, (len(wide),) * 3)
        assert c.min() < 0 and c.max() > 255
        assert abs(int(c.min())) < (1 << 11) and int(c.max()) < (1 << 11)     # 32-bit arithmetic has room: |sum| < 2^31


def test_box_fill_agrees_with_both_float32_addweighted_spellings():
    d = np.arange(256)
    for colour in (0, 255):
        want = cc.fill_fifth(colour, d)
        assert np.array_equal(cc.fill_addweighted(np.full(256, colour), d, fused=False), want)
        assert np.array_equal(cc.fill_addweighted(np.full(256, colour), d, fused=True), want)
        assert ((2 * colour + 8 * d) % 10 != 5).all()      # never a tie


def test_box_restatement_on_a_hand_made_case():
    """a 3 x 3 box cut by the left border of a 4 x 5 canvas of 100s, class 1 (red): the left side is outside and stays open"""
    got = cc.draw_boxes(np.full((4, 5, 3), 100, np.uint8), [cc.det(-1.5, 0.9, 2.2, 3.0, 1)])     # bx -1, by 0, bw 3, bh 2 -> x -1 .. 1, y 0 .. 1
    red, fill = [0, 0, 255], [80, 80, 131]
    assert got[0, :2].tolist() == [red, red] and got[1, :2].tolist() == [red, red]               # rows 0 and 1 are both outline rows
    assert (got[2:] == 100).all() and (got[:2, 2:] == 100).all()
    got = cc.draw_boxes(np.full((5, 5, 3), 100, np.uint8), [cc.det(-1.5, 0, 2.2, 3.5, 1)])       # x -1 .. 1, y 0 .. 2
    assert got[1, 0].tolist() == fill and got[1, 1].tolist() == red and got[0, 0].tolist() == red and got[2, 0].tolist() == red


@pytest.mark.parametrize("hw,mhw,region,viz", cc.BLEND_CASES, ids=["%dx%d-%dx%d-%d.%d.%d.%d-%d" % (c[0] + c[1] + c[2] + (c[3],)) for c in cc.BLEND_CASES])
def test_blend_mask_u8_bit_for_bit_emulated(emu_lib, hw, mhw, region, viz):
    cc.check_blend(emu_lib, hw, mhw, region, viz)


@pytest.mark.parametrize("hw", cc.CANVAS_SIZES, ids=["%dx%d" % s for s in cc.CANVAS_SIZES])
def test_boxes_bit_for_bit_emulated(emu_lib, hw):
    cc.check_boxes(emu_lib, hw)


@pytest.mark.parametrize("fmt", cc.FORMATS)
def test_fetch_bit_for_bit_emulated(emu_lib, fmt):
    for hw in cc.FETCH_SIZES.get(fmt, cc.CANVAS_SIZES):
        cc.check_fetch(emu_lib, fmt, hw)


def test_refusals_emulated(emu_lib):
    cc.check_canvas_refusals(emu_lib)


def test_engine_overlay_equals_visualize_mask_emulated(emu_lib):
    """One emulated EgoLanes pass (fp16, VP_DECODE_LANE_LABEL) on an odd region of a larger frame: the region of a fresh canvas equals
    vp_visualize_mask_bgr8, the rest is the frame; then the engine refusals that need a pass."""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    eng = emu_lib.Engine("egolanes", vw.pack_state_dict(synthetic.make_state_dict("egolanes", 2)), precision="fp16")
    try:
        eng.set_decode_mode(emu_lib.VP_DECODE_LANE_LABEL)
        eng._ck(eng._lib.vp_use_graph(eng._h, 0))          # one eager pass is enough here
        cc.check_engine_region(emu_lib, eng, emu_lib.VP_VIZ_EGOLANES, (40, 64), (5, 7, 41, 29), before_first_pass=True)
    finally:
        eng.close()
