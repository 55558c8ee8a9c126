"""The production display on vp_canvas without a GPU: the ABI (header, shared library, binding), the anchors of the restated rules (the lane increments
against both float32 spellings of addWeighted, the row positions against numpy.linspace, the disc of radius 3) and -- on the HIP-on-CPU emulation of the
real kernel and engine code (tests/emul) -- the operator entries bit for bit on the small cases of tests/display_cases.py, their refusals, and one EgoLanes
pass whose overlay equals the restatement on the logits vp_logits returns."""
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
import display_cases as dc  # noqa: E402

NEW_SYMBOLS = ("vp_canvas_add_planes_f32", "vp_canvas_overlay_lanes", "vp_canvas_draw_points", "vp_canvas_draw_lane_rows", "vp_canvas_fetch_resized")


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
    for m in ("overlay_lanes", "add_planes", "draw_lane_rows", "draw_points", "fetch"):
        assert callable(getattr(lib.Canvas, m)), m
    assert "size" in lib.Canvas.fetch.__code__.co_varnames


def test_lane_increments_are_both_float32_addweighted_spellings():
    """addWeighted(image, 1.0, colour, 0.4) on a byte: the same increment for every byte value, and no value within 0.25 of a tie"""
    d = np.arange(256)
    for colour, add in zip(dc.LANE_COLOURS, dc.LANE_ADD):
        for ch in range(3):
            for fused in (False, True):
                t = dc.addweighted_1_04(d, np.full(256, colour[ch]), fused).astype(np.float64)
                assert np.array_equal(np.rint(t).astype(np.int64), d + add[ch]), (colour, ch, fused)
                assert (np.abs(t - np.floor(t) - 0.5) > 0.25).all()
                assert np.array_equal(np.clip(np.rint(t), 0, 255), np.minimum(255, d + add[ch]))


def test_one_clamped_sum_equals_the_sequential_overlays_in_any_order():
    import itertools

    bgr, planes = cc.random_bgr(9, 13, 3), dc.random_planes(3, 3, 5, 4)
    bgr[:3] = 250                                         # close to the clamp: two planes together pass it
    region = (1, 0, 11, 8)
    want = dc.add_planes(bgr, planes, -0.5, dc.LANE_ADD, region)
    on = dc.planes_on(planes, -0.5, region)
    assert (on.sum(axis=0) >= 2).any() and (want == 255).any()
    for order in itertools.permutations(range(3)):
        assert np.array_equal(dc.add_planes_sequential(bgr, planes, -0.5, dc.LANE_ADD, region, order), want), order
    assert np.array_equal(want[:, :1], bgr[:, :1]) and np.array_equal(want[8:], bgr[8:])      # outside the region: untouched


def test_row_positions_are_numpy_linspace():
    assert np.array_equal(np.array([i * 511 // 63 for i in range(64)]), np.linspace(0, 511, 64, dtype=int))


def test_disc_of_radius_3_is_the_29_pixel_set():
    d = dc.disc(3)
    assert len(d) == 29
    for dy, half in ((0, 3), (1, 2), (2, 2), (3, 0)):
        for s in (dy, -dy):
            assert sorted(dx for dx, y in d if y == s) == list(range(-half, half + 1))
    assert dc.disc(0) == {(0, 0)}
    got = dc.draw_points(np.zeros((9, 9, 3), np.uint8), [(4, 4)], 3, (1, 2, 3))
    assert {(x - 4, y - 4) for y, x in np.argwhere(got[..., 0] == 1)} == d


def test_lane_row_points_restatement():
    logits = np.zeros((2, 64), np.float32)
    logits[0] = np.linspace(-0.1, 1.1, 64, dtype=np.float32)
    logits[1] = 0.5
    logits[1, 5], logits[1, 6] = np.nextafter(np.float32(0.5), np.float32(0)), np.nan
    logits[0, 7], logits[0, 8], logits[0, 9] = np.nan, np.inf, 1e6
    pts = dc.lane_row_points(logits, (10, 20))
    assert len(pts) == 64 - 5 and pts[0] == (10 + int(np.float32(-0.1) * np.float32(1024)), 20) and pts[-1][1] == 20 + 511
    assert pts[0][0] == 10 - 102                           # truncation toward zero, not floor


def test_identity_resize_is_the_identity():
    bgr = cc.random_bgr(11, 14, 1)
    assert np.array_equal(dc.resized(bgr, (11, 14)), bgr)


@pytest.mark.parametrize("hw,shape,region", dc.ADD_CASES, ids=dc.ADD_IDS)
def test_add_planes_bit_for_bit_emulated(emu_lib, hw, shape, region):
    dc.check_add(emu_lib, hw, shape, region)


@pytest.mark.parametrize("hw", cc.CANVAS_SIZES, ids=["%dx%d" % s for s in cc.CANVAS_SIZES])
def test_points_bit_for_bit_emulated(emu_lib, hw):
    dc.check_points(emu_lib, hw)


@pytest.mark.parametrize("hw,size", dc.RESIZE_CASES, ids=["%dx%d-%dx%d" % (c[0] + c[1]) for c in dc.RESIZE_CASES])
def test_fetch_resized_bit_for_bit_emulated(emu_lib, hw, size):
    dc.check_resize(emu_lib, hw, size)


@pytest.mark.parametrize("mode", dc.CHROMA_MODES)
@pytest.mark.parametrize("fmt", dc.YUV_FORMATS)
def test_fetch_resized_yuv_bit_for_bit_emulated(emu_lib, fmt, mode):
    for hw, size in dc.EVEN_TARGETS:
        dc.check_resize_yuv(emu_lib, hw, size, fmt, mode)
    if fmt == "yuy2":
        dc.check_resize_yuv(emu_lib, (7, 5), (3, 2), fmt, mode)


def test_every_kernel_on_more_than_one_workgroup_emulated(emu_lib):
    dc.check_big(emu_lib)


def test_refusals_emulated(emu_lib):
    dc.check_display_refusals(emu_lib)


def test_engine_lane_rows_emulated(emu_lib):
    """One emulated AutoSteer pass (fp16, eager) on a fixture frame placed at an odd origin of a larger frame: draw_lane_rows equals the restatement on
    the fetched logits.  Then the engine's "device" logits (host memory under the emulation) are overwritten with rows of the test's choosing: xp left and
    right of the frame, NaN, infinities, a product beyond the pixel range, h_vector at 0.5, just below it and NaN."""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    g = np.load(os.path.join(HERE, "golden", "autosteer_net.npz"))
    eng = emu_lib.Engine("autosteer", vw.pack_state_dict(synthetic.make_autosteer_state_dict(int(g["weight_seed"]))), precision="fp16")
    origin = (9, 13)
    bgr = cc.random_bgr(530, 1040, 6)
    bgr[13:13 + 512, 9:9 + 1024] = synthetic.synthetic_frame(512, 1024, int(g["frame_seeds"][0]))
    try:
        eng._ck(eng._lib.vp_use_graph(eng._h, 0))
        with cc.OnCanvas(emu_lib, bgr) as oc:
            c, f = oc.canvas, oc.frame
            with pytest.raises(emu_lib.VpError, match="Inference has not been run yet"):
                c.draw_lane_rows(eng)
            with pytest.raises(ValueError, match="VP_EGOLANES engines only"):
                c.overlay_lanes(eng, 0.0)
            eng.infer_frame(f, origin + (1024, 512))
            logits = eng.logits().copy()
            assert 1 <= len(dc.lane_row_points(logits, origin)) <= 63
            c.draw_lane_rows(eng)
            got, want = c.fetch("bgr8"), dc.draw_lane_rows(bgr, logits, origin)
            assert np.array_equal(got, want) and not np.array_equal(got, bgr)
            made = np.zeros((2, 64), np.float32)
            made[0] = np.linspace(-0.2, 1.2, 64, dtype=np.float32)
            made[1] = 0.75
            made[1, 4], made[1, 5], made[1, 6] = 0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nan
            made[0, 7], made[0, 8], made[0, 9], made[0, 10] = np.nan, np.inf, -np.inf, 1e6
            assert len(dc.lane_row_points(made, origin)) == 58
            ct.memmove(eng.device_outputs()[0], made.ctypes.data, made.nbytes)
            c.begin(f)
            c.draw_lane_rows(eng)
            assert np.array_equal(c.fetch("bgr8"), dc.draw_lane_rows(bgr, made, origin))
    finally:
        eng.close()


def test_engine_overlay_lanes_emulated(emu_lib):
    """One emulated EgoLanes pass (fp16) on an odd region of a larger frame: overlay_lanes at the median logit (about half of the samples on) equals the
    restatement on the fetched logits, pixels outside the region are the frame's; the kind, geometry and first-pass refusals."""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    eng = emu_lib.Engine("egolanes", vw.pack_state_dict(synthetic.make_state_dict("egolanes", 2)), precision="fp16")
    bgr = cc.random_bgr(40, 64, 4)
    region = (5, 7, 41, 29)
    try:
        eng._ck(eng._lib.vp_use_graph(eng._h, 0))          # one eager pass is enough here
        with cc.OnCanvas(emu_lib, bgr) as oc:
            c, f = oc.canvas, oc.frame
            with pytest.raises(emu_lib.VpError, match="Inference has not been run yet"):
                c.overlay_lanes(eng, 0.0)
            with pytest.raises(ValueError, match="VP_AUTOSTEER engines only"):
                c.draw_lane_rows(eng)
            eng.infer_frame(f, region)
            logits = eng.logits().copy()
            t = float(np.median(logits))
            c.overlay_lanes(eng, t)
            got, want = c.fetch("bgr8"), dc.overlay_lanes(bgr, logits, t, region)
            assert np.array_equal(got, want)
            on = dc.planes_on(logits.reshape(3, 80, 160), t, region)
            assert 0.2 < on.mean() < 0.8 and (on.sum(axis=0) >= 2).any()      # the median: about half of the samples on, some pixels in two planes
            assert np.array_equal(got[:7], bgr[:7]) and np.array_equal(got[:, :5], bgr[:, :5]) and not np.array_equal(got, bgr)
            with pytest.raises(ValueError, match="threshold"):
                c.overlay_lanes(eng, float("nan"))
            f.upload(cc.random_bgr(42, 64, 4), "bgr8")
            c.begin(f)
            with pytest.raises(ValueError, match="64 x 40 frame.*64 x 42 picture"):
                c.overlay_lanes(eng, t)
    finally:
        eng.close()
