"""The production display on vp_canvas on the MI355X: the additive lane overlay (operator and EgoLanes engine entry), points and the AutoSteer lane rows,
and the resized fetch.  Cases and numpy restatements: tests/display_cases.py (shared with tests/test_display_host.py).  Every comparison is equality of
bytes: against the restatement applied to the logits vp_logits returns, to the boxes' restatement of tests/canvas_cases.py and to
oracle.pre_post.resize_bilinear_u8."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import canvas_cases as cc  # noqa: E402
import display_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu
H, W = 720, 1280
LANES = (0, 420, 1280, 300)     # the production app's EgoLanes crop: rows >= 420 (main.cpp:497-505)
G = np.load(os.path.join(HERE, "golden", "autosteer_net.npz"))
STEER_SEEDS = [int(s) for s in G["frame_seeds"]]


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib as _lib

    return _lib


@pytest.fixture(scope="module")
def ego(lib, state_dicts):
    from autoware_vision_pilot_amd import weights as vw

    eng = lib.Engine("egolanes", vw.pack_state_dict(state_dicts("egolanes")), precision="fp16")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def steer(lib):
    from autoware_vision_pilot_amd import synthetic, weights as vw

    eng = lib.Engine("autosteer", vw.pack_state_dict(synthetic.make_autosteer_state_dict(int(G["weight_seed"]))), precision="fp16x3")
    yield eng
    eng.close()


def steer_frame(seed):
    from autoware_vision_pilot_amd import synthetic

    return synthetic.synthetic_frame(512, 1024, seed)


def device_pointer(a):
    """a float32 array in device memory: (pointer, the tensor that keeps it alive)"""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


# ---- 1. kernel shapes through the operator entries
@pytest.mark.parametrize("hw,shape,region", dc.ADD_CASES, ids=dc.ADD_IDS)
def test_add_planes_bit_for_bit_from_host_and_device_memory(lib, hw, shape, region):
    dc.check_add(lib, hw, shape, region, device_pointer=device_pointer)


@pytest.mark.parametrize("hw", cc.CANVAS_SIZES, ids=["%dx%d" % s for s in cc.CANVAS_SIZES])
def test_points_bit_for_bit(lib, hw):
    dc.check_points(lib, hw)


@pytest.mark.parametrize("hw,size", dc.RESIZE_CASES, ids=["%dx%d-%dx%d" % (c[0] + c[1]) for c in dc.RESIZE_CASES])
def test_fetch_resized_bit_for_bit(lib, hw, size):
    dc.check_resize(lib, hw, size)


@pytest.mark.parametrize("mode", dc.CHROMA_MODES)
@pytest.mark.parametrize("fmt", dc.YUV_FORMATS)
def test_fetch_resized_yuv_bit_for_bit(lib, fmt, mode):
    for hw, size in dc.EVEN_TARGETS:
        dc.check_resize_yuv(lib, hw, size, fmt, mode)
    if fmt == "yuy2":
        dc.check_resize_yuv(lib, (7, 5), (3, 2), fmt, mode)


def test_every_kernel_on_more_than_one_workgroup(lib):
    dc.check_big(lib)
    dc.check_big(lib, seed=12, device_pointer=device_pointer)


def test_refusals_without_an_engine(lib):
    dc.check_display_refusals(lib)


# ---- 2. engines
def test_overlay_lanes_on_the_production_crop(lib, ego):
    """EgoLanes on rows >= 420 of a 720p frame; the threshold is the median of the fetched logits, so about half of the samples are on.  Any decode mode:
    only the logits are read."""
    from autoware_vision_pilot_amd import synthetic

    bgr = synthetic.synthetic_frame(H, W, 17)
    with cc.OnCanvas(lib, bgr) as oc:
        c, f = oc.canvas, oc.frame
        ego.infer_frame(f, LANES)
        logits = ego.logits().copy()
        assert logits.size == 3 * 80 * 160
        t = float(np.median(logits))
        want = dc.overlay_lanes(bgr, logits, t, LANES)
        on = dc.planes_on(logits.reshape(3, 80, 160), t, LANES)
        assert 0.2 < on.mean() < 0.8 and (on.sum(axis=0) >= 2).any()
        for mode in (lib.VP_DECODE_SEG_MASK, lib.VP_DECODE_LANE_LABEL):
            ego.set_decode_mode(mode)
            c.begin(f)
            c.overlay_lanes(ego, t)
            got = c.fetch("bgr8")
            assert np.array_equal(got, want), np.argwhere(got != want)[:4]
        assert np.array_equal(got[:LANES[1]], bgr[:LANES[1]]) and not np.array_equal(got[LANES[1]:], bgr[LANES[1]:])      # outside the crop: untouched


@pytest.mark.parametrize("fi,origin,frame_hw", [(0, (0, 0), (512, 1024)), (1, (37, 11), (540, 1100))], ids=["whole-frame", "offset-region"])
def test_lane_rows_on_the_fixture_frames(lib, steer, fi, origin, frame_hw):
    """the frames of tests/golden/autosteer_net.npz: the rows the restatement takes from the fetched logits, between 1 and 63 of them, offset by the
    region's origin; the validity decision is the reference module's"""
    bgr = cc.random_bgr(*frame_hw, 20 + fi)
    x0, y0 = origin
    bgr[y0:y0 + 512, x0:x0 + 1024] = steer_frame(STEER_SEEDS[fi])
    with cc.OnCanvas(lib, bgr) as oc:
        c, f = oc.canvas, oc.frame
        steer.infer_frame(f, None if origin == (0, 0) else (x0, y0, 1024, 512))
        logits = steer.logits().copy()
        c.draw_lane_rows(steer)
        got = c.fetch("bgr8")
        pts = dc.lane_row_points(logits, origin)
        assert 1 <= len(pts) <= 63
        assert np.array_equal(logits.reshape(2, 64)[1] >= 0.5, G[f"h_{fi}"] >= 0.5)
        want = dc.draw_lane_rows(bgr, logits, origin)
        assert np.array_equal(got, want), np.argwhere(got != want)[:4]
        assert not np.array_equal(got, bgr)


def write_device(ptr, a):
    """a host array into device memory, through the HIP runtime this process already holds (the engine is idle: its last call returned synchronised)"""
    import ctypes as C

    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemcpy.restype, hip.hipMemcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0     # hipMemcpyHostToDevice
    assert hip.hipDeviceSynchronize() == 0


def test_lane_rows_that_draw_nothing(lib, steer):
    """the engine's device logits overwritten with rows of the test's choosing: xp left and right of the frame (clipped to the canvas), NaN, both
    infinities and a product beyond the pixel range (nothing), h_vector just below 0.5 and NaN (nothing), exactly 0.5 (drawn)"""
    logits = np.zeros((2, 64), np.float32)
    logits[0] = np.linspace(-0.2, 1.2, 64, dtype=np.float32)
    logits[1] = 0.75
    logits[1, 4], logits[1, 5], logits[1, 6] = 0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nan
    logits[0, 7], logits[0, 8], logits[0, 9], logits[0, 10] = np.nan, np.inf, -np.inf, 1e6
    origin = (9, 14)
    pts = dc.lane_row_points(logits, origin)
    assert len(pts) == 58 and min(p[0] for p in pts) < 0 and max(p[0] for p in pts) > 1060
    bgr = cc.random_bgr(530, 1040, 6)
    with cc.OnCanvas(lib, bgr) as oc:
        steer.infer_frame(oc.frame, origin + (1024, 512))
        write_device(steer.device_outputs()[0], logits)
        oc.canvas.draw_lane_rows(steer)
        got, want = oc.canvas.fetch("bgr8"), dc.draw_lane_rows(bgr, logits, origin)
        assert np.array_equal(got, want), np.argwhere(got != want)[:4]


# ---- 3. the whole display frame
def test_the_display_thread_on_a_1080p_frame(lib, ego):
    """begin, boxes, lanes on the (0, 420, W, H - 420) crop, fetch_resized NV12 1280 x 720 == the composed restatement"""
    from autoware_vision_pilot_amd import synthetic

    Hc, Wc = 1080, 1920
    crop = (0, 420, Wc, Hc - 420)
    bgr = synthetic.synthetic_frame(Hc, Wc, 23)
    rows = np.array([cc.det(100.4, 50.2, 400.9, 300.1, 1), cc.det(-20, 400, 300.5, 1200, 2), cc.det(900, 410, 1919.9, 1079.9, 3), cc.det(960, 500, 1100, 640, 0)], np.float32)
    with cc.OnCanvas(lib, bgr) as oc:
        c, f = oc.canvas, oc.frame
        ego.infer_frame(f, crop)
        logits = ego.logits().copy()
        t = float(np.median(logits))
        c.draw_detections(rows)
        c.overlay_lanes(ego, t)
        y, uv = c.fetch("nv12", size=(720, 1280))
        full = dc.overlay_lanes(cc.draw_boxes(bgr, rows), logits, t, crop)
        wy, wuv = cc.from_bgr("nv12", dc.resized(full, (720, 1280)))
        assert y.shape == (720, 1280) and uv.shape == (360, 1280)
        assert np.array_equal(y, wy) and np.array_equal(uv, wuv)
        assert np.array_equal(c.fetch("bgr8"), full)          # the canvas keeps the full-size picture


# ---- 4. ordering without host waits
def test_overlay_lanes_is_ordered_against_the_engine_on_the_device(lib, ego):
    """infer A; overlay; infer B; fetch -- nothing synchronised in between: the picture shows A's lanes, and the engine ends up with B's logits"""
    A, B = (cc.random_bgr(H, W, s) for s in (51, 52))
    fa, fb, c = lib.Frame(), lib.Frame(), lib.Canvas()
    try:
        fa.upload(A, "bgr8")
        fb.upload(B, "bgr8")
        logits = []
        for f in (fa, fb):       # the stand-alone passes; they also take the canvas past its first table upload
            ego.infer_frame(f, LANES)
            logits.append(ego.logits().copy())
            c.begin(f)
            c.overlay_lanes(ego, 0.0)
        c.sync()
        t = float(np.median(logits[0]))
        assert not np.array_equal(dc.planes_on(logits[0].reshape(3, 80, 160), t, LANES), dc.planes_on(logits[1].reshape(3, 80, 160), t, LANES))
        ego.upload_from_frame(fa, LANES)
        ego.enqueue()
        c.begin(fa)
        c.overlay_lanes(ego, t)
        ego.upload_from_frame(fb, LANES)
        ego.enqueue()
        got = c.fetch("bgr8")
        assert np.array_equal(got, dc.overlay_lanes(A, logits[0], t, LANES))
        ego.fetch_outputs()
        assert np.array_equal(ego.logits(), logits[1])
    finally:
        c.close()
        fa.close()
        fb.close()


def test_draw_lane_rows_is_ordered_against_the_engine_on_the_device(lib, steer):
    A, B = (steer_frame(s) for s in STEER_SEEDS[:2])
    fa, fb, c = lib.Frame(), lib.Frame(), lib.Canvas()
    try:
        fa.upload(A, "bgr8")
        fb.upload(B, "bgr8")
        logits = []
        for f in (fa, fb):
            steer.infer_frame(f)
            logits.append(steer.logits().copy())
        assert dc.lane_row_points(logits[0], (0, 0)) != dc.lane_row_points(logits[1], (0, 0))
        steer.upload_from_frame(fa)
        steer.enqueue()
        c.begin(fa)
        c.draw_lane_rows(steer)
        steer.upload_from_frame(fb)
        steer.enqueue()
        got = c.fetch("bgr8")
        assert np.array_equal(got, dc.draw_lane_rows(A, logits[0], (0, 0)))
        steer.fetch_outputs()
        assert np.array_equal(steer.logits(), logits[1])
    finally:
        c.close()
        fa.close()
        fb.close()


# ---- 5. refusals that need an engine
def test_engine_refusals(lib, ego, steer, state_dicts):
    from autoware_vision_pilot_amd import synthetic, weights as vw

    fresh_ego = lib.Engine("egolanes", vw.pack_state_dict(state_dicts("egolanes")), precision="fp16")
    fresh_steer = lib.Engine("autosteer", vw.pack_state_dict(synthetic.make_autosteer_state_dict(0)), precision="fp16")
    seg = lib.Engine("sceneseg", vw.pack_state_dict(state_dicts("sceneseg")), precision="fp16")
    bgr = steer_frame(3)
    try:
        with cc.OnCanvas(lib, bgr) as oc:
            c, f = oc.canvas, oc.frame
            with pytest.raises(lib.VpError, match="Inference has not been run yet"):       # before the first pass
                c.overlay_lanes(fresh_ego, 0.0)
            with pytest.raises(lib.VpError, match="Inference has not been run yet"):
                c.draw_lane_rows(fresh_steer)
            for eng in (steer, fresh_steer, seg):                                           # wrong kinds, in both directions
                with pytest.raises(ValueError, match="VP_EGOLANES engines only"):
                    c.overlay_lanes(eng, 0.0)
            for eng in (ego, fresh_ego, seg):
                with pytest.raises(ValueError, match="VP_AUTOSTEER engines only"):
                    c.draw_lane_rows(eng)
            with pytest.raises(ValueError, match="no mask or depth plane"):                 # and the existing calls keep refusing AutoSteer
                c.blend_mask(steer, 0)
            ego.infer_frame(f)
            steer.infer_frame(f)
            with pytest.raises(ValueError, match="threshold"):
                c.overlay_lanes(ego, float("inf"))
            c.overlay_lanes(ego, 0.0)
            c.draw_lane_rows(steer)
            want = dc.draw_lane_rows(dc.overlay_lanes(bgr, ego.logits(), 0.0, (0, 0, 1024, 512)), steer.logits(), (0, 0))
            assert np.array_equal(c.fetch("bgr8"), want)
            f.upload(cc.random_bgr(514, 1024, 6), "bgr8")                                   # another frame geometry
            c.begin(f)
            for draw in (lambda: c.overlay_lanes(ego, 0.0), lambda: c.draw_lane_rows(steer)):
                with pytest.raises(ValueError, match="1024 x 512 frame.*1024 x 514 picture"):
                    draw()
            ego.infer_tensor(np.zeros((3, 320, 640), np.float32))
            with pytest.raises(ValueError, match="tensor"):
                c.overlay_lanes(ego, 0.0)
    finally:
        for e in (fresh_ego, fresh_steer, seg):
            e.close()
