"""vp_frame on the MI355X: a camera frame uploaded once in its native format, converted to BGR8 on the device, consumed by any engine and by the detector.
Cases and the numpy oracle of the conversions: tests/frame_cases.py.  Every consumer check is bit for bit against the host path (vp_infer /
vp_detect_infer) on the numpy-converted BGR8 pixels."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frame_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib as _lib

    return _lib


@pytest.fixture(scope="module")
def seg_blob(state_dicts):
    from autoware_vision_pilot_amd import weights as vw

    return vw.pack_state_dict(state_dicts("sceneseg"))


@pytest.fixture(scope="module")
def seg(lib, seg_blob):
    """two SceneSeg fp16 engines on the same weights"""
    engs = [lib.Engine("sceneseg", seg_blob, precision="fp16") for _ in range(2)]
    yield engs
    for e in engs:
        e.close()


# ---- 1. conversions, bit for bit through vp_frame_fetch_bgr8
@pytest.mark.parametrize("fmt,h,w,strides", fc.CONVERSION_CASES, ids=[c[0] for c in fc.CONVERSION_CASES])
def test_conversion_bit_for_bit(lib, fmt, h, w, strides):
    fc.check_conversion(lib, fmt, h, w, strides)


@pytest.mark.parametrize("fmt", fc.YUV)
def test_table_frame(lib, fmt):
    fc.check_table(lib, fmt)


def test_production_sizes_and_registered_pool(lib):
    """more than one workgroup, w % 4 == 2 (the last store block of a row half empty), and the one-DMA path of a vp_register_frames pool"""
    for fmt, h, w in (("nv12", 270, 482), ("yuy2", 135, 482), ("rgba8", 67, 333)):
        fc.check_conversion(lib, fmt, h, w, (fc.PX_BYTES[fmt] * w + 9, w + 6), seed=5)
    pool = np.random.default_rng(6).integers(0, 256, size=(2, 40, 96), dtype=np.uint8)
    lib.register_frames(pool)
    f = lib.Frame()
    try:
        for fmt, planes, h, w in (("uyvy", [pool[0][:, :80]], 40, 40), ("nv12", [pool[0][:, :90], pool[1][:20, :90]], 40, 90), ("bgr8", [pool[1][:, :93]], 40, 31)):
            f.upload(planes, fmt, hw=(h, w))
            assert np.array_equal(f.fetch_bgr8(), fc.to_bgr(fmt, planes, h, w)), fmt
    finally:
        f.close()
        lib.unregister_frames(pool)


# ---- 2. a consumer equals the host path
@pytest.mark.parametrize("region", [(5, 7, 41, 29), None], ids=["odd-region", "whole"])
def test_sceneseg_consumer_equals_host(lib, seg, region):
    fc.check_consumer_equals_host(lib, seg[0], "nv12", 48, 64, region)


def test_consumer_visualisation_blends_with_the_region(lib, seg):
    """vp_visualize_mask_bgr8 blends with "the last frame": behind infer_frame that is the region, as behind vp_infer on the same pixels"""
    planes = fc.random_planes("yuy2", 40, 64, (133,), 9)
    bgr = np.ascontiguousarray(fc.to_bgr("yuy2", planes, 40, 64))
    fc.infer_view(lib, seg[0], bgr, 3, 5, 51, 31)
    want = seg[0].visualize_mask(0, (31, 51))
    f = lib.Frame()
    try:
        f.upload(planes, "yuy2", hw=(40, 64))
        seg[0].infer_frame(f, (3, 5, 51, 31))
        assert np.array_equal(seg[0].visualize_mask(0, (31, 51)), want)
    finally:
        f.close()


def test_autosteer_region_of_a_larger_frame(lib):
    from autoware_vision_pilot_amd import synthetic, weights as vw

    eng = lib.Engine("autosteer", vw.pack_state_dict(synthetic.make_autosteer_state_dict(0)), precision="fp16")
    try:
        fc.check_consumer_equals_host(lib, eng, "yuy2", 540, 1100, (37, 11, 1024, 512))
        f = lib.Frame()
        try:
            f.upload(np.zeros((540, 1100, 3), np.uint8), "bgr8")
            for region in (None, (0, 0, 1024, 510), (0, 0, 1022, 512)):
                with pytest.raises(ValueError, match="512 x 1024"):
                    eng.upload_from_frame(f, region)
        finally:
            f.close()
    finally:
        eng.close()


def test_autodrive_streaming_over_three_frames(lib):
    """three infer_frame calls == three vp_infer calls: the streaming pair (previous frame's features) is shared with the host path"""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    blob = vw.pack_state_dict(synthetic.make_autodrive_state_dict(0))
    host, dev = (lib.Engine("autodrive", blob, precision="fp16") for _ in range(2))
    f = lib.Frame()
    try:
        for i in range(3):
            planes = fc.random_planes("nv12", 48, 64, (67, 70), 20 + i)
            host.infer(fc.to_bgr("nv12", planes, 48, 64))
            f.upload(planes, "nv12", hw=(48, 64))
            dev.infer_frame(f)
            assert np.array_equal(dev.input_tensor(), host.input_tensor()), i
            assert np.array_equal(dev.logits(), host.logits()), i
    finally:
        f.close()
        host.close()
        dev.close()


# ---- 3. ordering without host waits
def test_reupload_orders_itself_behind_consumers_on_the_device(lib, seg):
    """upload(A), consume(e1), enqueue(e1), upload(B), consume(e2), enqueue(e2) -- and only then the first synchronisation: e1 saw A, e2 saw B.  Then both
    engines consume one uploaded frame from two threads."""
    e1, e2 = seg
    h, w = 720, 1280
    A, B = (fc.random_planes("yuy2", h, w, (2 * w + 64,), s) for s in (31, 32))
    want = []
    for e, p in ((e1, A), (e2, B)):      # the stand-alone passes; they also take both engines past their eager first pass, so nothing below waits
        e.infer(fc.to_bgr("yuy2", p, h, w))
        want.append(e.logits().copy())
    assert not np.array_equal(want[0], want[1])
    f = lib.Frame()
    try:
        for _ in range(2):               # the first round captures the graphs for the new stride, the second replays them: no host wait left
            f.upload(A, "yuy2", hw=(h, w))
            e1.upload_from_frame(f)
            e1.enqueue()
            f.upload(B, "yuy2", hw=(h, w))
            e2.upload_from_frame(f)
            e2.enqueue()
            e1.fetch_outputs()
            e2.fetch_outputs()
            assert np.array_equal(e1.logits(), want[0])
            assert np.array_equal(e2.logits(), want[1])
        got, errs = [None, None], []

        def run(i, e):
            try:
                e.infer_frame(f)
                got[i] = e.logits().copy()
            except Exception as ex:  # noqa: BLE001 -- reported below, on the main thread
                errs.append(ex)

        threads = [threading.Thread(target=run, args=(i, e)) for i, e in enumerate((e1, e2))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errs, errs
        assert np.array_equal(got[0], want[1]) and np.array_equal(got[1], want[1])     # the frame holds B
    finally:
        f.close()


# ---- 4. detector
def test_detector_on_a_yuy2_frame(lib):
    from autoware_vision_pilot_amd import synthetic, weights as vw

    g = np.load(os.path.join(HERE, "golden", "autospeed_net.npz"))
    conf, iou = float(g["conf"]), float(g["iou"])
    h, w = 360, 640
    bgr0 = synthetic.synthetic_frame(h, w, 21).astype(np.int64)
    # a YUY2 frame with the synthetic frame's content (forward BT.601, rounded; chroma of the even pixel): what a camera would have delivered
    b, gr, r = bgr0[:, :, 0], bgr0[:, :, 1], bgr0[:, :, 2]
    Y = np.clip((66 * r + 129 * gr + 25 * b + 128) // 256 + 16, 0, 255)
    U = np.clip((-38 * r - 74 * gr + 112 * b + 128) // 256 + 128, 0, 255)
    V = np.clip((112 * r - 94 * gr - 18 * b + 128) // 256 + 128, 0, 255)
    q = np.stack([Y[:, 0::2], U[:, 0::2], Y[:, 1::2], V[:, 0::2]], axis=2).astype(np.uint8)
    planes = [np.ascontiguousarray(q.reshape(h, 2 * w))]
    bgr = fc.to_bgr("yuy2", planes, h, w)
    eng = lib.Engine("autospeed", vw.pack_state_dict(synthetic.make_autospeed_state_dict(int(g["weight_seed"]))), precision="fp16")
    det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
    f = lib.Frame()
    try:
        det.attach(eng)
        f.upload(planes, "yuy2")
        for region in (None, (33, 17, 401, 299)):
            x0, y0, rw, rh = region or (0, 0, w, h)
            want_rows, want_n = det.infer(bgr[y0:y0 + rh, x0:x0 + rw], conf, iou)
            want_raw = eng.logits().copy()
            rows, n = det.infer_frame(f, conf, iou, region)
            print(f"region {region}: {n} detections")
            assert want_n > 0                                               # the comparison has something to compare
            assert n == want_n and np.array_equal(rows, want_rows)          # field for field
            assert np.array_equal(eng.logits(), want_raw)                   # and the network saw the same letterboxed tensor
        with pytest.raises(lib.VpError, match="frame region"):
            det.infer_frame(f, conf, iou, (0, 0, w + 1, h))
        empty = lib.Frame()
        try:
            with pytest.raises(lib.VpError, match="never uploaded"):
                det.infer_frame(empty, conf, iou)
        finally:
            empty.close()
    finally:
        f.close()
        det.close()
        eng.close()


# ---- 5. device upload
@pytest.mark.parametrize("fmt,h,w,strides", [("nv12", 30, 46, (50, 48)), ("uyvy", 21, 38, (81,)), ("bgr8", 9, 13, (40,))], ids=["nv12", "uyvy", "bgr8"])
def test_device_upload_from_a_torch_stream(lib, fmt, h, w, strides):
    """planes produced by torch on a side stream, handed over with that stream's handle: the bits of the host upload"""
    planes = fc.random_planes(fmt, h, w, strides, 40)
    parents = [p.base if p.base is not None else p for p in planes]
    side = torch.cuda.Stream()
    f = lib.Frame()
    try:
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
    assert np.array_equal(got, fc.to_bgr(fmt, planes, h, w))


# ---- 6. refusals
def test_upload_refusals(lib):
    fc.check_upload_refusals(lib)


def test_consumer_refusals(lib, seg, seg_blob):
    from autoware_vision_pilot_amd import synthetic, weights as vw

    e = seg[0]
    f = lib.Frame()
    made = []
    try:
        with pytest.raises(lib.VpError, match="never uploaded") as ei:          # VP_ERR_STATE before the first upload
            e.upload_from_frame(f)
        assert "error -4" in str(ei.value)
        with pytest.raises(lib.VpError, match="never uploaded"):
            e.infer_frame(f)
        f.upload(np.zeros((8, 12, 3), np.uint8), "bgr8")
        for region in ((0, 0, 13, 8), (11, 0, 2, 2), (0, 7, 2, 2), (-1, 0, 4, 4), (0, 0, 1, 8), (0, 0, 12, 0), (1, 0, 0, 0)):
            with pytest.raises(ValueError, match="frame region"):
                e.upload_from_frame(f, region)
        head = lib.Engine("sceneseg", seg_blob, precision="fp16", base=e)
        made.append(head)
        with pytest.raises(ValueError, match="frames go to the base"):
            head.upload_from_frame(f)
        enc = lib.Engine("sceneseg", seg_blob, precision="fp16", frames=2)
        made.append(enc)
        with pytest.raises(ValueError, match="batched encoder"):
            enc.upload_from_frame(f)
        speed = lib.Engine("autospeed", vw.pack_state_dict(synthetic.make_autospeed_state_dict(1)), precision="fp16")
        made.append(speed)
        for call in (speed.upload_from_frame, speed.infer_frame):
            with pytest.raises(lib.VpError, match="vp_detect_infer") as ei:      # the refusal vp_upload_frame gives today
                call(f)
            with pytest.raises(lib.VpError) as host:
                speed.upload_frame(np.zeros((8, 12, 3), np.uint8))
            assert str(ei.value) == str(host.value)
        rgb = lib.Engine("sceneseg", seg_blob, precision="fp16")
        made.append(rgb)
        rgb.set_input_format(lib.VP_RGB8, lib.VP_PLANES_RGB)
        with pytest.raises(ValueError, match="VP_BGR8"):
            rgb.upload_from_frame(f)
        rgb.set_input_format(lib.VP_BGR8, lib.VP_PLANES_RGB)                     # the plane order is the engine's own business
        rgb.upload_from_frame(f)
        rgb.sync()
        if lib.load().vp_device_count() >= 2:
            far = lib.Frame(gpu_id=1)
            try:
                far.upload(np.zeros((8, 12, 3), np.uint8), "bgr8")
                with pytest.raises(ValueError, match="lives on GPU 1"):
                    e.upload_from_frame(far)
            finally:
                far.close()
        else:                                                                    # one GPU visible: no frame can live elsewhere
            with pytest.raises(ValueError, match="gpu_id out of range"):
                lib.Frame(gpu_id=1)
    finally:
        for m in made:
            m.close()
        f.close()
