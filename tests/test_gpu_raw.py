"""Raw Bayer, P010 and GRAY16 uploads of vp_frame on the MI355X: frame_raw_to_bgr8_kernel and frame_deep_to_bgr8_kernel bit for bit against the numpy
restatement of the definition (tests/raw_cases.py), the device and registered-pool upload paths, rectification behind a raw upload, the re-upload
ordering and one detector pass."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import raw_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib as _lib

    return _lib


@pytest.fixture(scope="module")
def seg(lib, state_dicts):
    """two SceneSeg fp16 engines on the same weights"""
    from autoware_vision_pilot_amd import weights as vw

    blob = vw.pack_state_dict(state_dicts("sceneseg"))
    engs = [lib.Engine("sceneseg", blob, precision="fp16") for _ in range(2)]
    yield engs
    for e in engs:
        e.close()


# ---- 1. conversions, bit for bit through vp_frame_fetch_bgr8
@pytest.mark.parametrize("name,order,container,kw,hw", rc.CONVERSION_CASES, ids=[c[0] for c in rc.CONVERSION_CASES])
def test_conversion_bit_for_bit(lib, name, order, container, kw, hw):
    rc.check_conversion(lib, order, container, kw, hw)


@pytest.mark.parametrize("order,container,B,shift", rc.TABLE_CASES, ids=[f"{c[0]}{c[1]}-b{c[2]}" for c in rc.TABLE_CASES])
def test_value_table(lib, order, container, B, shift):
    rc.check_table(lib, order, container, B, shift)


@pytest.mark.parametrize("fmt,h,w,extras", rc.DEEP_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in rc.DEEP_CASES])
def test_p010_and_gray16_equal_the_narrowed_uploads(lib, fmt, h, w, extras):
    rc.check_deep(lib, fmt, h, w, extras)


def test_row_ends_inside_a_store_block(lib):
    rc.check_row_ends_inside_a_store_block(lib)


def read_device(ptr, n):
    """n bytes of device memory, through the HIP runtime this process already holds (the canvas is idle: vp_canvas_sync returned)"""
    import ctypes as C

    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemcpy.restype, hip.hipMemcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(n, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), n, 2) == 0          # hipMemcpyDeviceToHost
    return out.tobytes()


def test_zeros_behind_a_row_end(lib):
    rc.check_zeros_behind_a_row_end(lib, read_device)


def test_setting_applies_to_later_uploads(lib):
    rc.check_setting_applies_to_later_uploads(lib)


def test_refusals(lib):
    rc.check_refusals(lib)


def test_canvas_refuses_the_new_codes(lib):
    rc.check_canvas_refuses(lib)


# ---- 2. the other upload paths
DEVICE_CASES = (("bayer_gbrg8", 34, 66), ("bayer_grbg16", 34, 66), ("p010", 34, 66), ("gray16", 33, 67))


def _planes(fmt, h, w, seed):
    if fmt.startswith("bayer"):
        return [rc.random_raw(h, w, int(fmt[10:]), seed, bits=12 if fmt.endswith("16") else 0)]
    return rc.deep_planes(fmt, h, w, (3, 5), seed)


@pytest.mark.parametrize("fmt,h,w", DEVICE_CASES, ids=[c[0] for c in DEVICE_CASES])
def test_device_upload_equals_host_upload(lib, fmt, h, w):
    """the strided parents copied to the device as they are, handed over as device planes: the bits of the host upload"""
    planes = _planes(fmt, h, w, 40)
    kw = {"bits": 12, "black": 64, "gains": rc.GAINS, "lut": rc.gamma_lut(12)} if fmt.endswith("16") and fmt.startswith("bayer") else {}
    host = rc.upload_fetch(lib, fmt, planes, kw)
    dev = [torch.from_numpy(np.ascontiguousarray(p.base).view(np.uint8)).cuda() for p in planes]
    torch.cuda.synchronize()
    f = lib.Frame()
    try:
        f.set_raw(**kw)
        f.upload_device([t.data_ptr() for t in dev], [t.stride(0) for t in dev], fmt, h, w)
        got = f.fetch_bgr8()
    finally:
        f.close()
    assert np.array_equal(got, host)
    if fmt.startswith("bayer"):
        assert np.array_equal(got, rc.raw_to_bgr(fmt[6:10], planes[0], int(fmt[10:]), **kw))


def test_registered_pool_upload_equals_staged_upload(lib):
    """planes inside a vp_register_frames range go by one DMA per plane straight from the caller's memory"""
    pool = np.random.default_rng(6).integers(0, 256, size=(2, 40, 96), dtype=np.uint8)
    words = pool.view(np.uint16)                                       # [2][40][48]
    words &= 0x0FFF
    cases = (("bayer_bggr8", [pool[0][:, :90]], 40, 90), ("bayer_rggb16", [words[0][:, :46]], 40, 46), ("p010", [words[0][:, :42], words[1][:20, :42]], 40, 42),
             ("gray16", [words[1][:, :45]], 40, 45))
    staged = [rc.upload_fetch(lib, fmt, [p.copy() for p in planes], {"bits": 12} if fmt == "bayer_rggb16" else {}) for fmt, planes, _, _ in cases]
    lib.register_frames(pool)
    f = lib.Frame()
    try:
        for (fmt, planes, h, w), want in zip(cases, staged):
            f.set_raw(**({"bits": 12} if fmt == "bayer_rggb16" else {}))
            f.upload(planes, fmt)
            assert f.hw() == (h, w)
            assert np.array_equal(f.fetch_bgr8(), want), fmt
    finally:
        f.close()
        lib.unregister_frames(pool)
    assert np.array_equal(staged[1], rc.raw_to_bgr("rggb", words[0][:, :46], 16, bits=12))


# ---- 3. rectification behind a raw upload
def test_rectification_composes(lib):
    rc.check_rectification_composes(lib)


# ---- 4. consumers
def test_sceneseg_consumer_equals_host(lib, seg):
    rc.check_consumer_equals_host(lib, seg[0])


def test_reupload_orders_itself_behind_consumers_on_the_device(lib, seg):
    """upload(A), consume(e1), enqueue(e1), upload(B), consume(e2), enqueue(e2) -- and only then the first synchronisation: e1 saw A, e2 saw B"""
    e1, e2 = seg
    h, w = 360, 640
    kw = {"bits": 12, "black": 64, "gains": rc.GAINS}
    A, B = (rc.random_raw(h, w, 16, s, bits=12, extra=32) for s in (31, 32))
    want = []
    for e, p in ((e1, A), (e2, B)):      # the stand-alone passes; they also take both engines past their eager first pass, so nothing below waits
        e.infer(rc.raw_to_bgr("rggb", p, 16, **kw))
        want.append(e.logits().copy())
    assert not np.array_equal(want[0], want[1])
    f = lib.Frame()
    try:
        f.set_raw(**kw)
        for _ in range(2):               # the first round captures the graphs for the new stride, the second replays them: no host wait left
            f.upload(A, "bayer_rggb16")
            e1.upload_from_frame(f)
            e1.enqueue()
            f.upload(B, "bayer_rggb16")
            e2.upload_from_frame(f)
            e2.enqueue()
            e1.fetch_outputs()
            e2.fetch_outputs()
            assert np.array_equal(e1.logits(), want[0])
            assert np.array_equal(e2.logits(), want[1])
    finally:
        f.close()


def test_detector_on_a_raw_frame(lib):
    """vp_detect_infer_frame on a BAYER_RGGB8 upload of a mosaicked synthetic frame == the same pass on the BGR8 upload of the oracle's picture"""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    g = np.load(os.path.join(HERE, "golden", "autospeed_net.npz"))
    conf, iou = float(g["conf"]), float(g["iou"])
    h, w = 360, 640
    raw = np.ascontiguousarray(rc.mosaic("rggb", synthetic.synthetic_frame(h, w, 21)[:, :, ::-1]))       # the frame is BGR
    kw = {"gains": (300, 256, 280)}
    bgr = rc.raw_to_bgr("rggb", raw, 8, **kw)
    eng = lib.Engine("autospeed", vw.pack_state_dict(synthetic.make_autospeed_state_dict(int(g["weight_seed"]))), precision="fp16")
    det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
    f, ref = lib.Frame(), lib.Frame()
    try:
        det.attach(eng)
        f.set_raw(**kw)
        f.upload(raw, "bayer_rggb8")
        ref.upload(bgr, "bgr8")
        for region in (None, (33, 17, 401, 299)):
            want_rows, want_n = det.infer_frame(ref, conf, iou, region)
            want_raw = eng.logits().copy()
            rows, n = det.infer_frame(f, conf, iou, region)
            print(f"region {region}: {n} detections")
            assert want_n > 0                                               # the comparison has something to compare
            assert n == want_n and np.array_equal(rows, want_rows)          # field for field
            assert np.array_equal(eng.logits(), want_raw)                   # and the network saw the same letterboxed tensor
    finally:
        f.close()
        ref.close()
        det.close()
        eng.close()
