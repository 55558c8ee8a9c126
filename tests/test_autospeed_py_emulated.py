"""The two kernels of the Python AutoSpeed wrapper's stages (kernels_detect.hip letterbox_paste_kernel, detect_nms_kernel<true>) and their C ABI
(vp_detect_preprocess_pil, vp_detect_postprocess_agnostic; csrc/vp_detect.cpp) executed through the HIP-on-CPU emulation against
tests/autospeed_py_ref.py, at the shapes of tests/test_gpu_autospeed_py.py."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import autospeed_py_cases as cases  # noqa: E402
import autospeed_py_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def emu_lib():
    import build as emul_build

    from autoware_vision_pilot_amd import lib

    if not os.path.exists(emul_build.CLANG):
        pytest.skip("host clang++ of the ROCm toolchain not found")
    so = ct.CDLL(emul_build.build(), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    for name, (res, args) in lib._SIGS.items():
        fn = getattr(so, name)
        fn.restype, fn.argtypes = res, args
    saved = lib._lib
    lib._lib = so
    yield lib
    lib._lib = saved


@pytest.fixture(scope="module")
def det(emu_lib):
    d = emu_lib.Detector(cases.NET_H, cases.NET_W, max_boxes=128, max_attrs=8)
    yield d
    d.close()


@pytest.fixture(scope="module")
def big_det(emu_lib):
    d = emu_lib.Detector(cases.NET_H, cases.NET_W, max_boxes=cases.LARGE_BOXES, max_attrs=8)
    yield d
    d.close()


@pytest.mark.parametrize("shape", cases.LETTERBOX_FRAMES)
def test_pillow_letterbox_bit_exact(emu_lib, det, shape):
    f = cases.frame(shape[0], shape[1], 7 * shape[0] + shape[1])
    want, (pad_x, pad_y) = cases.check_letterbox(det, emu_lib.VP_RGB8, emu_lib.VP_BGR8, f)
    grey = np.float32(114) / np.float32(255)
    assert np.all(want[:, :pad_y] == grey) and np.all(want[:, :, :pad_x] == grey)
    view = np.ascontiguousarray(np.pad(f, ((0, 0), (0, 5), (0, 0))))[:, :shape[1]]      # a strided view: rows longer than 3 w
    got, _ = det.preprocess_pil(view)
    assert np.array_equal(got, want)


def test_to_tensor_table_on_the_kernels(emu_lib, det):
    """a frame that is not resized carries every byte value: the stored value is np.float32(v) / np.float32(255) for all 256 of them"""
    f = cases.frame(cases.NET_H, cases.NET_W, 1)
    got, _ = det.preprocess_pil(f)
    want = np.arange(256, dtype=np.float32) / np.float32(255)
    for c in range(3):
        assert np.array_equal(got[c].ravel()[:256].view(np.uint32), want.view(np.uint32))


def test_letterbox_refusals(emu_lib, det):
    with pytest.raises(emu_lib.VpError, match="collapses"):
        det.preprocess_pil(np.zeros((600, 1, 3), np.uint8))        # int(1 * 64 / 600) = 0 columns: Pillow refuses it too
    with pytest.raises(emu_lib.VpError, match="pixel_format"):
        det.preprocess_pil(np.zeros((8, 8, 3), np.uint8), 2)
    fresh = emu_lib.Detector(cases.NET_H, cases.NET_W, max_boxes=128, max_attrs=8)
    try:
        with pytest.raises(emu_lib.VpError, match="no letterbox geometry"):
            fresh.postprocess_agnostic(np.zeros((5, 8), np.float32), 0.6, 0.45)
    finally:
        fresh.close()
    with pytest.raises(emu_lib.VpError, match="vp_detect_postprocess_agnostic"):
        det.postprocess_agnostic(np.zeros((4, 10), np.float32), 0.6, 0.45)      # no class rows


@pytest.mark.parametrize("case", cases.decode_cases(), ids=lambda c: c[0])
def test_agnostic_decode_hand_built(det, case):
    name, raw, conf, iou, geom, ow, oh, cap, kept = case
    got, n, _ = cases.check_decode(det, raw, conf, iou, geom, ow, oh, cap=cap)
    assert n == len(kept)


def test_agnostic_decode_fixture_columns(det):
    for raw, conf, iou, geom, ow, oh, want in cases.fixture_cases():
        cases.check_decode(det, raw, conf, iou, geom, ow, oh, want=want)


def test_agnostic_decode_more_than_1024_candidates(big_det):
    """2100 boxes, every one a candidate: the sort runs on 4096 keys (four per thread), the compaction on three rows per thread"""
    raw, conf, iou, geom, ow, oh = cases.large_case()
    score_gap, iou_gap, n_cand = ref.candidate_iou_gap(raw, conf, iou)
    assert n_cand == raw.shape[1] == 2100 and iou_gap >= 0.05 and score_gap >= 0.1
    _, n, _ = cases.check_decode(big_det, raw, conf, iou, geom, ow, oh)
    assert n == 1890
    cases.check_decode(big_det, raw, conf, iou, geom, ow, oh, cap=5)


@pytest.mark.parametrize("key", sorted(cases.pin_cases()))
def test_agnostic_decode_keeps_the_two_kernel_library_s_bits(big_det, key):
    cases.check_parent_pin(big_det, key)


def test_existing_stages_keep_their_bits_around_the_new_ones(emu_lib, det):
    """vp_detect_preprocess / _postprocess before and after the Pillow path on the same handle: identical bits (they share the stored geometry)"""
    f = cases.frame(37, 53, 5)
    a, ga = det.preprocess(f)
    raw = cases.decode_cases()[1][1]
    da, na = det.postprocess(raw, 0.25, 0.45)
    det.preprocess_pil(f)
    det.postprocess_agnostic(raw, 0.6, 0.45)
    b, gb = det.preprocess(f)
    db, nb = det.postprocess(raw, 0.25, 0.45)
    assert ga == gb and np.array_equal(a.view(np.uint32), b.view(np.uint32)) and na == nb and np.array_equal(da.view(np.uint32), db.view(np.uint32))


def test_twin_end_to_end_on_cpu(emu_lib):
    """infer.AutoSpeedNetworkInfer built and run as a user does (constructor first, no inference before it), parity mode, one fixture frame: the
    reference wrapper's rows -- count, order and class equal, floats within 1e-3 * max(1, |ref|); and [] when nothing is kept."""
    from PIL import Image

    from autoware_vision_pilot_amd import infer, synthetic, weights as vw

    g = np.load(cases.GOLDEN)
    h, w, seed = (int(v) for v in g["frames"][1])
    image = Image.fromarray(np.ascontiguousarray(synthetic.synthetic_frame(h, w, seed)[:, :, ::-1]))
    twin = infer.AutoSpeedNetworkInfer(vw.pack_state_dict(synthetic.make_autospeed_state_dict(int(g["weight_seed"]))), precision="fp16x3")
    try:
        assert twin.model.output_dims() == (1, 8, 1, 10752)
        assert (twin.conf_thres, twin.iou_thres, twin.train_size) == (0.6, 0.45, (1024, 512))
        twin.conf_thres, twin.iou_thres = float(g["conf"]), float(g["iou"])
        rows = twin.inference(image)
        want = g["rows_1"]
        got = np.array(rows, np.float32).reshape(-1, 6)
        assert isinstance(rows, list) and got.shape == want.shape and np.array_equal(got[:, 5], want[:, 5])
        assert cases.rel(got[:, :5], want[:, :5]) <= 1e-3
        assert twin.resize_letterbox(image) == (float(g["geom_1"][0]), int(g["geom_1"][1]), int(g["geom_1"][2]))
        twin.conf_thres = 0.9
        assert twin.inference(image) == []
    finally:
        twin._detector.close()
        twin.model.close()
    with pytest.raises(ValueError):
        infer.AutoSpeedNetworkInfer("")
