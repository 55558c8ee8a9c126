"""The Python AutoSpeed wrapper's twin on the MI355X: vp_detect_preprocess_pil (Pillow letterbox), vp_detect_postprocess_agnostic (class-agnostic decode
+ NMS), vp_detect_infer_pil and infer.AutoSpeedNetworkInfer.  References: tests/autospeed_py_ref.py (Pillow itself + the torch / numpy restatement of
Models/inference/auto_speed_infer.py) and tests/golden/autospeed_py.npz, the rows of the reference class's own method bodies on the synthetic
checkpoint.  Note on the letterbox frames: 90 x 100 pads left and right like 37 x 53 (no h x w or w x h reading of it pads top and bottom in a
64 x 128 input), so 40 x 100 stands beside it for the other direction."""
import os
import sys

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import autospeed_py_cases as cases  # noqa: E402
import autospeed_py_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
G = np.load(cases.GOLDEN)
CONF, IOU = float(G["conf"]), float(G["iou"])


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (first: one shared HIP runtime)

    from autoware_vision_pilot_amd import lib as vplib

    return vplib


@pytest.fixture(scope="module")
def det(lib):
    d = lib.Detector(cases.NET_H, cases.NET_W, max_boxes=128, max_attrs=8)
    yield d
    d.close()


@pytest.fixture(scope="module")
def big_det(lib):
    d = lib.Detector(cases.NET_H, cases.NET_W, max_boxes=cases.LARGE_BOXES, max_attrs=8)
    yield d
    d.close()


@pytest.fixture(scope="module")
def blob():
    from autoware_vision_pilot_amd import synthetic, weights as vw

    return vw.pack_state_dict(synthetic.make_autospeed_state_dict(int(G["weight_seed"])))


def _image(fi):
    from autoware_vision_pilot_amd import synthetic

    h, w, seed = (int(v) for v in G["frames"][fi])
    return Image.fromarray(np.ascontiguousarray(synthetic.synthetic_frame(h, w, seed)[:, :, ::-1]))


def _twin(blob, precision, act_scale=False):
    from autoware_vision_pilot_amd import infer

    t = infer.AutoSpeedNetworkInfer(blob, precision=precision, act_scale=act_scale)
    t.conf_thres, t.iou_thres = CONF, IOU                     # the fixture's thresholds (the defaults miss its margins on the synthetic checkpoint)
    return t


@pytest.fixture(scope="module")
def x3(blob):
    t = _twin(blob, "fp16x3")
    yield t
    t._detector.close()
    t.model.close()


# ---------------------------------------------------------------------------------------------------------------- letterbox
@pytest.mark.parametrize("shape", cases.LETTERBOX_FRAMES)
def test_pillow_letterbox_bit_exact(lib, det, shape):
    f = cases.frame(shape[0], shape[1], 7 * shape[0] + shape[1])
    cases.check_letterbox(det, lib.VP_RGB8, lib.VP_BGR8, f)


def test_pillow_letterbox_bit_exact_720p_into_the_network_size(lib):
    d = lib.Detector(512, 1024, max_boxes=128, max_attrs=8)
    try:
        _, (pad_x, pad_y) = cases.check_letterbox(d, lib.VP_RGB8, lib.VP_BGR8, cases.frame(720, 1280, 9))
        assert (pad_x, pad_y) == (57, 0)
    finally:
        d.close()


def test_to_tensor_table(det):
    """np.float32(v) / np.float32(255) for all 256 byte values, on a frame that is not resized"""
    got, _ = det.preprocess_pil(cases.frame(cases.NET_H, cases.NET_W, 1))
    want = np.arange(256, dtype=np.float32) / np.float32(255)
    for c in range(3):
        assert np.array_equal(got[c].ravel()[:256].view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("case", cases.decode_cases(), ids=lambda c: c[0])
def test_agnostic_decode_hand_built(det, case):
    name, raw, conf, iou, geom, ow, oh, cap, kept = case
    got, n, err = cases.check_decode(det, raw, conf, iou, geom, ow, oh, cap=cap)
    print(f"{name}: {n} kept, floats against the restatement {err:.2e}")
    assert n == len(kept)


def test_agnostic_decode_fixture_columns(det):
    for raw, conf, iou, geom, ow, oh, want in cases.fixture_cases():
        _, n, err = cases.check_decode(det, raw, conf, iou, geom, ow, oh, want=want)
        print(f"fixture columns: {n} kept, floats against the reference wrapper's rows {err:.2e}")


def test_agnostic_decode_more_than_1024_candidates(big_det):
    """2100 boxes, every one a candidate: the sort runs on 4096 keys (four per thread), the compaction on three rows per thread"""
    raw, conf, iou, geom, ow, oh = cases.large_case()
    score_gap, iou_gap, n_cand = ref.candidate_iou_gap(raw, conf, iou)
    print(f"{n_cand} candidates of {raw.shape[1]} boxes, IoU gap {iou_gap:.3f}, score gap {score_gap:.3f}")
    assert n_cand == raw.shape[1] == 2100 and iou_gap >= 0.05 and score_gap >= 0.1
    _, n, err = cases.check_decode(big_det, raw, conf, iou, geom, ow, oh)
    print(f"{n} kept, floats against the restatement {err:.2e}")
    assert n == 1890
    cases.check_decode(big_det, raw, conf, iou, geom, ow, oh, cap=5)


@pytest.mark.parametrize("key", sorted(cases.pin_cases()))
def test_agnostic_decode_keeps_the_two_kernel_library_s_bits(big_det, key):
    """tests/golden/detect_agnostic_parent.npz: counts, row order, corners and class of the library before the two kernels became one, bit for bit"""
    cases.check_parent_pin(big_det, key)


# --------------------------------------------------------------------------------------------------------------- whole path
def _check_rows(rows, fi, what):
    want = G[f"rows_{fi}"]
    got = np.array(rows, np.float32).reshape(-1, 6)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got[:, 5], want[:, 5])
    err = cases.rel(got[:, :5], want[:, :5])
    print(f"{what}, frame {fi}: {len(got)} rows, coordinates / score against the reference wrapper's {err:.2e}")
    assert err <= 1e-3


def test_twin_against_the_reference_wrapper(x3):
    for fi in range(2):
        image = _image(fi)
        rows = x3.inference(image)
        assert isinstance(rows, list) and all(isinstance(r, list) and len(r) == 6 for r in rows)
        _check_rows(rows, fi, "fp16x3")
        assert x3.resize_letterbox(image) == tuple(G[f"geom_{fi}"][:1]) + (int(G[f"geom_{fi}"][1]), int(G[f"geom_{fi}"][2]))
        got = x3.model.logits().reshape(8, -1)[:, ::int(G["box_step"])]
        assert cases.rel(got, G[f"raw_{fi}"]) <= 1e-3                 # the network saw the Pillow letterbox
    x3.conf_thres = 0.9
    try:
        assert x3.inference(_image(0)) == []
    finally:
        x3.conf_thres = CONF


def test_twin_with_activation_scale(blob):
    t = _twin(blob, "fp16x3", act_scale=True)
    try:
        for fi in range(2):                                        # the first image calibrates
            _check_rows(t.inference(_image(fi)), fi, "fp16x3 + act_scale")
    finally:
        t._detector.close()
        t.model.close()


def test_twin_fp16_keeps_the_same_set(blob):
    """VP_FP16 (non-parity): the same number of rows, and every reference row has exactly one partner of its class.  Bounds from the fp16 raw bar of
    tests/test_gpu_autospeed_net.py, not from measurement: a raw box row is within 3e-2 * 1024 letterbox pixels, a corner is cx -+ w / 2 (1.5 of that)
    divided by the letterbox scale; a score is within 3e-2 (the second sigmoid only shrinks an error)."""
    t = _twin(blob, "fp16")
    try:
        for fi in range(2):
            want = G[f"rows_{fi}"]
            got = np.array(t.inference(_image(fi)), np.float32).reshape(-1, 6)
            assert got.shape == want.shape
            tol_xy = 1.5 * 3e-2 * 1024.0 / float(G[f"geom_{fi}"][0])
            match = []
            for r in want:
                d = np.abs(got[:, :4] - r[:4]).max(axis=1) + np.where(got[:, 5] == r[5], 0.0, np.inf)
                j = int(np.argmin(d))
                assert d[j] <= tol_xy and abs(got[j, 4] - r[4]) <= 3e-2
                match.append(j)
            assert sorted(match) == list(range(len(got)))
            print(f"fp16 (non-parity), frame {fi}: the same {len(got)} rows; largest corner distance {max(float(np.abs(got[j, :4] - r[:4]).max()) for j, r in zip(match, want)):.3f} px")
    finally:
        t._detector.close()
        t.model.close()


def test_constructor_errors():
    from autoware_vision_pilot_amd import infer

    with pytest.raises(ValueError):
        infer.AutoSpeedNetworkInfer("")
    with pytest.raises(ValueError):
        infer.AutoSpeedNetworkInfer(None)


# ----------------------------------------------------------------------------------------------------------- unchanged paths
def test_detect_infer_keeps_its_bits_around_infer_pil(x3):
    """vp_detect_infer on one frame before and after a vp_detect_infer_pil call on the same handle (they share its buffers and stored geometry)"""
    d = x3._detector
    bgr = np.ascontiguousarray(np.asarray(_image(0))[:, :, ::-1])
    a, na = d.infer(bgr, 0.4, 0.65)
    raw_a, ga = x3.model.logits().copy(), d.letterbox()
    rows, n = d.infer_pil(np.asarray(_image(1)), CONF, IOU)
    assert n == len(G["rows_1"])
    b, nb = d.infer(bgr, 0.4, 0.65)
    assert na == nb and na > 0 and ga == d.letterbox()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(raw_a.view(np.uint32), x3.model.logits().view(np.uint32))
