"""vp_metric's label part without a GPU: the ABI, the numpy reference of tests/label_cases.py against the results pinned from the reference project's loaders
(tests/golden/label_cases.npz, tools/pin_label.py), the crop against PIL.Image.crop, the dataset boxes and the class weights."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import abi  # noqa: E402
import label_cases as lc  # noqa: E402

SEG_PINS = ("comma", "bdd", "iddaw", "mapillary")
DEPTH_PINS = ("random", "negative_and_zero", "constant", "one_nan", "one_inf")


@pytest.fixture(scope="module")
def golden():
    return np.load(lc.GOLDEN)


def test_new_symbols_are_declared_exported_and_bound_and_the_record_matches():
    from autoware_vision_pilot_amd import lib

    src = abi.header_source()
    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in lc.SYMBOLS:
        assert s in declared and s in exported and s in lib.EXPORTED_SYMBOLS, s
    assert all(s.startswith("vp_") for s in exported)
    assert "enum vp_label_dtype { VP_LABEL_F32 = 0, VP_LABEL_F64 = 1 };" in src and (lib.VP_LABEL_F32, lib.VP_LABEL_F64) == (0, 1)
    assert "uint32_t n, freq[3], unmatched, outside, nonfinite;" in src and "double min, max;" in src
    D = lib.LABEL_FRAME_DTYPE
    assert D.itemsize == 48
    for name, off in (("kind", 0), ("n", 4), ("freq", 8), ("unmatched", 20), ("outside", 24), ("nonfinite", 28), ("min", 32), ("max", 40)):
        assert D.fields[name][1] == off, name
    # the table ships in the header and in the binding, and is the cases' own
    rows = ", ".join("{%d, %d, %d, %d}" % tuple(r) for r in lc.COLOURS)
    assert rows in " ".join(src.replace("\\", " ").split())
    assert np.array_equal(lib.SCENESEG_COLOURS, lc.COLOURS) and lib.SCENESEG_COLOURS.dtype == np.uint8
    # the older records are as they were
    assert ct.sizeof(lib.MetricFrame) == 72 and ct.sizeof(lib.MetricSummary) == 80 and ct.sizeof(lib.MetricLanesFrame) == 96


def test_nearest_table_is_the_projects():
    from oracle import pre_post

    for src, dst in ((37, 16), (53, 24), (5, 16), (7, 24), (990, 320), (1919, 640), (1024, 320), (2047, 640), (320, 320), (1, 9)):
        t = lc.nearest_index(src, dst)
        assert np.array_equal(t, pre_post.nearest_index(src, dst)) and t.max() <= src - 1 and t.min() == 0


@pytest.mark.parametrize("name", SEG_PINS)
def test_colour_reference_equals_the_pinned_loader(golden, name):
    """extractROI + createGroundTruth: planes, frequencies and class weights, 0 differences"""
    from autoware_vision_pilot_amd import lib

    label, dataset, planes = golden["seg_%s_label" % name], str(golden["seg_%s_dataset" % name]), golden["seg_%s_planes" % name]
    box = lib.sceneseg_roi(dataset, label.shape[1], label.shape[0])
    ch, cw = planes.shape[1:]
    cls, rec = lc.seg_ref(label, (ch, cw), box)          # the identity tables: the full-resolution crop
    assert np.array_equal(lc.nearest_index(ch, ch), np.arange(ch))
    for c in range(3):
        assert np.array_equal(np.where(cls == c, 255, 0).astype(np.uint8), planes[c]), (name, c)
    assert rec["freq"] == tuple(int(f) for f in golden["seg_%s_freq" % name]) and rec["n"] == ch * cw
    assert rec["unmatched"] == int((planes.sum(axis=0) == 0).sum()) and rec["unmatched"] > 0
    assert rec["outside"] == {"comma": 0, "bdd": 1000 * 500 - 24 * 36, "iddaw": 2047 * 1024 - 24 * 30, "mapillary": 0}[name]
    got = lib.class_weights({"n": rec["n"], "freq": rec["freq"]})
    assert np.array(got, np.float64).tobytes() == golden["seg_%s_weights" % name].tobytes()


def test_pinned_boxes(golden):
    from autoware_vision_pilot_amd import lib

    h, w = 40, 50
    for dataset in lc.ROI_DATASETS:
        box = lib.sceneseg_roi(dataset, w, h)
        size = (w, h) if box is None else (box[2] - box[0], box[3] - box[1])
        assert size == tuple(int(v) for v in golden["roi_" + dataset]), dataset
    assert lib.sceneseg_roi("ACDC", 1920, 1080) == (0, 0, 1919, 990) and lib.sceneseg_roi("BDD100K", 1280, 720) == (0, 0, 1000, 500)
    assert lib.sceneseg_roi("IDDAW", 2048, 1536) == (0, 476, 2047, 1500) and lib.sceneseg_roi("MUSES", 1920, 1080) == (0, 0, 1919, 918)
    assert lib.sceneseg_roi("COMMA10K", 1164, 874) == (0, 0, 1163, 611) and lib.sceneseg_roi("MAPILLARY", 10, 10) is None and lib.sceneseg_roi("other", 1, 1) is None


@pytest.mark.parametrize("tag", ("f32", "f64"))
@pytest.mark.parametrize("name", DEPTH_PINS)
def test_depth_reference_equals_the_pinned_loader(golden, name, tag):
    """getItemVal's normalisation at full resolution (identity tables), bits"""
    v, truth = golden["depth_%s_%s_label" % (name, tag)], golden["depth_%s_%s_truth" % (name, tag)]
    assert v.dtype == truth.dtype == (np.float32 if tag == "f32" else np.float64)
    assert np.array_equal(v, lc.depth_case(name, v.dtype), equal_nan=True)
    gt, rec = lc.depth_ref(v, v.shape)
    assert lc.same_f32(gt, truth.astype(np.float32)), name
    assert rec["nonfinite"] == int((~np.isfinite(v)).sum()) and rec["n"] == v.size
    if name in ("constant", "one_nan"):
        assert np.isnan(gt).all()
    if name == "one_nan":
        assert np.isnan(rec["min"]) and np.isnan(rec["max"]) and rec["nonfinite"] == 1
    if name == "one_inf":
        assert rec["max"] == np.inf and rec["nonfinite"] == 1 and (gt[np.isfinite(gt)] == 0).all() and np.isnan(gt).sum() == 1


@pytest.mark.parametrize("box", ((0, 0, 33, 20), (0, 10, 63, 50), (-3, -2, 15, 9), (5, 5, 9, 8), (30, 0, 40, 12), (0, 476, 2047, 1500)))
@pytest.mark.parametrize("mode", ("RGB", "L"))
def test_crop_pads_as_pil_does(box, mode):
    img = lc.palette_image(40, 34, 21)
    if mode == "L":
        img = np.ascontiguousarray(img[..., 0])
    want = np.array(Image.fromarray(img, mode).crop(box))
    got, outside = lc.crop_pad(img, box)
    assert np.array_equal(got, want)
    ys, xs = np.arange(box[1], box[3]), np.arange(box[0], box[2])
    assert outside == got.shape[0] * got.shape[1] - int(((ys >= 0) & (ys < 40)).sum()) * int(((xs >= 0) & (xs < 34)).sum())


def test_class_weights_and_zero_extremes():
    from autoware_vision_pilot_amd import lib

    assert lib.class_weights({"n": 1899810, "freq": (0, 5120, 1894690)}) == [1899810 / 5120, 1899810 / 10240, 1899810 / 1899810]
    z = np.array([[0.0, -0.0], [1.0, 0.0]])
    mn, mx = lc.extremes(z)
    assert np.signbit(mn) and mn == 0 and mx == 1
    mn, mx = lc.extremes(-z)
    assert mn == -1 and mx == 0 and not np.signbit(mx)
    # sampling the classes equals classifying the samples: both maps are per pixel
    img = lc.palette_image(37, 53, 22)
    gt, _ = lc.seg_ref(img, (16, 24))
    assert np.array_equal(gt, lc.classify(img[lc.nearest_index(37, 16)][:, lc.nearest_index(53, 24)], lc.COLOURS))


def test_binding_refuses_what_is_not_a_label():
    from autoware_vision_pilot_amd import lib

    for bad in (np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4), np.int16), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError):
            lib._label_u8(bad)
    for bad in (np.zeros((4, 4), np.float16), np.zeros((4, 4, 1), np.float32)):
        with pytest.raises(ValueError):
            lib._label_depth(bad)
    a, ch, h, w, stride = lib._label_u8(lc.strided(lc.palette_image(5, 7, 23), 3, 9))
    assert (ch, h, w, stride) == (3, 5, 7, 30)
    a, dt, h, w, stride = lib._label_depth(lc.depth_case("strided", np.float64))
    assert (dt, h, w, stride) == (lib.VP_LABEL_F64, 21, 30, 33)
