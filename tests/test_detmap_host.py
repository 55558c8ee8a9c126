"""The detector's validation mAP without a GPU: the restatement tests/detmap_ref.py against the fixture the reference's own code wrote
(tests/golden/detmap.npz, tools/pin_detmap.py), the host entry vp_metric_det_ap against the reference's compute_ap results, and the ABI."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import abi  # noqa: E402
import detmap_cases as dc  # noqa: E402
import detmap_ref as dr  # noqa: E402

NEW_SYMBOLS = ("vp_metric_add_det", "vp_metric_add_det_pair", "vp_metric_add_det_raw", "vp_metric_det_frames", "vp_metric_fetch_det", "vp_metric_det_ap",
               "vp_op_detect_validate")


@pytest.fixture(scope="module")
def golden():
    return dc.golden()


@pytest.fixture(scope="module")
def ref_frames():
    """the restatement on every frame, computed once: name -> (rows, tp, counts, labels)"""
    out = {}
    for name in dc.FRAMES:
        raw, labels = dc.frame(name)
        rows, tp, counts = dr.run_frame(raw, dc.labels_px(labels), dc.IOU_V, dc.CONF, dc.IOU)
        out[name] = (rows, tp, counts, labels)
    return out


def test_the_fixture_holds_every_frame_and_the_inputs_are_the_pinned_ones(golden):
    assert tuple(str(n) for n in golden["frames"]) == dc.FRAMES
    assert np.array_equal(golden["iou_v_bits"], dc.bits(dc.IOU_V))
    for name in dc.FRAMES:
        assert dc.digest(*dc.frame(name)) == str(golden[name + "_sha256"]), name


def test_the_cases_exercise_what_they_are_for(golden):
    counts = {n: tuple(int(v) for v in golden[n + "_counts"]) for n in dc.FRAMES}
    assert 0 < counts["small"][0] < 64 and counts["small"][2] > 0
    assert counts["small_empty"] == counts["small_miss"] == (0, 0, 0) and dc.frame("small_miss")[1].shape[0] == 2 and dc.frame("small_empty")[1].shape[0] == 0
    assert counts["small_nolabel"][2] > 0 and dc.frame("small_nolabel")[1].shape[0] == 0
    assert counts["mid"][0] > 2048 and counts["mid"][0] & (counts["mid"][0] - 1) and counts["mid"][2] == dc.MAX_DET
    assert counts["dense"][0] > dc.MAX_NMS == counts["dense"][1] and counts["dense"][2] == dc.MAX_DET
    raw = dc.frame("dense")[0]
    assert np.isnan(raw[4:]).sum() == 1 and ((raw[2] == 0) & (raw[3] == 0)).sum() == 2
    # mid: the stop at max_det cut survivors off; class offsets decide suppressions (the agnostic rule keeps another set); shared best labels
    raw, labels = dc.frame("mid")
    assert dr.validate(raw, dc.CONF, dc.IOU, max_det=10 ** 6)[1][2] > dc.MAX_DET
    rows = golden["mid_rows"]
    sc = raw[4:].T
    i, c = np.nonzero(sc > np.float32(dc.CONF))
    order = np.argsort(-sc[i, c], kind="stable")
    cx, cy, w, h = (raw[k][i[order]] for k in range(4))
    box = np.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), 1).astype(np.float32)
    agnostic = dr.greedy(box, np.float32(dc.IOU), dc.MAX_DET)
    assert not np.array_equal(dc.bits(box[agnostic]), dc.bits(rows[:, :4]))
    iou = dr.pair_iou(rows, dc.labels_px(labels))
    same = labels[:, None, 0] == rows[None, :, 5]
    best = np.where(same, iou, -1).argmax(0)[(np.where(same, iou, -1).max(0) >= 0.5)]
    assert best.size > np.unique(best).size


def test_restatement_reproduces_the_fixture_bit_for_bit(golden, ref_frames):
    for name in dc.FRAMES:
        rows, tp, counts, _ = ref_frames[name]
        want_rows, want_tp, want_counts = dc.golden_frame(golden, name)
        assert counts == want_counts, name
        assert np.array_equal(dc.bits(rows), dc.bits(want_rows)), name
        assert np.array_equal(tp, want_tp), name


def dataset(golden):
    return dc.dataset_arrays([(golden[n + "_rows"], golden[n + "_tp"], dc.frame(n)[1]) for n in dc.FRAMES])


def test_restatement_dataset_scores_are_compute_ap(golden):
    s = dr.dataset_scores(*dataset(golden))
    assert s["grid_index"] == int(golden["ds_grid_index"])
    assert np.abs(np.array([s["precision"], s["recall"], s["map50"], s["map"]]) - golden["ds_scores"]).max() <= 1e-12
    assert np.array_equal(s["tp"], golden["ds_tp"]) and np.array_equal(s["fp"], golden["ds_fp"])


def test_det_ap_is_compute_ap(golden):
    """the library's host code against the reference's compute_ap: 1e-12 absolute on scores in [0, 1] (the bar of tests/test_rectify_host.py for double
    host arithmetic), the chosen grid index and the rounded tp / fp exactly"""
    from autoware_vision_pilot_amd import lib

    tp, conf, cls, lab = dataset(golden)
    s = lib.det_ap(tp, conf, cls, lab, n_iou=10)
    got = np.array([s["precision"], s["recall"], s["map50"], s["map"]])
    print("det_ap", got.tolist(), "reference", golden["ds_scores"].tolist(), "max abs difference", np.abs(got - golden["ds_scores"]).max())
    assert s["rows"] == int(golden["ds_rows"]) == tp.size and s["labels"] == int(golden["ds_labels"]) == lab.size
    assert np.array_equal(s["class_id"], golden["ds_classes"]) and s["classes"] == golden["ds_classes"].size
    assert s["grid_index"] == int(golden["ds_grid_index"])
    assert np.abs(got - golden["ds_scores"]).max() <= 1e-12
    assert np.array_equal(s["tp"], golden["ds_tp"]) and np.array_equal(s["fp"], golden["ds_fp"])
    ref = dr.dataset_scores(tp, conf, cls, lab)
    assert np.abs(s["ap50"] - ref["ap50"]).max() <= 1e-12 and np.abs(s["ap"] - ref["ap"]).max() <= 1e-12
    assert np.array_equal(s["class_labels"], ref["class_labels"])


def test_det_ap_all_false_tp_gives_four_zeros(golden):
    from autoware_vision_pilot_amd import lib

    tp, conf, cls, lab = dataset(golden)
    s = lib.det_ap(np.zeros_like(tp), conf, cls, lab)
    assert (s["precision"], s["recall"], s["map50"], s["map"], s["grid_index"]) == (0.0, 0.0, 0.0, 0.0, -1)
    assert s["classes"] == 3 and not s["ap"].any() and not s["tp"].any()
    assert lib.det_ap(tp << np.uint32(10), conf, cls, lab)["map"] == 0.0            # bits beyond n_iou are no hits
    empty = lib.det_ap([], [], [], [])
    assert (empty["rows"], empty["classes"], empty["map"]) == (0, 0, 0.0)
    with pytest.raises(ValueError):
        lib.det_ap(tp, conf, cls, lab, n_iou=17)


def test_new_symbols_are_declared_exported_and_bound_and_the_structs_match():
    from autoware_vision_pilot_amd import lib

    src = abi.header_source()
    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in exported and s in lib.EXPORTED_SYMBOLS, s
    for name, value in (("VP_DET_MAX_NMS", 30000), ("VP_DET_MAX_DET", 300), ("VP_DET_MAX_CLASSES", 80), ("VP_DET_MAX_IOU", 16), ("VP_DET_MAX_LABELS", 4096)):
        assert "#define %s %d" % (name, value) in src and getattr(lib, name) == value
    assert "uint32_t candidates, ranked, kept, labels, first_row;" in src and "float x1, y1, x2, y2, conf, cls;" in src
    assert lib.METRIC_DET_FRAME_DTYPE.itemsize == 20 and lib.METRIC_DET_ROW_DTYPE.itemsize == 28 and lib.METRIC_DET_ROW_DTYPE.fields["tp"][1] == 24
    S = lib.MetricDetSummary
    assert S.precision.offset == 24 and S.class_id.offset == 56 and S.class_labels.offset == 376 and S.ap50.offset == 696 and ct.sizeof(S) == 696 + 4 * 640
    # the defaults: the trainer's thresholds and torch.linspace(0.5, 0.95, 10) from its bits
    import torch

    assert (lib.DET_CONF, lib.DET_IOU) == (0.001, 0.65) and np.array_equal(lib.DET_IOU_V, torch.linspace(0.5, 0.95, 10).numpy())
    assert "3f000000 3f0ccccd 3f19999a 3f266666 3f333333 3f400000 3f4ccccd 3f59999a 3f666666 3f733333" in open(abi.HEADER).read()
    assert ct.sizeof(lib.MetricFrame) == 72                                            # vp_metric_frame is unchanged
