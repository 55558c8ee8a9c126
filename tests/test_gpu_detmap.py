"""The detector's validation mAP on the MI355X (vp_metric_add_det*, include/vp_hip.h): every case of tests/detmap_cases.py bit for bit against the
fixture of the reference's own code, run-to-run equality, the engine entries against the operator entry, the pair form, the refusals, and scene
records beside detector records in one vp_metric."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- first: one shared HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import detmap_cases as dc  # noqa: E402
import detmap_ref as dr  # noqa: E402

pytestmark = pytest.mark.gpu
FRAME = (720, 1280, 21)


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib as _lib

    return _lib


@pytest.fixture(scope="module")
def detectors(lib):
    """VP_AUTOSPEED engines on synthetic weights, one per precision, each with a pass on the same frame behind it"""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    blob = vw.pack_state_dict(synthetic.make_autospeed_state_dict(5))
    frame = synthetic.synthetic_frame(*FRAME)
    out = {}
    for prec in ("fp16", "fp16x3"):
        eng = lib.Engine("autospeed", blob, precision=prec)
        det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
        det.attach(eng)
        det.infer(frame, 0.25, 0.45)
        out[prec] = (eng, det)
    yield out
    for eng, det in out.values():
        det.close()
        eng.close()


def labels_for(seed, n=5):
    rng = np.random.default_rng(seed)
    return dc._labels(rng, n)


# ---- 1. the cases, bit for bit
@pytest.mark.parametrize("name", dc.SINGLE)
def test_detect_validate_bit_for_bit(lib, name):
    dc.check_validate(lib, name)


@pytest.mark.parametrize("name", dc.SINGLE)
def test_add_det_raw_one_frame_bit_for_bit_and_equal_from_run_to_run(lib, name):
    dc.check_frames(lib, (name,))


def test_dataset_records_and_summary_against_compute_ap(lib):
    s = dc.check_frames(lib, dc.FRAMES)
    g = dc.golden()
    assert np.array_equal(s["tp"], g["ds_tp"]) and np.array_equal(s["fp"], g["ds_fp"]) and np.array_equal(s["class_id"], g["ds_classes"])
    assert s["rows"] == int(g["ds_rows"]) and s["labels"] == int(g["ds_labels"])


# ---- 2. the engine entries
@pytest.mark.parametrize("prec", ("fp16", "fp16x3"))
def test_add_det_equals_add_det_raw_on_the_fetched_tensor(lib, detectors, prec):
    eng, _ = detectors[prec]
    raw = eng.logits().reshape(8, 10752).copy()
    labels = labels_for(3)
    m = lib.Metric(max_frames=4)
    try:
        m.add_det(eng, labels)
        m.add_det_raw(raw, labels, (512, 1024))
        m.add_det(eng, None)
        fr, rows, s = m.fetch_det()
        k = int(fr[0]["kept"])
        assert fr[0]["candidates"] > 0 and k > 0 and fr[1]["first_row"] == k and fr[2]["labels"] == 0
        for f in ("candidates", "ranked", "kept"):
            assert fr[0][f] == fr[1][f] == fr[2][f]
        assert rows[:k].tobytes() == rows[k:2 * k].tobytes()
        assert dc.rows_of(rows[:k]).tobytes() == dc.rows_of(rows[2 * k:3 * k]).tobytes() and not rows[2 * k:3 * k]["tp"].any()
        want_rows, want_tp, want_counts = dr.run_frame(raw, dc.labels_px(labels), dc.IOU_V)
        assert (int(fr[0]["candidates"]), int(fr[0]["ranked"]), k) == want_counts
        assert np.array_equal(dc.bits(dc.rows_of(rows[:k])), dc.bits(want_rows)) and np.array_equal(rows[:k]["tp"], want_tp)
        assert s["frames"] == 3 and s["rows"] == 3 * k and s["labels"] == 10
    finally:
        m.close()


def test_pair_with_itself_matches_every_label_at_all_thresholds(lib, detectors):
    eng, _ = detectors["fp16"]
    x3, _ = detectors["fp16x3"]
    raw = eng.logits().reshape(8, 10752).copy()
    label_conf = 0.4                                   # the threshold tests/golden/autospeed_net.npz was pinned at: 20 .. 2000 boxes above it on this frame
    m = lib.Metric(max_frames=4)
    try:
        m.add_det_pair(eng, eng, label_conf)
        m.add_det_pair(eng, x3, label_conf)
        fr, rows, s = m.fetch_det()
        k = int(fr[0]["kept"])
        mine = rows[:k]
        n_lab = int((mine["conf"] > np.float32(label_conf)).sum())
        assert n_lab > 0 and fr[0]["labels"] == n_lab
        assert (mine["tp"][:n_lab] == 0x3FF).all() and not mine["tp"][n_lab:].any()      # scores descend: the labels are the first rows
        assert fr[1]["labels"] > 0 and fr[1]["first_row"] == k
        m.reset()
        m.add_det_pair(eng, eng, label_conf)
        _, _, alone = m.fetch_det()
        want = dr.dataset_scores(mine["tp"], mine["conf"], mine["cls"], mine["cls"][:n_lab])
        print("pair with itself: map", alone["map"], "the 101-point integration on the same rows", want["map"])
        assert abs(alone["map"] - want["map"]) <= 1e-12 and abs(alone["map50"] - want["map50"]) <= 1e-12
        assert alone["grid_index"] == want["grid_index"]
        want_rows = dr.validate(raw)[0]
        assert np.array_equal(dc.bits(dc.rows_of(mine)), dc.bits(want_rows))
    finally:
        m.close()


# ---- 3. refusals
def test_refusals(lib, detectors, engines, state_dicts):
    from autoware_vision_pilot_amd import synthetic, weights as vw

    eng, _ = detectors["fp16"]
    seg = engines("sceneseg", "fp16")
    seg.infer(synthetic.synthetic_frame(360, 640, 3))
    fresh = lib.Engine("autospeed", vw.pack_state_dict(synthetic.make_autospeed_state_dict(5)), precision="fp16")
    raw, labels = dc.frame("small")
    m = lib.Metric(max_frames=2)
    try:
        for bad in (lambda: m.add_det(seg, labels), lambda: m.add_det_pair(eng, seg), lambda: m.add_det_pair(seg, eng),
                    lambda: m.add_det(eng, labels, iou_v=np.zeros(17, np.float32)), lambda: m.add_det(eng, labels, iou_v=np.zeros(0, np.float32)),
                    lambda: m.add_det(eng, np.zeros((4097, 5), np.float32)), lambda: m.add_det(eng, labels, conf=float("nan")),
                    lambda: m.add_det_raw(np.zeros((4 + 81, 8), np.float32), labels), lambda: m.add_det_raw(np.zeros((5, 16385), np.float32), labels),
                    lambda: m.add_det_raw(np.zeros((4 + 80, 2048), np.float32), labels),
                    lambda: m._ck(lib.load().vp_metric_add_det_raw(m._h, None, 0, 1, 64, 512, 1024, None, 0, 0.001, 0.65, lib._ptr(dc.IOU_V), 10)),
                    lambda: m._ck(lib.load().vp_metric_add_det(m._h, eng._h, None, 2, 0.001, 0.65, lib._ptr(dc.IOU_V), 10)),
                    lambda: m._ck(lib.load().vp_metric_add_det(m._h, eng._h, None, 0, 0.001, 0.65, None, 10)),
                    lambda: lib.detect_validate(np.zeros((4 + 81, 8), np.float32))):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(lib.VpError, match="Inference has not been run yet"):
            m.add_det(fresh, labels)
        with pytest.raises(lib.VpError, match="Inference has not been run yet"):
            m.add_det_pair(eng, fresh)
        assert m.det_frames() == 0
        m.add_det_raw(raw, labels)
        with pytest.raises(ValueError, match="another threshold table"):
            m.add_det_raw(raw, labels, iou_v=dc.IOU_V[:5])
        m.add_det(eng, labels)
        with pytest.raises(lib.VpError, match="full"):
            m.add_det(eng, labels)
        m.reset()
        assert m.det_frames() == 0
        m.add_det_raw(raw, labels, iou_v=dc.IOU_V[:5])                                   # a reset frees the table
        assert m.fetch_det()[2]["n_iou"] == 5
    finally:
        m.close()
        fresh.close()


# ---- 4. scene records and detector records in one vp_metric
def test_scene_and_detector_records_do_not_touch_each_other(lib, detectors, engines):
    from autoware_vision_pilot_amd import synthetic

    eng, _ = detectors["fp16"]
    seg = engines("sceneseg", "fp16")
    seg.infer(synthetic.synthetic_frame(360, 640, 4))
    h, w = seg.output_dims()[-2:]
    gt = np.random.default_rng(8).integers(0, 4, (h, w)).astype(np.uint8)
    raw, labels = dc.frame("mid")
    lab2 = labels_for(6)
    scene, det = lib.Metric(max_frames=4), lib.Metric(max_frames=4)
    both = lib.Metric(max_frames=4)
    try:
        scene.add_seg(seg, gt)
        scene.add_seg(seg, gt, "bits")
        det.add_det_raw(raw, labels)
        det.add_det(eng, lab2)
        both.add_seg(seg, gt)
        both.add_det_raw(raw, labels)
        both.add_seg(seg, gt, "bits")
        both.add_det(eng, lab2)
        assert (both.frames(), both.det_frames()) == (2, 2) and (scene.det_frames(), det.frames()) == (0, 0)
        rec_b, sum_b = both.fetch()
        fr_b, rows_b, s_b = both.fetch_det()
        rec_s, sum_s = scene.fetch()
        fr_d, rows_d, s_d = det.fetch_det()
        assert rec_b.tobytes() == rec_s.tobytes() and repr(sum_b) == repr(sum_s)
        assert fr_b.tobytes() == fr_d.tobytes() and rows_b.tobytes() == rows_d.tobytes() and s_b["map"] == s_d["map"] and s_b["rows"] == s_d["rows"] > 300
        assert scene.fetch_det()[2]["frames"] == 0 and det.fetch()[1]["frames"] == 0
    finally:
        for m in (scene, det, both):
            m.close()
