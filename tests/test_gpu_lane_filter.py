"""vp_lanes on the MI355X: the whole case set of tests/lane_filter_cases.py through the operator entry, bit for bit against the numpy twin; the
smoothing sequence; the engine entry against the operator entry on the engine's own logits (stand-alone engines and a shared-prefix head); the ordering
against queued passes; every refusal.  All planes are 3 x 80 x 160."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- first: one shared HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lane_filter_cases as lc  # noqa: E402
import lane_filter_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib as _lib

    return _lib


@pytest.fixture(scope="module")
def frames():
    from oracle import pre_post

    return [pre_post.synthetic_frame(360, 640, s) for s in (31, 32, 33)]


def record_of_logits(lib, lg, thr):
    """(record, point lists) of the operator entry on a fresh handle"""
    lanes = lib.Lanes(capacity=1)
    try:
        lanes.add_logits(lg, thr)
        pts = [lanes.fetch_points(0, lane) for lane in (0, 1)]
        return lanes.fetch()[0], pts
    finally:
        lanes.close()


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))


# ---- 1. the whole set through the operator entry
def test_hand_made_cases(lib):
    frames_ = [lc.HAND[k][0] for k in lc.HAND_NAMES]
    thr = [lc.HAND[k][1] for k in lc.HAND_NAMES]
    wants = [ref.LaneFilterRef().update(f, t) for f, t in zip(frames_, thr)]
    for k, w in zip(lc.HAND_NAMES, wants):
        assert tuple(lc.lane_tuple(r) for r in w) == lc.EXPECT[k], k
    lc.run_and_check(lib, frames_, thr, wants, capacity=5)


def test_generated_set(lib):
    frames_, results, _, _ = lc.generated()
    lc.run_and_check(lib, frames_, [0.0] * len(frames_), results, capacity=64)


# ---- 2. the smoothing sequence
def test_sequence_and_reset(lib):
    lc.check_sequence(lib)


# ---- 3. the engine entry equals the operator entry on the engine's own logits
@pytest.mark.parametrize("prec", ("fp16", "fp16x3"))
def test_add_engine_equals_add_logits(lib, engines, frame720, prec):
    eng = engines("egolanes", prec)
    eng.infer(frame720)
    lg = eng.logits()
    assert lg.shape == (3, 80, 160)
    thr = float(np.median(lg))
    lanes = lib.Lanes(capacity=2)
    try:
        lanes.add(eng, thr)
        pts = [lanes.fetch_points(0, lane) for lane in (0, 1)]
        got = (lanes.fetch()[0], pts)
    finally:
        lanes.close()
    want = record_of_logits(lib, lg, thr)
    assert same(got, want)
    twin = ref.LaneFilterRef().update(lg, thr)                   # and both are the twin's
    for lane in (0, 1):
        lc.check_lane(got[0]["lane"][lane], got[1][lane], twin[lane])
    assert (lg > thr).sum() > 1000                               # the median splits the planes: there is something to search


def test_add_shared_prefix_head(lib, state_dicts, frame720):
    from autoware_vision_pilot_amd import synthetic, weights as vw

    sd_seg = state_dicts("sceneseg")
    sd_ego = synthetic.share_backbone(dict(state_dicts("egolanes")), "egolanes", sd_seg, "sceneseg")
    base = lib.Engine("sceneseg", vw.pack_state_dict(sd_seg), precision="fp16")
    head = lib.Engine("egolanes", vw.pack_state_dict(sd_ego), precision="fp16", base=base)
    lanes = lib.Lanes(capacity=2)
    try:
        base.infer(frame720)
        head.infer_shared()
        lg = head.logits()
        thr = float(np.median(lg))
        lanes.add(head, thr)
        pts = [lanes.fetch_points(0, lane) for lane in (0, 1)]
        got = (lanes.fetch()[0], pts)
        assert same(got, record_of_logits(lib, lg, thr))
        with pytest.raises(ValueError, match="VP_EGOLANES engines only"):
            lanes.add(base, 0.0)
    finally:
        lanes.close()
        head.close()
        base.close()


# ---- 4. ordering without host waits
def test_adds_are_ordered_against_queued_passes(lib, engines, frames):
    """three passes on three frames, an add behind each, nothing synchronised in between, one fetch: each record is its own frame's"""
    ego = engines("egolanes", "fp16")
    fr = [lib.Frame() for _ in frames]
    lanes = lib.Lanes(capacity=4)
    try:
        for f, img in zip(fr, frames):
            f.upload(img, "bgr8")
        logits = []
        for f in fr:                                             # the stand-alone passes (they also take the engine past its eager first pass)
            ego.infer_frame(f)
            logits.append(ego.logits().copy())
        thr = float(np.median(logits[0]))
        want = [record_of_logits(lib, lg, thr) for lg in logits]
        assert want[0][0].tobytes() != want[1][0].tobytes() and want[1][0].tobytes() != want[2][0].tobytes()
        for f in fr:
            ego.upload_from_frame(f)
            ego.enqueue()
            lanes.add(ego, thr)
        assert lanes.pending() == 3
        pts = [[lanes.fetch_points(i, lane) for lane in (0, 1)] for i in range(3)]
        recs = lanes.fetch()
        ego.fetch_outputs()
        # one handle saw the three frames in a row, so its coefficients are smoothed; everything the device wrote and the raw fit are each frame's own
        prev = [None, None]
        for i in range(3):
            twin = ref.LaneFilterRef().update(logits[i], thr)
            for lane in (0, 1):
                g, w = recs[i]["lane"][lane], want[i][0]["lane"][lane]
                for k in ("start_x", "start_y", "n_windows_up", "n_windows_down", "n_points_up", "n_points_down", "min_y", "max_y", "S", "T", "windows", "order", "raw_coeffs"):
                    assert g[k].tobytes() == w[k].tobytes(), (i, lane, k)
                assert pts[i][lane].tobytes() == want[i][1][lane].tobytes()
                prev[lane] = lc.check_lane(g, pts[i][lane], twin[lane], prev[lane])
    finally:
        lanes.close()
        for f in fr:
            f.close()


# ---- 5. refusals
def test_refusals_without_an_engine(lib):
    lc.check_refusals_no_engine(lib)


def test_refusals_with_engines(lib, engines, state_dicts, frames):
    from autoware_vision_pilot_amd import weights as vw

    ego, seg = engines("egolanes", "fp16"), engines("sceneseg", "fp16")
    for e in (ego, seg):
        e.infer(frames[0])
    fresh = lib.Engine("egolanes", vw.pack_state_dict(state_dicts("egolanes")), precision="fp16")
    lanes = lib.Lanes(capacity=1)
    try:
        with pytest.raises(ValueError, match="VP_EGOLANES engines only"):
            lanes.add(seg, 0.0)
        with pytest.raises(lib.VpError, match="Inference has not been run yet"):
            lanes.add(fresh, 0.0)
        assert lanes.pending() == 0
        lanes.add(ego, 0.0)
        with pytest.raises(lib.VpError, match="pending already"):
            lanes.add(ego, 0.0)
        with pytest.raises(lib.VpError, match="pending"):
            lanes.reset()
        assert lanes.pending() == 1 and len(lanes.fetch()) == 1
        if torch.cuda.device_count() > 1:                        # a filter on another GPU than the engine
            other = lib.Lanes(gpu_id=1, capacity=1)
            try:
                with pytest.raises(ValueError, match="lives on GPU"):
                    other.add(ego, 0.0)
            finally:
                other.close()
    finally:
        lanes.close()
        fresh.close()
