"""vp_metric's lane part on the MI355X: the cases of tests/metric_lanes_cases.py on the device, and the engine entries: engine add against operator add,
the ordering against queued passes, the pair forms, run-to-run determinism, the refusals."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- first: one shared HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import metric_lanes_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib as _lib

    return _lib


@pytest.fixture(scope="module")
def frames():
    from oracle import pre_post

    return [pre_post.synthetic_frame(360, 640, s) for s in (31, 32, 33)]


@pytest.fixture(scope="module")
def steer_frames():
    from oracle import pre_post

    return [pre_post.synthetic_frame(512, 1024, s) for s in (41, 42, 43)]


@pytest.fixture(scope="module")
def steer(lib):
    """AutoSteer engines, fp16 and fp16x3, on the synthetic weights"""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    blob = vw.pack_state_dict(synthetic.make_autosteer_state_dict(0))
    out = {p: lib.Engine("autosteer", blob, precision=p) for p in ("fp16", "fp16x3")}
    yield out
    for e in out.values():
        e.close()


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


def lane_truth(engine, seed):
    h, w = engine.output_dims()[-2:]
    return lc.general_inputs((h, w), seed=seed)[1]


def row_targets(seed, rows=64):
    rng = np.random.default_rng(seed)
    return rng.random(rows).astype(np.float32), (rng.random(rows) < 0.7).astype(np.float32)


def rows_of(engine):
    lg = engine.logits()
    assert lg.shape == (2, 64, 1)
    return lg[0].reshape(-1), lg[1].reshape(-1)


# ---- 1. the shared cases
@pytest.mark.parametrize("shape", lc.EXACT_SHAPES, ids=ids(lc.EXACT_SHAPES))
def test_lanes_edge_exact(lib, shape):
    lc.check_lanes_exact(lib, shape)


@pytest.mark.parametrize("shape", lc.GENERAL_SHAPES, ids=ids(lc.GENERAL_SHAPES))
def test_lanes_general(lib, shape):
    lc.check_lanes_general(lib, shape)


def test_lanes_gt_forms(lib):
    lc.check_lanes_gt_forms(lib)


def test_lanes_nan_answers(lib):
    lc.check_lanes_nan_answers(lib)


def test_lanes_accumulator(lib):
    lc.check_lanes_accumulator(lib, lib.VpError)


def test_lanes_and_rows_refusals_without_an_engine(lib):
    lc.check_lanes_refusals(lib)


@pytest.mark.parametrize("case", lc.ROWS_DYADIC, ids=["%dx%d" % c[:2] for c in lc.ROWS_DYADIC])
def test_rows_dyadic_bit_for_bit(lib, case):
    lc.check_rows_dyadic(lib, case)


@pytest.mark.parametrize("case", lc.ROWS_GENERAL, ids=["%dx%d" % c[:2] for c in lc.ROWS_GENERAL])
def test_rows_general(lib, case):
    lc.check_rows_general(lib, case)


def test_rows_special_values(lib):
    lc.check_rows_special(lib)


def test_device_pointers_are_accepted(lib):
    """logits and ground truth already on the device (torch tensors): the record of the host arrays"""
    lg, bits = lc.general_inputs((17, 33), seed=5)
    d_lg, d_bits = torch.from_numpy(lg).cuda(), torch.from_numpy(bits).cuda()
    d_big = torch.from_numpy(lc.bits_4x(bits, 9)).cuda()
    d_planes = torch.from_numpy(lc.planes_of_bits(bits)).cuda()
    torch.cuda.synchronize()
    m = lib.Metric(max_frames=4)
    try:
        m.add_lanes_logits(lg, bits)
        for gt, form in ((d_bits, "bits"), (d_big, "bits4x"), (d_planes, "planes")):
            m.add_lanes_logits(d_lg.data_ptr(), gt.data_ptr(), form, device_hw=(17, 33))
        rec, _ = m.fetch_lanes()
        assert all(rec[k:k + 1].tobytes() == rec[0:1].tobytes() for k in (1, 2, 3)) and np.isfinite(rec[0]["score"])
    finally:
        m.close()


# ---- 2. the engine path equals the operator path
def test_add_lanes_equals_add_lanes_logits(lib, engines, frames):
    m = lib.Metric(max_frames=8)
    try:
        for prec in ("fp16", "fp16x3"):
            eng = engines("egolanes", prec)
            eng.infer(frames[0])
            lg = eng.logits()
            assert lg.shape == (3, 80, 160)
            bits = lane_truth(eng, 3)
            for gt, form in ((bits, "bits"), (lc.bits_4x(bits, 4), "bits4x"), (lc.planes_of_bits(bits), "planes")):
                m.reset()
                m.add_lanes(eng, gt, form)
                m.add_lanes_logits(lg, gt, form)
                rec, _ = m.fetch_lanes()
                assert rec[0:1].tobytes() == rec[1:2].tobytes() and np.isfinite(rec[0]["score"]) and rec[0]["n"] == 12800 and rec[0]["nonfinite"] == 0
            want = lc.lanes_ref(lg, lc.planes_of_bits(bits), torch.float64)
            assert abs(float(rec[0]["score"]) - want["score"]) <= lc.lanes_bars(lg, want, want)["score"][0]
    finally:
        m.close()


def test_add_rows_equals_add_rows_raw(lib, steer, steer_frames):
    m = lib.Metric(max_frames=8)
    try:
        for prec, eng in steer.items():
            eng.infer(steer_frames[0])
            xp, hv = rows_of(eng)
            txp, th = row_targets(5)
            m.reset()
            m.add_rows(eng, txp, th)
            m.add_rows_raw(xp, hv, txp, th)
            rec, s = m.fetch_rows()
            assert rec[0:1].tobytes() == rec[1:2].tobytes() and s["lines"] == 2
            want = lc.rows_ref(xp, hv, txp, th)
            assert abs(float(rec[0]["dist"]) - want["dist"][0]) <= 2.0 ** -23 * want["dist"][0] and int(rec[0]["target_valid"]) == int(want["target_valid"][0])
    finally:
        m.close()


# ---- 3. ordering without host waits
def test_lane_adds_are_ordered_against_queued_passes(lib, engines, steer, frames, steer_frames):
    """three passes on different frames, each followed by an add, nothing synchronised in between, ONE fetch of each kind: each record is what the
    operator entry gives for that frame's outputs, fetched separately"""
    ego, st = engines("egolanes", "fp16"), steer["fp16"]
    m = lib.Metric(max_frames=16)
    fr, sfr = [lib.Frame() for _ in frames], [lib.Frame() for _ in steer_frames]
    try:
        for f, img in zip(fr + sfr, frames + steer_frames):
            f.upload(img, "bgr8")
        gts = [lane_truth(ego, 50 + i) for i in range(3)]
        tgs = [row_targets(60 + i) for i in range(3)]
        for i in range(3):                      # the stand-alone passes (they also take the engines past their eager first pass)
            ego.infer_frame(fr[i])
            st.infer_frame(sfr[i])
            m.add_lanes_logits(ego.logits(), gts[i])
            m.add_rows_raw(*rows_of(st), *tgs[i])
        want_l, want_r = m.fetch_lanes()[0], m.fetch_rows()[0]
        assert want_l[0:1].tobytes() != want_l[2:3].tobytes() and want_r[0:1].tobytes() != want_r[2:3].tobytes()
        m.reset()
        for i in range(3):
            ego.upload_from_frame(fr[i])
            ego.enqueue()
            m.add_lanes(ego, gts[i])
            st.upload_from_frame(sfr[i])
            st.enqueue()
            m.add_rows(st, *tgs[i])
        got_l, got_r = m.fetch_lanes()[0], m.fetch_rows()[0]
        assert got_l.tobytes() == want_l.tobytes() and got_r.tobytes() == want_r.tobytes()
        ego.fetch_outputs()
        st.fetch_outputs()
    finally:
        m.close()
        for f in fr + sfr:
            f.close()


# ---- 4. the pair forms
def test_pair_forms(lib, engines, steer, frames, steer_frames):
    ego, egox3 = engines("egolanes", "fp16"), engines("egolanes", "fp16x3")
    m = lib.Metric(max_frames=8)
    try:
        for e in (ego, egox3):
            e.infer(frames[2])
        for e in steer.values():
            e.infer(steer_frames[2])
        own = (ego.logits() > 0).astype(np.float32)
        m.add_lanes_pair(ego, ego)
        m.add_lanes_logits(ego.logits(), own, "planes")
        m.add_lanes_pair(ego, egox3)
        m.add_lanes_logits(ego.logits(), (egox3.logits() > 0).astype(np.float32), "planes")
        rec, s = m.fetch_lanes()
        assert rec[0]["bce"].tobytes() == rec[1]["bce"].tobytes() and rec[0:1].tobytes() == rec[1:2].tobytes()
        assert rec[2:3].tobytes() == rec[3:4].tobytes() and s["nan_frames"] == 0
        assert (rec[0]["bce"] <= np.log(2.0) + 1e-6).all()                 # its own prediction as the truth: no term above log 2
        m.add_rows_pair(steer["fp16"], steer["fp16"])
        m.add_rows_pair(steer["fp16"], steer["fp16x3"])
        rows, rs = m.fetch_rows()
        assert float(rows[0]["dist"]) == 0.0 and int(rows[0]["tp"]) == 7 and int(rows[0]["valid"]) == int(rows[0]["target_valid"])
        xp, hv = rows_of(steer["fp16"])
        txp, th = rows_of(steer["fp16x3"])
        want = lc.rows_ref(xp, hv, txp, th)
        assert abs(float(rows[1]["dist"]) - want["dist"][0]) <= 2.0 ** -23 * want["dist"][0] + 1e-12 and rs["lines"] == 2
    finally:
        m.close()


# ---- 5. determinism
def test_two_runs_give_equal_records(lib):
    runs = []
    for _ in range(2):
        m = lib.Metric(max_frames=8)
        try:
            for shape in ((80, 160), (100, 260), (17, 33)):
                m.add_lanes_logits(*lc.general_case(shape)[:2])
            m.add_rows_raw(*lc.rows_general(8, 1000, 3))
            runs.append((m.fetch_lanes()[0].tobytes(), m.fetch_rows()[0].tobytes()))
        finally:
            m.close()
    assert runs[0] == runs[1]


# ---- 6. refusals
def test_refusals_with_engines(lib, engines, steer, state_dicts, frames, steer_frames):
    from autoware_vision_pilot_amd import weights as vw

    ego, seg, st = engines("egolanes", "fp16"), engines("sceneseg", "fp16"), steer["fp16"]
    for e in (ego, seg):
        e.infer(frames[0])
    st.infer(steer_frames[0])
    fresh = lib.Engine("egolanes", vw.pack_state_dict(state_dicts("egolanes")), precision="fp16")
    m = lib.Metric(max_frames=4)
    try:
        bits = lane_truth(ego, 1)
        txp, th = row_targets(2)
        with pytest.raises(ValueError, match="VP_SCENESEG and VP_DOMAINSEG engines only"):      # as before this entry existed
            m.add_seg(ego, bits)
        for bad in (lambda: m.add_lanes(seg, np.zeros(seg.output_dims()[-2:], np.uint8)), lambda: m.add_lanes(st, np.zeros((64, 1), np.uint8)),
                    lambda: m.add_lanes_pair(ego, seg), lambda: m.add_lanes_pair(seg, ego), lambda: m.add_lanes(ego, bits, 3), lambda: m.add_rows(ego, txp, th),
                    lambda: m.add_rows(seg, txp, th), lambda: m.add_rows_pair(st, ego), lambda: m.add_rows_pair(ego, st), lambda: m.add_rows(st, txp, th, thr=[])):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(lib.VpError, match="Inference has not been run yet"):
            m.add_lanes(fresh, bits)
        with pytest.raises(lib.VpError, match="Inference has not been run yet"):
            m.add_lanes_pair(ego, fresh)
        assert m.lanes_frames() == 0 and m.rows_lines() == 0 and m.frames() == 0
        m.add_rows(st, txp, th)
        with pytest.raises(ValueError, match="another threshold table"):
            m.add_rows(st, txp, th, thr=[0.02, 0.05])
        with pytest.raises(ValueError, match="another threshold table"):
            m.add_rows_pair(st, st, thr=[0.03, 0.05, 0.10])
        assert m.rows_lines() == 1
        if torch.cuda.device_count() > 1:                                     # a metric on another GPU than the engines
            other = lib.Metric(gpu_id=1, max_frames=2)
            try:
                for bad in (lambda: other.add_lanes(ego, bits), lambda: other.add_rows(st, txp, th)):
                    with pytest.raises(ValueError, match="lives on GPU"):
                        bad()
            finally:
                other.close()
    finally:
        m.close()
        fresh.close()
