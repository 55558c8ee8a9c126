"""vp_metric on the MI355X: the cases of tests/metric_cases.py on the device (select, segmentation counts, depth exact and general, the reference's NaN
answers, the accumulator), and the engine entries: engine path against operator path, the ordering against queued passes, the pair forms, the refusals."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- first: one shared HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import metric_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib as _lib

    return _lib


@pytest.fixture(scope="module")
def frames():
    from oracle import pre_post

    return [pre_post.synthetic_frame(360, 640, s) for s in (21, 22, 23)]


@pytest.fixture(scope="module")
def heads(lib, state_dicts):
    """fp16: a SceneSeg base with a Scene3D and a DomainSeg head on its encoder"""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    sd_seg = state_dicts("sceneseg")
    sd_3d = synthetic.share_backbone(dict(state_dicts("scene3d")), "scene3d", sd_seg, "sceneseg")
    sd_dom = synthetic.share_backbone(dict(state_dicts("domainseg")), "domainseg", sd_seg, "sceneseg", also_context_neck=True)
    base = lib.Engine("sceneseg", vw.pack_state_dict(sd_seg), precision="fp16")
    out = {"base": base, "scene3d": lib.Engine("scene3d", vw.pack_state_dict(sd_3d), precision="fp16", base=base),
           "domainseg": lib.Engine("domainseg", vw.pack_state_dict(sd_dom), precision="fp16", base=base)}
    yield out
    for k in ("scene3d", "domainseg", "base"):
        out[k].close()


def truth_for(engine, seed, depth=False):
    h, w = engine.output_dims()[-2:]
    rng = np.random.default_rng(seed)
    if depth:
        return (rng.random((h, w)) * 30.0 + 1.0).astype(np.float32)
    return rng.integers(0, 5, (h, w)).astype(np.uint8)


def same_records(a, b):
    return a.tobytes() == b.tobytes()


# ---- 1. the shared cases
@pytest.mark.parametrize("n", mc.SELECT_SIZES)
def test_select_bit_for_bit(lib, n):
    mc.check_select(lib, n)


def test_select_refusals(lib):
    mc.check_select_refusals(lib)


@pytest.mark.parametrize("shape", mc.SEG_SHAPES, ids=["x".join(map(str, s)) for s in mc.SEG_SHAPES])
def test_seg_counts_bit_for_bit(lib, shape):
    mc.check_seg(lib, shape)


def test_seg_absent_class_scores_one(lib):
    mc.check_seg_absent_class(lib)


@pytest.mark.parametrize("shape", tuple(mc.EXACT_SEEDS), ids=["x".join(map(str, s)) for s in mc.EXACT_SEEDS])
def test_depth_exact(lib, shape):
    mc.check_depth_exact(lib, shape)


@pytest.mark.parametrize("shape", mc.GENERAL_SHAPES, ids=["x".join(map(str, s)) for s in mc.GENERAL_SHAPES])
def test_depth_general(lib, shape):
    mc.check_depth_general(lib, shape)


def test_depth_nan_answers(lib):
    mc.check_depth_nan_answers(lib)


def test_accumulator(lib):
    mc.check_accumulator(lib, lib.VpError)


def test_refusals_without_an_engine(lib):
    mc.check_refusals(lib)


# ---- 2. the engine path equals the operator path
def test_add_seg_equals_add_seg_logits(lib, engines, heads, frames):
    """a stand-alone SceneSeg and DomainSeg engine and a DomainSeg head: the record from the device-resident logits equals the operator entry's on the
    logits fetched from that pass, in both ground-truth forms"""
    m = lib.Metric(max_frames=16)
    try:
        heads["base"].infer(frames[0])
        heads["domainseg"].infer_shared()
        for eng in (engines("sceneseg", "fp16"), engines("domainseg", "fp16"), heads["base"], heads["domainseg"]):
            if eng not in heads.values():
                eng.infer(frames[0])
            lg = eng.logits()
            for form in ("label", "bits"):
                gt = truth_for(eng, 5) if form == "label" else (truth_for(eng, 6).astype(np.int64) * 37 % 256).astype(np.uint8)
                m.reset()
                m.add_seg(eng, gt, form)
                m.add_seg_logits(lg, gt, form)
                rec, _ = m.fetch()
                assert same_records(rec[0:1], rec[1:2])
                mc.assert_seg_record(rec[0], mc.expected_seg_record(lg, gt, form))
                assert rec[0]["P"].sum() > 0
    finally:
        m.close()


def test_add_depth_equals_add_depth_plane(lib, engines, heads, frames):
    m = lib.Metric(max_frames=4)
    try:
        heads["base"].infer(frames[1])
        heads["scene3d"].infer_shared()
        alone = engines("scene3d", "fp16")
        alone.infer(frames[1])
        for eng in (alone, heads["scene3d"]):
            lg = eng.logits()
            gt = truth_for(eng, 7, depth=True)
            m.reset()
            m.add_depth(eng, gt)
            m.add_depth_plane(lg[0], gt)
            rec, _ = m.fetch()
            assert same_records(rec[0:1], rec[1:2])
            assert rec[0]["kind"] == mc.VP_SCENE3D and np.isfinite(rec[0]["mae"]) and np.isfinite(rec[0]["mel"]) and rec[0]["kept"] > 0
    finally:
        m.close()


# ---- 3. ordering without host waits
def test_adds_are_ordered_against_queued_passes(lib, engines, frames):
    """three passes on different frames, each followed by an add, nothing synchronised in between, ONE fetch: each record is what the operator entry
    gives for that frame's logits, fetched separately"""
    seg, s3d = engines("sceneseg", "fp16"), engines("scene3d", "fp16")
    m = lib.Metric(max_frames=16)
    fr = [lib.Frame() for _ in frames]
    try:
        for f, img in zip(fr, frames):
            f.upload(img, "bgr8")
        gts = [truth_for(seg, 30 + i) for i in range(3)]
        gds = [truth_for(s3d, 40 + i, depth=True) for i in range(3)]
        for i, f in enumerate(fr):             # the stand-alone passes (they also take the engines past their eager first pass)
            seg.infer_frame(f)
            s3d.infer_frame(f)
            m.add_seg_logits(seg.logits(), gts[i])
            m.add_depth_plane(s3d.logits()[0], gds[i])
        want, _ = m.fetch()
        assert not same_records(want[0:1], want[2:3]) and not same_records(want[1:2], want[3:4])
        m.reset()
        for i, f in enumerate(fr):
            seg.upload_from_frame(f)
            seg.enqueue()
            m.add_seg(seg, gts[i])
            s3d.upload_from_frame(f)
            s3d.enqueue()
            m.add_depth(s3d, gds[i])
        got, _ = m.fetch()
        assert same_records(got, want)
        seg.fetch_outputs()
        s3d.fetch_outputs()
    finally:
        m.close()
        for f in fr:
            f.close()


# ---- 4. the pair forms
def test_pair_forms(lib, engines, frames):
    seg, segx3, s3d = engines("sceneseg", "fp16"), engines("sceneseg", "fp16x3"), engines("scene3d", "fp16")
    m = lib.Metric(max_frames=8)
    try:
        for e in (seg, segx3, s3d):
            e.infer(frames[2])
        m.add_seg_pair(seg, seg)
        m.add_depth_pair(s3d, s3d)
        m.add_seg_pair(seg, segx3)
        label = mc.predict(segx3.logits()).astype(np.uint8)          # fp16x3's own prediction as the label map (3: no class)
        m.add_seg_logits(seg.logits(), label, "label")
        rec, s = m.fetch()
        assert rec[0]["I"].tolist() == rec[0]["P"].tolist() == rec[0]["G"].tolist() and rec[0]["P"].sum() == rec[0]["n"]
        assert mc.seg_scores(rec[0]["I"].tolist(), rec[0]["P"].tolist(), rec[0]["G"].tolist()) == ([1.0, 1.0, 1.0], 1.0)
        assert np.isnan(rec[1]["mae"]) and rec[1]["mel"] == 0.0 and rec[1]["kept"] == 0
        assert same_records(rec[2:3], rec[3:4])
        assert rec[2]["I"].sum() > 0.9 * rec[2]["n"]                 # the two precisions agree on most pixels
        assert s["nan_frames"] == 1 and s["sceneseg_frames"] == 3
    finally:
        m.close()


# ---- 5. refusals
def test_refusals_with_engines(lib, engines, state_dicts, frames):
    from autoware_vision_pilot_amd import weights as vw

    seg, dom, s3d = engines("sceneseg", "fp16"), engines("domainseg", "fp16"), engines("scene3d", "fp16")
    for e in (seg, dom, s3d):
        e.infer(frames[0])
    fresh = lib.Engine("sceneseg", vw.pack_state_dict(state_dicts("sceneseg")), precision="fp16")
    m = lib.Metric(max_frames=4)
    try:
        gt, gd = truth_for(seg, 1), truth_for(s3d, 2, depth=True)
        for bad in (lambda: m.add_seg(s3d, gt), lambda: m.add_depth(seg, gd), lambda: m.add_depth(dom, gd), lambda: m.add_seg_pair(seg, dom),
                    lambda: m.add_seg_pair(seg, s3d), lambda: m.add_depth_pair(s3d, seg), lambda: m.add_seg(seg, gt, 2)):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(lib.VpError, match="Inference has not been run yet"):
            m.add_seg(fresh, gt)
        with pytest.raises(lib.VpError, match="Inference has not been run yet"):
            m.add_seg_pair(seg, fresh)
        assert m.frames() == 0
    finally:
        m.close()
        fresh.close()
