"""vp_metric's label part on the MI355X: the cases of tests/label_cases.py through the label kernels, bit for bit against the numpy reference; the fused
operator forms against add_seg_logits / add_depth_plane fed host-prepared ground truth; the engine entries against add_seg / add_depth; order, reset and
the refusals."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- first: one shared HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import label_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib as _lib

    return _lib


@pytest.fixture(scope="module")
def frame():
    from oracle import pre_post

    return pre_post.synthetic_frame(360, 640, 31)


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


# ---- 1. the label kernels
@pytest.mark.parametrize("name", lc.COLOUR_CASES)
def test_colour_labels_bit_for_bit(lib, name):
    want = lc.check_colour(lib, name)
    if name == "nine_colours":
        assert want["unmatched"] > 0 and min(want["freq"]) > 0
    if name in ("padded_rows", "wide_crop", "negative_box"):
        assert want["outside"] > 0
    if name == "padded_rows":
        assert want["outside"] == 10 * 63


@pytest.mark.parametrize("name", lc.MASK_CASES)
def test_mask_labels_bit_for_bit(lib, name):
    want = lc.check_mask(lib, name)
    assert want["freq"][0] > 0 and want["freq"][1:] == (0, 0)


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=("f32", "f64"))
@pytest.mark.parametrize("name", lc.DEPTH_CASES)
def test_depth_labels_bit_for_bit(lib, name, dtype):
    gt, want = lc.check_depth(lib, name, dtype)
    if name in ("constant", "one_nan"):
        assert np.isnan(gt).all()
    if name == "one_nan":
        assert want["nonfinite"] == 1 and np.isnan(want["min"])
    if name == "one_inf":
        assert want["nonfinite"] == 1 and want["max"] == np.inf
    if name == "negative_and_zero":
        assert want["min"] < 0 < want["max"] and np.isfinite(gt).all()


# ---- 2. the fused path
def test_fused_records_equal_host_prepared_ground_truth(lib):
    lc.check_fused(lib)


def test_three_adds_from_one_overwritten_host_buffer(lib):
    lc.check_one_buffer(lib)


# ---- 3. the engines
def test_engine_entries_equal_add_seg_and_add_depth(lib, heads, frame):
    """add_seg_label on SceneSeg and DomainSeg, add_depth_label on Scene3D: the vp_metric_frame is that of add_seg / add_depth with the reference's ground truth"""
    m = lib.Metric(max_frames=16)
    try:
        heads["base"].infer(frame)
        heads["domainseg"].infer_shared()
        heads["scene3d"].infer_shared()
        out_hw = tuple(heads["base"].output_dims()[-2:])
        wants = []
        img = lc.palette_image(257, 515, 32)
        for crop in (None, (0, 0, 514, 180), (0, 100, 515, 300)):
            want_gt, want = lc.seg_ref(img, out_hw, crop)
            m.add_seg_label(heads["base"], img, crop=crop)
            m.add_seg(heads["base"], want_gt, "label")
            wants.append(want)
        mask = lc.mask_case("large")[0]
        want_gt, want = lc.seg_ref(mask, out_hw)
        m.add_seg_label(heads["domainseg"], mask)
        m.add_seg(heads["domainseg"], want_gt, "label")
        wants.append(want)
        for dtype in (np.float32, np.float64):
            v = lc.depth_case("large", dtype)
            want_gt, want = lc.depth_ref(v, out_hw)
            m.add_depth_label(heads["scene3d"], v)
            m.add_depth(heads["scene3d"], want_gt)
            wants.append(want)
        rec, summary = m.fetch()
        assert len(rec) == 12 and summary["nan_frames"] == 0
        for k in range(0, 12, 2):
            assert rec[k:k + 1].tobytes() == rec[k + 1:k + 2].tobytes(), k
        assert rec[0]["P"].sum() > 0 and rec[0]["G"].sum() > 0 and rec[6]["G"][0] > 0 and rec[8]["kept"] > 0
        labels = m.fetch_labels()
        assert [int(r["kind"]) for r in labels] == [lc.VP_SCENESEG] * 3 + [lc.VP_DOMAINSEG] + [lc.VP_SCENE3D] * 2
        for got, want in zip(labels, wants):
            lc.assert_record(got, want)
        # the engine refusals: another kind, and no record added
        for bad in (lambda: m.add_seg_label(heads["scene3d"], img), lambda: m.add_depth_label(heads["base"], lc.depth_case("random", np.float32)),
                    lambda: m.add_seg_label(heads["base"], img, crop=(4, 4, 4, 9)), lambda: m.add_depth_label(heads["scene3d"], np.zeros((4, 4), np.float32)[:, :0])):
            with pytest.raises(ValueError):
                bad()
        assert m.frames() == 12 and m.label_frames() == 6
    finally:
        m.close()


def test_engine_without_a_pass_is_a_state_error(lib, state_dicts):
    from autoware_vision_pilot_amd import weights as vw

    fresh = lib.Engine("sceneseg", vw.pack_state_dict(state_dicts("sceneseg")), precision="fp16")
    m = lib.Metric(max_frames=2)
    try:
        with pytest.raises(lib.VpError, match="not been run"):
            m.add_seg_label(fresh, lc.palette_image(12, 20, 33))
        assert m.frames() == 0 and m.label_frames() == 0
    finally:
        m.close()
        fresh.close()


# ---- 4. order, reset, refusals
def test_fetch_labels_order_and_reset(lib):
    m = lib.Metric(max_frames=8)
    try:
        lg = lc.random_logits(3, (16, 24), 34)
        names = ("enlarge", "shrink", "dropped_column", "padded_rows")
        for name in names:
            img, crop, colours, _ = lc.colour_case(name)
            m.add_seg_logits_label(lg, img, crop=crop, colours=colours)
        labels = m.fetch_labels()
        assert [int(r["n"]) for r in labels] == [5 * 7, 37 * 53, 20 * 33, 40 * 63]
        for got, name in zip(labels, names):
            img, crop, colours, out_hw = lc.colour_case(name)
            lc.assert_record(got, lc.seg_ref(img, out_hw, crop, colours)[1])
        assert len(m.fetch()[0]) == 4     # the metric records do not hold the label records, and the other way round
        m.reset()
        assert m.label_frames() == 0 and m.frames() == 0 and len(m.fetch_labels()) == 0
        m.add_depth_plane_label(np.zeros((16, 24), np.float32), lc.depth_case("random", np.float32))
        labels = m.fetch_labels()
        assert len(labels) == 1 and int(labels[0]["kind"]) == lc.VP_SCENE3D
    finally:
        m.close()


def test_refusals(lib):
    lc.check_refusals(lib)
