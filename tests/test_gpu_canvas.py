"""vp_canvas on the MI355X: one picture per camera frame, drawn into on the device by every engine (heads included) and the detector, fetched once in any
vp_frame format.  Cases and numpy restatements: tests/canvas_cases.py.  Masks and depth are checked bit for bit against the existing calls
(vp_visualize_mask_bgr8, vp_visualize_depth_bgr8) or against their arithmetic applied to vp_mask_u8; boxes and the forward YUV form against the two
definitions include/vp_hip.h states."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import canvas_cases as cc  # noqa: E402
from oracle import weights  # noqa: E402

pytestmark = pytest.mark.gpu
H, W = 720, 1280
LANES = (0, 420, 1280, 300)     # the production app's EgoLanes crop: rows >= 420 (main.cpp:497-505)


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib as _lib

    return _lib


@pytest.fixture(scope="module")
def nets(lib, state_dicts):
    """fp16: a SceneSeg base with Scene3D and DomainSeg heads, and a stand-alone EgoLanes engine decoding lane labels"""
    from autoware_vision_pilot_amd import weights as vw

    sd_seg = state_dicts("sceneseg")
    sd_3d = weights.share_backbone(dict(state_dicts("scene3d")), "scene3d", sd_seg, "sceneseg")
    sd_dom = weights.share_backbone(dict(state_dicts("domainseg")), "domainseg", sd_seg, "sceneseg", also_context_neck=True)
    base = lib.Engine("sceneseg", vw.pack_state_dict(sd_seg), precision="fp16")
    out = {"base": base, "scene3d": lib.Engine("scene3d", vw.pack_state_dict(sd_3d), precision="fp16", base=base),
           "domainseg": lib.Engine("domainseg", vw.pack_state_dict(sd_dom), precision="fp16", base=base),
           "egolanes": lib.Engine("egolanes", vw.pack_state_dict(state_dicts("egolanes")), precision="fp16")}
    out["egolanes"].set_decode_mode(lib.VP_DECODE_LANE_LABEL)
    yield out
    for k in ("scene3d", "domainseg", "egolanes", "base"):
        out[k].close()


@pytest.fixture(scope="module")
def detector(lib):
    from autoware_vision_pilot_amd import synthetic, weights as vw

    eng = lib.Engine("autospeed", vw.pack_state_dict(synthetic.make_autospeed_state_dict(0)), precision="fp16")
    det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
    det.attach(eng)
    yield eng, det
    det.close()
    eng.close()


# ---- 1. kernel shapes through the operator entry, the boxes and the fetch
@pytest.mark.parametrize("hw,mhw,region,viz", cc.BLEND_CASES, ids=["%dx%d-%dx%d-%d.%d.%d.%d-%d" % (c[0] + c[1] + c[2] + (c[3],)) for c in cc.BLEND_CASES])
def test_blend_mask_u8_bit_for_bit(lib, hw, mhw, region, viz):
    cc.check_blend(lib, hw, mhw, region, viz)


def test_blend_mask_u8_from_device_memory_and_more_than_one_workgroup(lib):
    """a device-resident mask (torch), and a region wider than one workgroup's 1024 pixels"""
    import torch

    bgr, mask = cc.random_bgr(9, 2307, 2), cc.random_mask(5, 700, 3)
    region = (3, 1, 2301, 7)
    dmask = torch.from_numpy(mask).cuda()
    torch.cuda.synchronize()
    with cc.OnCanvas(lib, bgr) as oc:
        oc.canvas.blend_mask_u8(dmask.data_ptr(), 1, region, device_hw=mask.shape)
        assert np.array_equal(oc.canvas.fetch("bgr8"), cc.blend_region(bgr, mask, 1, region))


@pytest.mark.parametrize("hw", cc.CANVAS_SIZES, ids=["%dx%d" % s for s in cc.CANVAS_SIZES])
def test_boxes_bit_for_bit(lib, hw):
    cc.check_boxes(lib, hw)


@pytest.mark.parametrize("fmt", cc.FORMATS)
def test_fetch_bit_for_bit(lib, fmt):
    for hw in cc.FETCH_SIZES.get(fmt, cc.CANVAS_SIZES):
        cc.check_fetch(lib, fmt, hw)


def test_refusals_without_an_engine(lib):
    cc.check_canvas_refusals(lib)


# ---- 2. engines: exact against the existing calls
def test_base_on_a_whole_frame_equals_visualize_mask(lib, nets):
    cc.check_engine_region(lib, nets["base"], lib.VP_VIZ_SCENE, (90, 160), None)


def test_base_on_an_odd_region_of_a_larger_frame(lib, nets):
    cc.check_engine_region(lib, nets["base"], lib.VP_VIZ_SCENE, (97, 171), (5, 7, 141, 79))


@pytest.mark.parametrize("region", [None, (5, 7, 141, 79)], ids=["whole", "odd-region"])
def test_heads_draw_where_their_base_took_its_input(lib, nets, region):
    """what vp_visualize_mask_bgr8 refuses: Scene3D and DomainSeg heads.  Masks against the blend's restatement applied to vp_mask_u8, the depth map against
    vp_visualize_depth_bgr8 at the region's size, two overlays stacked in both orders against the sequential restatement."""
    base, s3d, dom = nets["base"], nets["scene3d"], nets["domainseg"]
    bgr = cc.random_bgr(97, 171, 8)
    r = region if region is not None else (0, 0, 171, 97)
    with cc.OnCanvas(lib, bgr) as oc:
        c, f = oc.canvas, oc.frame
        base.infer_frame(f, region)
        s3d.infer_shared()
        dom.infer_shared()
        with pytest.raises(lib.VpError, match="base engine"):
            dom.visualize_mask(lib.VP_VIZ_DOMAIN, (r[3], r[2]))          # the existing call has no picture for a head
        m_base, m_3d, m_dom = base.mask().copy(), s3d.mask().copy(), dom.mask().copy()
        depth = s3d.visualize_depth(r[3], r[2])
        for eng, mask, viz in ((s3d, m_3d, lib.VP_VIZ_SCENE), (dom, m_dom, lib.VP_VIZ_DOMAIN)):
            c.begin(f)
            c.blend_mask(eng, viz)
            assert np.array_equal(c.fetch("bgr8"), cc.blend_region(bgr, mask, viz, r)), viz
        c.begin(f)
        c.paste_depth(s3d)
        pasted = c.fetch("bgr8")
        assert np.array_equal(pasted, cc.paste_region(bgr, depth, r))
        c.blend_mask(dom, lib.VP_VIZ_DOMAIN)                              # a mask over the depth map ...
        assert np.array_equal(c.fetch("bgr8"), cc.blend_region(pasted, m_dom, lib.VP_VIZ_DOMAIN, r))
        c.begin(f)                                                        # ... and two masks in both orders
        c.blend_mask(base, lib.VP_VIZ_SCENE)
        c.blend_mask(dom, lib.VP_VIZ_DOMAIN)
        ab = c.fetch("bgr8")
        c.begin(f)
        c.blend_mask(dom, lib.VP_VIZ_DOMAIN)
        c.blend_mask(base, lib.VP_VIZ_SCENE)
        ba = c.fetch("bgr8")
        assert np.array_equal(ab, cc.blend_region(cc.blend_region(bgr, m_base, 0, r), m_dom, 1, r))
        assert np.array_equal(ba, cc.blend_region(cc.blend_region(bgr, m_dom, 1, r), m_base, 0, r))
        assert not np.array_equal(ab, ba)
        c.begin(f)
        c.blend_mask(base, lib.VP_VIZ_SCENE)
        c.paste_depth(s3d)                                                # opaque: the mask under it is gone
        assert np.array_equal(c.fetch("bgr8"), pasted)


def test_lanes_on_their_crop_and_boxes_on_the_full_frame_fetched_as_nv12(lib, nets, detector):
    """the production app's two consumers of one camera frame (EgoLanes on rows >= 420 with VP_DECODE_LANE_LABEL, AutoSpeed on the full frame) on ONE canvas,
    handed back as NV12 and as BGR8"""
    from autoware_vision_pilot_amd import synthetic

    ego, (_, det) = nets["egolanes"], detector
    bgr = synthetic.synthetic_frame(H, W, 17)
    with cc.OnCanvas(lib, bgr) as oc:
        c, f = oc.canvas, oc.frame
        ego.infer_frame(f, LANES)
        rows, _ = det.infer_frame(f, 0.05, 0.45)
        rows = np.concatenate([rows[:70], np.array([cc.det(100.4, 50.2, 400.9, 300.1, 1), cc.det(-20, 400, 300.5, 900, 2), cc.det(900, 410, 1279.9, 719.9, 3)], np.float32)])
        want_lanes = ego.visualize_mask(lib.VP_VIZ_EGOLANES, (LANES[3], LANES[2]))
        c.blend_mask(ego, lib.VP_VIZ_EGOLANES)
        c.draw_detections(rows)
        want = cc.draw_boxes(cc.paste_region(bgr, want_lanes, LANES), rows)
        assert np.array_equal(want[:LANES[1]], cc.draw_boxes(bgr, rows)[:LANES[1]])      # above the crop: the frame and the boxes only
        y, uv = c.fetch("nv12")
        wy, wuv = cc.from_bgr("nv12", want)
        assert np.array_equal(y, wy) and np.array_equal(uv, wuv)
        assert np.array_equal(c.fetch("bgr8"), want)


# ---- 3. ordering without host waits
def test_a_draw_is_ordered_against_the_engine_on_the_device(lib, nets):
    """infer A; blend; infer B; fetch -- nothing synchronised in between: the picture shows A's mask, and the engine ends up with B's"""
    base = nets["base"]
    A, B = (cc.random_bgr(H, W, s) for s in (41, 42))
    fa, fb, c = lib.Frame(), lib.Frame(), lib.Canvas()
    try:
        fa.upload(A, "bgr8")
        fb.upload(B, "bgr8")
        masks = []
        for f in (fa, fb):       # the stand-alone passes; they also take the engine past its eager first pass and the canvas past its first table upload
            base.infer_frame(f)
            masks.append(base.mask().copy())
            c.begin(f)
            c.blend_mask(base, lib.VP_VIZ_SCENE)
        c.sync()
        assert not np.array_equal(masks[0], masks[1])
        base.upload_from_frame(fa)
        base.enqueue()
        c.begin(fa)
        c.blend_mask(base, lib.VP_VIZ_SCENE)
        base.upload_from_frame(fb)
        base.enqueue()
        got = c.fetch("bgr8")
        assert np.array_equal(got, cc.blend_region(A, masks[0], 0, (0, 0, W, H)))
        base.fetch_outputs()
        assert np.array_equal(base.mask(), masks[1])
    finally:
        c.close()
        fa.close()
        fb.close()


def test_begin_counts_as_a_consumer_of_the_frame(lib):
    """begin; vp_frame_upload(other content); fetch -- the canvas holds the first picture"""
    A, B = (cc.random_bgr(H, W, s) for s in (43, 44))
    f, c = lib.Frame(), lib.Canvas()
    try:
        for _ in range(2):       # the second round runs with every buffer in place
            f.upload(A, "bgr8")
            c.begin(f)
            f.upload(B, "bgr8")
            assert np.array_equal(c.fetch("bgr8"), A)
            assert np.array_equal(f.fetch_bgr8(), B)
    finally:
        c.close()
        f.close()


# ---- 4. refusals that need an engine
def test_engine_refusals(lib, nets, detector, state_dicts):
    from autoware_vision_pilot_amd import synthetic, weights as vw

    ego = nets["egolanes"]
    bgr = cc.random_bgr(64, 96, 5)
    with cc.OnCanvas(lib, bgr) as oc:
        c, f = oc.canvas, oc.frame
        for kind, eng in (("autospeed", detector[0]), ("autodrive", lib.Engine("autodrive", vw.pack_state_dict(synthetic.make_autodrive_state_dict(0)), precision="fp16")),
                          ("autosteer", lib.Engine("autosteer", vw.pack_state_dict(synthetic.make_autosteer_state_dict(0)), precision="fp16"))):
            try:
                for draw in (lambda: c.blend_mask(eng, 0), lambda: c.paste_depth(eng)):
                    with pytest.raises(ValueError, match="no mask or depth plane"):
                        draw()
            finally:
                if kind != "autospeed":
                    eng.close()
        enc = lib.Engine("sceneseg", vw.pack_state_dict(state_dicts("sceneseg")), precision="fp16", frames=2)
        fresh = lib.Engine("egolanes", vw.pack_state_dict(state_dicts("egolanes")), precision="fp16")
        try:
            with pytest.raises(ValueError, match="batched encoder"):
                c.blend_mask(enc, 0)
            for draw in (lambda: c.blend_mask(fresh, 2), lambda: c.paste_depth(fresh)):
                with pytest.raises(lib.VpError, match="Inference has not been run yet"):
                    draw()
        finally:
            enc.close()
            fresh.close()
        ego.infer(bgr)                                   # a host frame records the whole frame: 96 x 64 here
        c.blend_mask(ego, lib.VP_VIZ_EGOLANES)
        assert np.array_equal(c.fetch("bgr8"), ego.visualize_mask(lib.VP_VIZ_EGOLANES, (64, 96)))
        with pytest.raises(ValueError, match="viz_type"):
            c.blend_mask(ego, 3)
        ego.infer(cc.random_bgr(64, 98, 6))
        for draw in (lambda: c.blend_mask(ego, 2), lambda: c.paste_depth(ego)):
            with pytest.raises(ValueError, match="98 x 64 frame.*96 x 64 picture"):
                draw()
        ego.infer_tensor(np.zeros((3, 320, 640), np.float32))
        with pytest.raises(ValueError, match="tensor"):
            c.blend_mask(ego, 2)
        ego.infer_frame(f)                               # and a frame makes it drawable again
        c.begin(f)
        c.blend_mask(ego, lib.VP_VIZ_EGOLANES)
        assert np.array_equal(c.fetch("bgr8"), ego.visualize_mask(lib.VP_VIZ_EGOLANES, (64, 96)))
