"""SURVEY.md N4 on the MI355X: the AutoSpeed detector network as an engine of this library (VP_AUTOSPEED) and the one-call form vp_detect_attach +
vp_detect_infer (frame in, detections out).  References: tests/autospeed_net_ref.py (torch CPU fp32 restatement) and tests/golden/autospeed_net.npz,
the outputs of the reference's own nn.Module on the same weights and frames; oracle/autospeed.py for decode + NMS."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import autospeed_net_ref as ref  # noqa: E402
from oracle import autospeed  # noqa: E402

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(HERE, "golden", "autospeed_net.npz"))
CONF, IOU = float(G["conf"]), float(G["iou"])
FRAMES = [(720, 1280, 21), (1080, 1920, 25), (487, 301, 31), (641, 1283, 32)]     # the first two are the fixture's (condition) frames


def _rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def _frame(h, w, seed):
    from autoware_vision_pilot_amd import synthetic

    return synthetic.synthetic_frame(h, w, seed)


@pytest.fixture(scope="module")
def sd():
    from autoware_vision_pilot_amd import synthetic

    return synthetic.make_autospeed_state_dict(int(G["weight_seed"]))


def _pair(sd, precision):
    from autoware_vision_pilot_amd import lib, weights as vw

    eng = lib.Engine("autospeed", vw.pack_state_dict(sd), precision=precision)
    det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
    det.attach(eng)
    return eng, det


@pytest.fixture(scope="module")
def x3(sd):
    eng, det = _pair(sd, "fp16x3")
    yield eng, det
    det.close()
    eng.close()


def test_raw_against_restatement_and_reference_module(x3, sd):
    eng, det = x3
    assert tuple(G["frames"][0]) == FRAMES[0] and tuple(G["frames"][1]) == FRAMES[1]
    for fi, (h, w, seed) in enumerate(FRAMES):
        f = _frame(h, w, seed)
        det.infer(f, CONF, IOU)
        got = eng.logits().reshape(8, 10752).copy()
        x, _ = autospeed.preprocess(f, 512, 1024)
        want, _ = ref.forward(sd, x)
        err = _rel(got, want)
        print(f"frame {h}x{w}: raw against the restatement {err:.2e}")
        assert err <= 1e-3
        if fi < 2:
            e2 = _rel(got[:, ::int(G["box_step"])], G[f"raw_{fi}"])
            print(f"frame {h}x{w}: raw against the reference module's vectors {e2:.2e}")
            assert e2 <= 1e-3


def test_graph_replay_is_bit_stable_and_tensor_entry_gives_the_same_bits(x3):
    eng, det = x3
    f = _frame(*FRAMES[0])
    runs = []
    for _ in range(3):
        d, n = det.infer(f, CONF, IOU)
        runs.append((eng.logits().copy(), d.copy(), n))
    for r in runs[1:]:
        assert np.array_equal(r[0].view(np.uint32), runs[0][0].view(np.uint32)) and np.array_equal(r[1].view(np.uint32), runs[0][1].view(np.uint32)) and r[2] == runs[0][2]
    x, _ = det.preprocess(f)                    # the letterbox kernel's tensor on the host
    eng.infer_tensor(x)
    assert np.array_equal(eng.logits().view(np.uint32), runs[0][0].view(np.uint32))
    det.infer(f, CONF, IOU)                     # and back to the device-resident form
    assert np.array_equal(eng.logits().view(np.uint32), runs[0][0].view(np.uint32))


def test_detections_are_the_oracles_decode_of_the_engines_own_raw(x3):
    eng, det = x3
    for h, w, seed in FRAMES:
        got, n = det.infer(_frame(h, w, seed), CONF, IOU)
        raw = eng.logits().reshape(8, 10752)
        scale, px, py = det.letterbox()
        want = autospeed.postprocess(raw, CONF, IOU, scale, px, py, w, h)
        assert n == len(want) and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))          # kept set, order, every coordinate: bit for bit
        got3, n3 = det.infer(_frame(h, w, seed), CONF, IOU, cap=3)
        assert n3 == n and np.array_equal(got3.view(np.uint32), want[:3].view(np.uint32))


def test_detections_against_the_reference_modules(x3):
    """The fixture's frames were chosen (tools/pin_autospeed_net.py check_conditions) so that the reference's raw has 20 .. 2000 candidates, no class
    score within 2e-3 of the confidence threshold and no candidate pair with an IoU within 2e-3 of the IoU threshold: a 1e-3 engine keeps the same set."""
    eng, det = x3
    for fi in range(2):
        h, w, seed = FRAMES[fi]
        got, n = det.infer(_frame(h, w, seed), CONF, IOU)
        want = G[f"det_{fi}"]
        assert n == len(want) and got.shape == want.shape
        assert np.array_equal(got[:, 5], want[:, 5])
        err = _rel(got[:, :5], want[:, :5])
        print(f"frame {h}x{w}: {n} detections, coordinates / confidence against the reference's {err:.2e}")
        assert err <= 1e-3


def _same_kept_set(got, want, scale):
    """The fp16 engine's kept detections against the reference's, box by box.  Bounds from the fp16 raw bar above, not from measurement: a raw box row
    is within 3e-2 * 1024 letterbox pixels, a corner is cx -+ w / 2 (1.5 of that) divided by the letterbox scale; a confidence is within 3e-2.  Every
    reference detection has exactly one partner of its class inside those bounds; the order is by descending confidence, so it is the reference's
    order wherever two reference confidences are further apart than both errors together."""
    tol_xy, tol_c = 1.5 * 3e-2 * 1024.0 / scale, 3e-2
    assert np.all(np.diff(got[:, 4]) <= 0)
    match = []
    for r in want:
        d = np.abs(got[:, :4] - r[:4]).max(axis=1) + np.where(got[:, 5] == r[5], 0.0, np.inf)
        j = int(np.argmin(d))
        assert d[j] <= tol_xy and abs(got[j, 4] - r[4]) <= tol_c
        match.append(j)
    assert sorted(match) == list(range(len(got)))            # one to one
    inv = np.argsort(match)                                   # reference index of got[i]
    for i in range(len(got)):
        for j in range(i + 1, len(got)):
            if inv[i] > inv[j]:                               # swapped against the reference: only inside the confidence error
                assert want[inv[j], 4] - want[inv[i], 4] <= 2 * tol_c


def test_fp16_engine(sd):
    """VP_FP16 (non-parity): finite, the same kept set on the condition frames, raw in the project's fp16 regression form -- 3e-2 of the largest value,
    box rows relative to 1024, score rows relative to 1."""
    eng, det = _pair(sd, "fp16")
    try:
        for fi in range(2):
            h, w, seed = FRAMES[fi]
            f = _frame(h, w, seed)
            got, n = det.infer(f, CONF, IOU)
            raw = eng.logits().reshape(8, 10752)
            assert np.isfinite(raw).all()
            x, _ = autospeed.preprocess(f, 512, 1024)
            want, _ = ref.forward(sd, x)
            eb, es = float(np.abs(raw[:4] - want[:4]).max()) / 1024.0, float(np.abs(raw[4:] - want[4:]).max())
            print(f"fp16 frame {h}x{w}: box rows {eb:.2e} of 1024, score rows {es:.2e}; kept {n} (reference {len(G[f'det_{fi}'])})")
            assert eb <= 3e-2 and es <= 3e-2
            wd = G[f"det_{fi}"]
            assert n == len(wd) and np.array_equal(got[:, 5], wd[:, 5])
            _same_kept_set(got, wd, float(det.letterbox()[0]))
    finally:
        det.close()
        eng.close()


def test_attach_refusals(x3, sd):
    from autoware_vision_pilot_amd import lib, synthetic, weights as vw

    eng, _ = x3
    other = lib.Engine("autodrive", vw.pack_state_dict(synthetic.make_autodrive_state_dict(0)), precision="fp16")
    d = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
    try:
        with pytest.raises(ValueError, match="VP_AUTOSPEED"):
            d.attach(other)
        with pytest.raises(lib.VpError, match="vp_detect_attach"):
            d.infer(_frame(64, 64, 1), CONF, IOU)               # nothing attached
    finally:
        d.close()
        other.close()
    for args, pat in (((640, 640, 10752, 8), "640 x 640"), ((512, 1024, 8400, 8), "max_boxes >= 10752"), ((512, 1024, 10752, 7), "max_attrs >= 8")):
        d = lib.Detector(args[0], args[1], max_boxes=args[2], max_attrs=args[3])
        try:
            with pytest.raises(ValueError, match=pat):
                d.attach(eng)
        finally:
            d.close()
    with pytest.raises(ValueError, match="VP_WEIGHTS_FP8"):
        lib.Engine("autospeed", vw.pack_state_dict(sd), precision="fp16", weights_fp8=True)
    with pytest.raises(lib.VpError, match="vp_detect_infer"):
        eng.infer(_frame(720, 1280, 1))


def test_range_guard_covers_the_detector_output(sd):
    """A non-finite input tensor surfaces as VpRangeError from the synchronising call, as for every other engine."""
    from autoware_vision_pilot_amd import lib, weights as vw

    eng = lib.Engine("autospeed", vw.pack_state_dict(sd), precision="fp16x3")
    try:
        x = np.full((3, 512, 1024), 0.5, np.float32)
        eng.infer_tensor(x)
        x[1, 100, 100] = np.inf
        with pytest.raises(lib.VpRangeError):
            eng.infer_tensor(x)
        x[1, 100, 100] = 0.5
        eng.infer_tensor(x)
        assert np.isfinite(eng.logits()).all()
    finally:
        eng.close()


def test_range_guard_through_detect_infer(x3, sd):
    """vp_detect_infer's own VP_ERR_RANGE path (the probe's verdict fetched behind the graph, checked after the one synchronisation) and its mapping to
    VpRangeError in Detector.infer.  A frame is bytes, so the overflow has to come from the weights: the first level's box branch scaled so that its
    logits leave the fp16 range (every single weight stays inside it: the engine loads).  The handle is usable afterwards: with a sound engine attached
    it returns the bits the fixture's detector returns."""
    from autoware_vision_pilot_amd import lib, weights as vw

    bad = dict(sd)
    bad["head.box.0.1.norm.weight"] = sd["head.box.0.1.norm.weight"] * np.float32(1e3)
    bad["head.box.0.2.weight"] = sd["head.box.0.2.weight"] * np.float32(1e2)
    eng = lib.Engine("autospeed", vw.pack_state_dict(bad), precision="fp16x3")
    det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
    good_eng, good_det = x3
    f = _frame(*FRAMES[0])
    try:
        det.attach(eng)
        for _ in range(2):                                    # the eager first pass and the replayed graph; a failed call leaves the handle usable
            with pytest.raises(lib.VpRangeError, match="vp_detect_infer"):
                det.infer(f, CONF, IOU)
        det.attach(good_eng)
        got, n = det.infer(f, CONF, IOU)
        want, nw = good_det.infer(f, CONF, IOU)
        assert n == nw and n > 0 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    finally:
        det.close()
        eng.close()


def test_attach_none_detaches(x3):
    eng, det0 = x3
    f = _frame(*FRAMES[0])
    want, nw = det0.infer(f, CONF, IOU)
    from autoware_vision_pilot_amd import lib

    det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
    try:
        det.attach(eng)
        got, n = det.infer(f, CONF, IOU)
        assert n == nw and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        det.attach(None)
        with pytest.raises(lib.VpError, match="vp_detect_attach"):
            det.infer(f, CONF, IOU)
        x, _ = det.preprocess(f)                              # the two-call form does not need a network
        assert x.shape == (3, 512, 1024)
        det.attach(eng)
        got, n = det.infer(f, CONF, IOU)
        assert n == nw and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        with pytest.raises(lib.VpError, match="vp_detect_infer: bad frame geometry"):
            det.infer(np.zeros((0, 4, 3), np.uint8), CONF, IOU)
    finally:
        det.close()
