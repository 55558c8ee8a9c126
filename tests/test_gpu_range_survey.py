"""The range survey on the GPU (include/vp_hip.h "RANGE SURVEY"): act_exp_hist_kernel against numpy on the operator cases, vp_range_survey on whole
engines against the statistics of vp_tensor_read, an overflow that the survey locates where vp_infer only reports it, and the refusals.  Every comparison
is exact: the counters are integers and the abs-max is a maximum."""
import os

import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import range_hist_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = cases.operator_cases()
FULL_LIMIT = 1 << 22     # tensors up to this many elements are compared bin by bin; larger ones by the count / sum identities (plus the three largest of SceneSeg fp16x3)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_exp_hist_operator(case):
    from autoware_vision_pilot_amd import lib

    _, hi, lo, c = case
    cases.check_operator(lib, hi, lo, c)


def test_exp_hist_operator_grid_stride():
    """more octets than the launch has threads (1024 blocks x 256): every thread walks its grid-stride loop more than once"""
    from autoware_vision_pilot_amd import lib

    hi, lo = cases.planes(32, 32, 257, 257, True, 9)
    assert 257 * 257 * 4 > 1024 * 256
    cases.check_operator(lib, hi, lo, 32)


# ------------------------------------------------------------------------------------------------ whole engines
class _Runner:
    """an engine and how its fixture frame goes in: run() -> the output tensor of one plain pass"""

    def __init__(self, lib, kind, precision, state_dicts, frame720, **kw):
        from autoware_vision_pilot_amd import synthetic, weights as vw

        self.det = None
        if kind in ("sceneseg", "scene3d", "domainseg", "egolanes"):
            self.eng = lib.Engine(kind, vw.pack_state_dict(state_dicts(kind)), precision=precision)
            self.run = lambda: self._infer(frame720)
        elif kind == "autodrive":
            g = np.load(os.path.join(HERE, "golden", "autodrive.npz"))
            f0, f1 = (synthetic.synthetic_frame(1080, 1920, int(s)) for s in g["frame_seeds"][:2])
            self.eng = lib.Engine(kind, vw.pack_state_dict(synthetic.make_autodrive_state_dict(int(g["weight_seed"]))), precision=precision)
            self.eng.infer_pair(f0, f1)
            self.run = lambda: self._infer(f1)     # the stream continues: every later pass pairs f1 with f1
        elif kind == "autosteer":
            g = np.load(os.path.join(HERE, "golden", "act_scale_nets.npz"))
            h, w, seed = (int(v) for v in g["autosteer_frame"])
            frame = synthetic.synthetic_frame(h, w, seed)
            self.eng = lib.Engine(kind, vw.pack_state_dict(synthetic.make_autosteer_state_dict(int(g["weight_seed"]))), precision=precision, **kw)
            self.eng.set_input_format(lib.VP_BGR8, lib.VP_PLANES_RGB)
            self.run = lambda: self._infer(frame)
        else:
            g = np.load(os.path.join(HERE, "golden", "act_scale_nets.npz"))
            gold = np.load(os.path.join(HERE, "golden", "autospeed_net.npz"))
            h, w, seed = (int(v) for v in g["autospeed_frame"])
            frame = synthetic.synthetic_frame(h, w, seed)
            self.eng = lib.Engine(kind, vw.pack_state_dict(synthetic.make_autospeed_state_dict(int(g["weight_seed"]))), precision=precision)
            self.det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
            self.det.attach(self.eng)
            conf, iou = float(gold["conf"]), float(gold["iou"])
            self.run = lambda: (self.det.infer(frame, conf, iou), self.eng.logits().copy())[1]

    def _infer(self, frame):
        self.eng.infer(frame)
        return self.eng.logits().copy()

    def close(self):
        if self.det is not None:
            self.det.close()
        self.eng.close()


def _identities(info, rec):
    name, c, h, w = info
    assert (rec["name"], rec["c"], rec["h"], rec["w"]) == (name, c, h, w)
    assert rec["count"] == c * h * w, name
    assert int(rec["bins"].sum()) + rec["zeros"] + rec["nonfinite"] == rec["count"], name


def _equal_surveys(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x["bins"], y["bins"]) and np.array_equal(_bits(x["absmax"]), _bits(y["absmax"])), x["name"]
        assert (x["exp"], x["count"], x["nonfinite"], x["zeros"]) == (y["exp"], y["count"], y["nonfinite"], y["zeros"]), x["name"]


def _check_engine(R, full, also_full=0):
    """full: every stored tensor of at most FULL_LIMIT elements (and the `also_full` largest ones) against numpy on tensor_read; the rest, or all of them
    when not full, by the identities.  Then: a second survey gives equal words, the next pass equal logits, the plan hash stays."""
    eng = R.eng
    R.run()
    before = R.run()
    h0 = eng.plan_hash()
    s = eng.range_survey()
    info = eng.tensors()
    assert len(s) == len(info) > 0
    stored = [i for i, r in enumerate(s) if r["count"] > 0]
    assert len(stored) >= len(info) // 2, (len(stored), len(info))     # a plan stores most of its tensors: nothing may drop out of the survey unnoticed
    by_size = sorted(stored, key=lambda i: -s[i]["count"])
    compared = 0
    for i in stored:
        _identities(info[i], s[i])
        if not full or (s[i]["count"] > FULL_LIMIT and i not in by_size[:also_full]):
            continue
        r = s[i]
        x = eng.tensor_read(i)
        if r["exp"]:
            x = x * np.float32(2.0 ** -r["exp"])       # stored values: exact
        bins, zeros, nonfinite, count, absmax = cases.stats(x)
        assert np.array_equal(r["bins"], bins), (r["name"], r["bins"].tolist(), bins.tolist())
        assert (r["zeros"], r["nonfinite"], r["count"]) == (zeros, nonfinite, count), r["name"]
        assert np.array_equal(_bits(r["absmax"]), _bits(absmax)), (r["name"], r["absmax"], absmax)
        compared += 1
    print(f"{len(info)} tensors, {len(stored)} stored, {compared} compared bin by bin")
    assert not full or compared >= min(len(stored), 8)
    _equal_surveys(s, eng.range_survey())
    out = eng.logits()
    assert np.array_equal(_bits(out), _bits(before))                   # the survey's own pass left the outputs of a plain pass
    assert np.array_equal(_bits(R.run()), _bits(before)) and eng.plan_hash() == h0
    return s


@pytest.mark.parametrize("kind,precision", [("sceneseg", "fp16x3"), ("sceneseg", "fp16"), ("egolanes", "fp16x3"), ("egolanes", "fp16"), ("autospeed", "fp16x3"),
                                            ("autosteer", "fp16x3"), ("autodrive", "fp16x3")])
def test_survey_equals_numpy_on_tensor_read(kind, precision, state_dicts, frame720):
    from autoware_vision_pilot_amd import lib

    R = _Runner(lib, kind, precision, state_dicts, frame720)
    try:
        s = _check_engine(R, full=True, also_full=3 if (kind, precision) == ("sceneseg", "fp16x3") else 0)
        assert all(r["nonfinite"] == 0 and r["exp"] == 0 for r in s)
    finally:
        R.close()


@pytest.mark.parametrize("kind", ["scene3d", "domainseg"])
def test_survey_identities(kind, state_dicts, frame720):
    from autoware_vision_pilot_amd import lib

    R = _Runner(lib, kind, "fp16x3", state_dicts, frame720)
    try:
        _check_engine(R, full=False)
    finally:
        R.close()


def test_survey_reports_stored_values_on_an_act_scale_engine(state_dicts, frame720):
    """VP_ACT_SCALE: after a calibration the survey sees the STORED planes (tensor_read times 2^-exp) and names each tensor's exponent"""
    from autoware_vision_pilot_amd import lib

    R = _Runner(lib, "autosteer", "fp16x3", state_dicts, frame720, act_scale=True)
    try:
        R.run()
        R.eng.calibrate_range()
        s = _check_engine(R, full=True)
        exps = R.eng.act_scales()
        assert (exps != 0).any() and [r["exp"] for r in s] == [int(e) for e in exps]
    finally:
        R.close()


# ------------------------------------------------------------------------------------------------ overflow: located, not raised
def _hot(sd, factor):
    out = dict(sd)
    k = "Backbone.encoder.8.1.weight"          # BatchNorm scale of features[8] (320 -> 1280): scales f4, the context and the whole decoder
    assert k in sd
    out[k] = sd[k] * np.float32(factor)
    return out


def test_overflow_is_located(state_dicts, frame720):
    """tests/test_gpu_range_guard.py's construction: vp_infer answers VP_ERR_RANGE, one bit; the survey returns and names the first tensor that left the range"""
    from autoware_vision_pilot_amd import lib, weights as vw

    sd = state_dicts("sceneseg")
    hot = lib.Engine("sceneseg", vw.pack_state_dict(_hot(sd, 1e4)), precision="fp16x3")
    good = lib.Engine("sceneseg", vw.pack_state_dict(sd), precision="fp16x3")
    try:
        with pytest.raises(lib.VpRangeError):
            hot.infer(frame720)
        s = hot.range_survey()
        stored = [r for r in s if r["count"] > 0]
        bad = [k for k, r in enumerate(stored) if r["nonfinite"] > 0]
        assert bad, "no tensor reports a non-finite value"
        first = bad[0]
        print("first non-finite tensor:", stored[first]["name"], "non-finite", stored[first]["nonfinite"], "of", stored[first]["count"])
        for r in stored[:first]:
            assert r["nonfinite"] == 0 and r["absmax"] <= 65504.0, r["name"]
        # everything in front of the scaled layer computes what the healthy engine computes: the frame can only leave the range at or behind it
        assert first >= [r["name"] for r in stored].index("Backbone.encoder.8")
        assert not np.isfinite(hot.logits()).all()
        with pytest.raises(lib.VpRangeError):       # the survey changed nothing: the frame is still reported
            hot.infer(frame720)
        good.infer(frame720)
        assert all(r["nonfinite"] == 0 for r in good.range_survey())
        assert np.isfinite(good.logits()).all()
    finally:
        hot.close()
        good.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(state_dicts, frame720):
    from autoware_vision_pilot_amd import lib, synthetic, weights as vw

    sd_seg = state_dicts("sceneseg")
    sd3 = synthetic.share_backbone(dict(state_dicts("scene3d")), "scene3d", sd_seg, "sceneseg")
    base = lib.Engine("sceneseg", vw.pack_state_dict(sd_seg), precision="fp16x3")
    head = lib.Engine("scene3d", vw.pack_state_dict(sd3), precision="fp16x3", base=base)
    batched = lib.Engine("sceneseg", vw.pack_state_dict(sd_seg), precision="fp16x3", frames=2)
    try:
        with pytest.raises(lib.VpError, match="error -4"):        # VP_ERR_STATE: nothing resident
            base.range_survey()
        base.infer_multi([head], frame720)
        with pytest.raises(ValueError, match="shared-prefix"):    # VP_ERR_ARG
            head.range_survey()
        with pytest.raises(ValueError, match="batched"):
            batched.range_survey()
        assert len(base.range_survey()) == len(base.tensors())      # the base engine of a shared head owns its whole network
    finally:
        head.close()
        batched.close()
        base.close()
