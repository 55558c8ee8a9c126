"""The AutoSpeed detector network's CPU pin: tests/autospeed_net_ref.py -- the functional restatement of the reference's YOLO.forward --
reproduces tests/golden/autospeed_net.npz, the outputs of the reference's OWN nn.Module (tools/pin_autospeed_net.py asserted distance 0.0 between
the two when it wrote the file), and the synthetic generator has the module's key list."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import autospeed_net_ref as ref  # noqa: E402
from autoware_vision_pilot_amd import synthetic  # noqa: E402
from oracle import autospeed  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "autospeed_net.npz")


def _close(a, b, tol=1e-4):   # the comparison of tests/test_oracle_golden.py
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) <= tol


def test_state_dict_has_the_reference_modules_keys():
    """AutoSpeedNetwork().build_model('n', 4).state_dict() has 375 keys, 116 of them under `net.`; one num_batches_tracked per BatchNorm is among them
    (60 / 14), which the generator leaves out as the AutoDrive path does: 315 / 102 tensors here.  9.3 M parameters."""
    sd = synthetic.make_autospeed_state_dict(0)
    keys = list(sd)
    bn = [k for k in keys if k.endswith(".norm.running_var")]
    assert len(keys) + len(bn) == 375
    net = [k for k in keys if k.startswith("net.")]
    assert len(net) + sum(k.startswith("net.") for k in bn) == 116
    assert all(k.startswith(("net.", "fpn.", "head.")) for k in keys) and "head.dfl.conv.weight" in sd
    assert not any(k.endswith("num_batches_tracked") for k in keys)
    ad = [k for k, _, _ in synthetic.autodrive_spec() if k.startswith("backbone.")]
    assert [k[len("net."):] for k in net] == [k[len("backbone."):] for k in ad]          # AutoDrive's backbone, key for key
    assert np.array_equal(sd["head.dfl.conv.weight"].ravel(), np.arange(16, dtype=np.float32))
    assert synthetic.autospeed_param_count() == sum(v.size for k, v in sd.items() if not k.endswith(("running_mean", "running_var")))
    assert 9.2e6 < synthetic.autospeed_param_count() < 9.4e6
    assert sd["head.cls.0.4.weight"].shape[0] == synthetic.AS_NUM_CLASSES and synthetic.AS_NUM_ANCHORS == 10752


def test_restatement_reproduces_the_reference_modules_vectors():
    g = np.load(GOLDEN)
    sd = synthetic.make_autospeed_state_dict(int(g["weight_seed"]))
    bs, ts = int(g["box_step"]), int(g["tap_step"])
    for fi, (h, w, seed) in enumerate(g["frames"]):
        frame = synthetic.synthetic_frame(int(h), int(w), int(seed))
        x, geom = autospeed.preprocess(frame, ref.NET_H, ref.NET_W)
        raw, taps = ref.forward(sd, x)
        assert raw.shape == (4 + synthetic.AS_NUM_CLASSES, synthetic.AS_NUM_ANCHORS)
        assert _close(raw[:, ::bs], g[f"raw_{fi}"])
        for name, t in zip(("p3", "p4", "p5"), taps):
            assert _close(t.ravel()[::ts], g[f"{name}_{fi}"]), name
        # the conditions the detection tests rely on hold for the reference's raw (checked when the fixture was written): 20 .. 2000 candidates
        n = int((g[f"raw_{fi}"][4:].max(axis=0) >= g["conf"]).sum()) * bs
        assert 20 <= n <= 2000 + bs * 8
        det = autospeed.postprocess(raw, float(g["conf"]), float(g["iou"]), geom[0], geom[1], geom[2], int(w), int(h))
        want = g[f"det_{fi}"]
        assert det.shape == want.shape and len(want) >= 5
        assert np.array_equal(det[:, 5], want[:, 5]) and _close(det[:, :5], want[:, :5], tol=1e-3)
