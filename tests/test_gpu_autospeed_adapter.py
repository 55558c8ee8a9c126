"""adapters/autospeed_hip_engine.hpp (AutoSpeedHipEngine, the drop-in for AutoSpeedOnnxEngine) compiled against the stand-in OpenCV header and driven
by adapters/test/autospeed_check.cpp as the production app's detector thread drives the reference engine: inference(image, conf, iou).  On the CPU the
construction-failure convention; on the MI355X its detections and raw tensor against the C ABI's through the ctypes binding, bit for bit, and the
detections against the reference module's kept set (tests/golden/autospeed_net.npz)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "adapters", "test", "autospeed_check")
G = np.load(os.path.join(ROOT, "tests", "golden", "autospeed_net.npz"))


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "adapters")], check=True, capture_output=True)


def test_autospeed_engine_adapter_error_conventions():
    _build()
    r = subprocess.run([BIN], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "conventions OK" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("precision,prec_arg", [("fp16x3", "fp32"), ("fp16", "fp16")])
def test_autospeed_engine_adapter_matches_c_abi(tmp_path, precision, prec_arg):
    from autoware_vision_pilot_amd import lib, synthetic, weights as vw

    _build()
    h, w, seed = (int(v) for v in G["frames"][0])
    frame = synthetic.synthetic_frame(h, w, seed)
    blob, ff, out = tmp_path / "autospeed.vpw", tmp_path / "frame.bgr", tmp_path / "out.bin"
    blob.write_bytes(vw.pack_state_dict(synthetic.make_autospeed_state_dict(int(G["weight_seed"]))))
    frame.tofile(ff)
    conf, iou = float(G["conf"]), float(G["iou"])              # the fixture's thresholds: float32 values, passed on with all their digits
    r = subprocess.run([BIN, str(blob), str(ff), str(h), str(w), str(out), prec_arg, repr(conf), repr(iou)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(out, dtype=np.uint8)
    n = int(raw[:4].view(np.int32)[0])
    det_bytes = raw[4:4 + 24 * n]
    shape = tuple(int(v) for v in raw[4 + 24 * n:4 + 24 * n + 24].view(np.int64))
    assert shape == (1, 8, 10752)
    tensor = raw[4 + 24 * n + 24:].view(np.float32).reshape(8, 10752)
    eng = lib.Engine("autospeed", blob.read_bytes(), precision=precision)
    det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
    try:
        det.attach(eng)
        want, nw = det.infer(frame, conf, iou, cap=10752)
        assert n == nw and n > 0
        got = det_bytes.view(np.float32).reshape(n, 6).copy()
        got[:, 5] = det_bytes.view(np.int32).reshape(n, 6)[:, 5].astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))                       # kept set, order, coordinates, confidence, class
        assert np.array_equal(tensor.view(np.uint32), eng.logits().reshape(8, 10752).view(np.uint32))
    finally:
        det.close()
        eng.close()
    ref = G["det_0"]                                                                           # ... and against the reference's own module
    assert n == len(ref) and np.array_equal(got[:, 5], ref[:, 5])
    if precision == "fp16x3":
        assert float((np.abs(got[:, :5] - ref[:, :5]) / np.maximum(1.0, np.abs(ref[:, :5]))).max()) <= 1e-3
