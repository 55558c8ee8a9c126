#!/usr/bin/env python3
"""What the detector's validation record (vp_metric_add_det*) costs on one MI355X.  THE WEIGHTS ARE SYNTHETIC.  Nothing is fixed in advance: the file
records what was measured, one run on one box.

  (a) microseconds per add_det_raw record at nb 10752, nc 4 on the VP_AUTOSPEED fp16 engine's own output (device-resident), wall clock over FRAMES
      adds and the one fetch behind them, after WARM adds; the record's candidate count beside it
  (b) the same on a dense tensor: the dense case of tests/detmap_cases.py with the fourth class raised above the threshold (43 007 candidates)
  (c) the same frames through tests/detmap_ref.py on the host (validate + match), wall clock
  (d) VP_AUTOSPEED fp16 passes/s, enqueue only, with and without an add_det behind every pass, alternating rounds in one process

python tools/bench_detmap.py > profiles/detmap.txt"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import detmap_cases as dc
import detmap_ref as dr
from autoware_vision_pilot_amd import lib, synthetic, weights as vw

WARM, FRAMES = 20, 200


def per_record_us(m, d_raw, labels):
    def adds(n):
        for _ in range(n):
            m.add_det_raw(d_raw.data_ptr(), labels, (dc.NET_H, dc.NET_W), device_shape=(4, 10752))

    m.reset()
    adds(WARM)
    m.fetch_det()
    m.reset()
    t0 = time.perf_counter()
    adds(FRAMES)
    fr, _, _ = m.fetch_det()
    return round((time.perf_counter() - t0) * 1e6 / FRAMES, 1), fr


def host_us(raw, labels, reps=5):
    px = dc.labels_px(labels)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dr.run_frame(raw, px, dc.IOU_V)
        t.append((time.perf_counter() - t0) * 1e6)
    return round(float(np.median(t)), 1)


def main():
    eng = lib.Engine("autospeed", vw.pack_state_dict(synthetic.make_autospeed_state_dict(5)), precision="fp16")
    det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
    det.attach(eng)
    det.infer(synthetic.synthetic_frame(720, 1280, 21), 0.4, 0.65)
    own = eng.logits().reshape(8, 10752).copy()
    dense, labels = dc.frame("dense")
    dense = dense.copy()
    dense[7] = 0.002 + 0.5 * dense[4][::-1]
    dense[7, 100] = 0.5
    out = {"library": lib.version(), "weights": "SYNTHETIC; one run on one box", "frames_per_measurement": FRAMES, "warm_up": WARM}
    m = lib.Metric(max_frames=WARM + FRAMES)
    for name, raw in (("engine_output", own), ("dense", dense)):
        d_raw = torch.from_numpy(raw).cuda()
        torch.cuda.synchronize()
        rounds = []
        for _ in range(3):
            us, fr = per_record_us(m, d_raw, labels)
            rounds.append(us)
        out[name] = {"candidates": int(fr[0]["candidates"]), "ranked": int(fr[0]["ranked"]), "kept": int(fr[0]["kept"]), "a_b_device_us_per_record_rounds": rounds,
                     "c_host_restatement_us_per_frame": host_us(raw, labels)}
    d = {"without": [], "with_add_det": []}
    for _ in range(3):
        for key in d:
            m.reset()
            for _ in range(WARM):
                eng.enqueue()
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(FRAMES):
                eng.enqueue()
                if key != "without":
                    m.add_det(eng, labels)
            eng.sync()
            m.fetch_det()
            d[key].append(round(FRAMES / (time.perf_counter() - t0), 1))
    out["d_autospeed_fp16_passes_per_s_rounds"] = d
    print(json.dumps(out, indent=1))
    m.close()
    det.close()
    eng.close()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("bench_detmap.py needs a GPU")
    main()
