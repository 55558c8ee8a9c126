#!/usr/bin/env python3
"""What the lateral thread's lane filter costs on one MI355X with vp_lanes, against the path it replaces.  THE WEIGHTS ARE SYNTHETIC (the seeded EgoLanes
state-dict of tests/conftest.py), so the planes are not lane-shaped; the threshold is the median logit, which keeps all four searches busy.  Nothing is
fixed in advance: the file records what was measured.  No ratio is promised -- the search is serial by nature; what disappears is the D2H of the logits
and the host's threshold loop.

Host to host per frame, wall clock, p50 / p90 over FRAMES frames after WARM, the 1280 x 720 frame uploaded from pageable host memory every time:
  (a) the path before vp_lanes: vp_upload_frame, vp_enqueue, vp_fetch_outputs (logits only: 153 600 bytes D2H), vp_logits and the adapter's
      threshold loop (three 0/1 float planes) in numpy.  The serial pixel search of LaneFilter::update would FOLLOW this on the host and is NOT in it.
  (b) vp_upload_frame, vp_enqueue, vp_lanes_add, vp_lanes_fetch: start points, windows, moments, fit and smoothing included (one record D2H).
  (p) the pass alone for scale: vp_upload_frame, vp_enqueue, vp_sync.
Device time of the kernel: FRAMES vp_lanes_add calls on the engine's resident logits between two events on the ENGINE's stream (every add makes that
stream wait for the filter's read, so the second event lies behind the last launch), divided by FRAMES.

NOT MEASURED: the reference's own LaneFilter::update on the CPU (OpenCV is not available where this runs), so the host search that (a) leaves to the
caller has no figure here and that half of the comparison is missing.

python tools/bench_lanes.py > profiles/lanes.txt"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401 -- first: one shared HIP runtime

from autoware_vision_pilot_amd import lib, synthetic, weights as vw
from oracle import weights

WARM, FRAMES = 20, 200
H, W = 720, 1280
RECORD_BYTES = 2 * (8 * 4 + 8 * 8 + 2 * 20 * 4 * 2)   # vp::LaneFilterRecord: two lanes of 8 ints, 8 moments, 2 x 20 windows of 4 shorts


def pct(v, q):
    return round(float(np.percentile(np.asarray(v) * 1e6, q)), 1)


def timed(step):
    for _ in range(WARM):
        step()
    t = []
    for _ in range(FRAMES):
        t0 = time.perf_counter()
        step()
        t.append(time.perf_counter() - t0)
    return {"p50_us": pct(t, 50), "p90_us": pct(t, 90), "min_us": pct(t, 0)}


def main():
    frame = synthetic.synthetic_frame(H, W, 21)
    eng = lib.Engine("egolanes", vw.pack_state_dict(weights.make_state_dict("egolanes", 2)), precision="fp16")
    eng.set_outputs(logits=True, mask=False)
    eng.infer(frame)
    thr = float(np.median(eng.logits()))
    lanes = lib.Lanes(capacity=WARM + FRAMES)
    out = {"library": lib.version(), "weights": "SYNTHETIC (seeded state-dict); frame: synthetic 1280 x 720; threshold: the median logit %.6f" % thr,
           "frames_per_measurement": FRAMES, "warm_up": WARM}

    def path_a():
        eng.upload_frame(frame)
        eng.enqueue()
        eng.fetch_outputs()
        lg = eng.logits()
        return [(lg[c] > thr).astype(np.float32) for c in range(3)]

    def path_b():
        eng.upload_frame(frame)
        eng.enqueue()
        lanes.add(eng, thr)
        return lanes.fetch()

    def pass_alone():
        eng.upload_frame(frame)
        eng.enqueue()
        eng.sync()

    rounds = {"a_logits_and_threshold": [], "b_lanes_add_fetch": [], "p_pass_alone": []}
    for _ in range(3):                                           # interleaved rounds: a drift of the machine shows in all three
        rounds["p_pass_alone"].append(timed(pass_alone))
        rounds["a_logits_and_threshold"].append(timed(path_a))
        rounds["b_lanes_add_fetch"].append(timed(path_b))
    out["host_to_host_rounds"] = rounds
    out["host_to_host_p50_us"] = {k: sorted(r["p50_us"] for r in v)[1] for k, v in rounds.items()}
    rec = path_b()[0]
    out["record_of_the_frame"] = {side: {"start": [int(rec["lane"][i]["start_x"]), int(rec["lane"][i]["start_y"])],
                                         "windows": int(rec["lane"][i]["n_windows_up"]) + int(rec["lane"][i]["n_windows_down"]),
                                         "points": int(rec["lane"][i]["n_points_up"]) + int(rec["lane"][i]["n_points_down"]), "order": int(rec["lane"][i]["order"])}
                                  for i, side in enumerate(("left", "right"))}
    # the kernel's own time
    eng.sync()
    kernel = []
    for _ in range(3):
        for _ in range(WARM):
            lanes.add(eng, thr)
        lanes.fetch()
        eng.sync()
        eng.timer_begin()
        for _ in range(FRAMES):
            lanes.add(eng, thr)
        kernel.append(round(eng.timer_end() * 1e3 / FRAMES, 2))
        lanes.fetch()
    out["kernel_us_per_record_rounds"] = kernel
    out["kernel_us_per_record"] = sorted(kernel)[1]
    out["bytes_device_to_host_per_frame"] = {"a_logits": 3 * 80 * 160 * 4, "b_record": RECORD_BYTES, "b_points_on_request_at_most": 2 * 1920 * 2}
    out["not_measured"] = "the reference's CPU LaneFilter::update (no OpenCV here): the host search that follows path (a) has no figure"
    lanes.close()
    eng.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
