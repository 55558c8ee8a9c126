#!/usr/bin/env python3
"""What VP_ACT_SCALE costs the AutoSteer and AutoSpeed engines on one MI355X: one-camera p50 / p99 of vp_infer (AutoSteer) and of vp_detect_infer
(AutoSpeed: letterbox, network, decode + NMS, one wait) and the in-graph time per frame (vp_enqueue back to back, one wait at the end) of the flagged,
calibrated engine and of the unflagged engine -- same process, same build, latency plan, the two engines taking turns over three rounds, the protocol of
tools/bench_act_scale.py -- and the time of one vp_calibrate_range call.  The unflagged figures are the ones to hold against the commit before the flag
reached these kinds, whose plans are the same: --unflagged-only --tree DIR measures the unflagged engines alone with the package built in DIR (a
checkout of that commit; the cases and frames stay this tree's).  Needs a GPU: there is no fall-back.

python tools/bench_act_scale_nets.py > profiles/act_scale_nets.txt"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=ROOT, help="the checkout whose built package is measured")
ap.add_argument("--unflagged-only", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401  (first: one shared HIP runtime)

import act_scale_nets_cases as cases
from autoware_vision_pilot_amd import lib

ROUNDS, WARM, TIMED, B2B = 3, 100, 1000, 2000
out = {"library": lib.version(), "protocol": f"{ROUNDS} rounds, engines taking turns; per round {WARM} warm-up + {TIMED} timed calls, then {B2B} vp_enqueue back to back"}
for net in ("autosteer", "autospeed"):
    N = cases.Net(lib, net)
    blob = N.blob("ordinary")
    engs = {"unflagged": N.engine(blob, plan_latency=True)}
    if not args.unflagged_only:
        engs["act_scale"] = N.engine(blob, plan_latency=True, act_scale=True)
        N.run(*engs["act_scale"])
        t0 = time.perf_counter()
        engs["act_scale"][0].calibrate_range()
        out[f"{net}_calibrate_range_one_call_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        exps = engs["act_scale"][0].act_scales()
        out[f"{net}_exponents_min_max"] = [int(exps.min()), int(exps.max())]
    res = {tag: {"p50": [], "p99": [], "graph": []} for tag in engs}
    for rnd in range(ROUNDS):
        for tag, (eng, det) in engs.items():
            for _ in range(WARM):
                N.run(eng, det) if det is None else det.infer(N.frame, 0.4, 0.65)
            t = []
            for _ in range(TIMED):
                t0 = time.perf_counter()
                if det is None:
                    eng.infer(N.frame)
                else:
                    det.infer(N.frame, 0.4, 0.65)
                t.append((time.perf_counter() - t0) * 1e6)
            res[tag]["p50"].append(round(float(np.percentile(t, 50)), 1))
            res[tag]["p99"].append(round(float(np.percentile(t, 99)), 1))
            for _ in range(50):
                eng.enqueue()
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(B2B):
                eng.enqueue()
            eng.sync()
            res[tag]["graph"].append(round((time.perf_counter() - t0) / B2B * 1e6, 1))
    call = "vp_infer" if net == "autosteer" else "vp_detect_infer"
    for tag in engs:
        out[f"{net}_{tag}_{call}_p50_us_rounds"] = res[tag]["p50"]
        out[f"{net}_{tag}_{call}_p99_us_rounds"] = res[tag]["p99"]
        out[f"{net}_{tag}_in_graph_us_per_frame_rounds"] = res[tag]["graph"]
    if args.unflagged_only:
        N.close()
        continue
    out[f"{net}_p50_ratio_act_scale_over_unflagged"] = round(float(np.median(res["act_scale"]["p50"]) / np.median(res["unflagged"]["p50"])), 4)
    out[f"{net}_in_graph_ratio_act_scale_over_unflagged"] = round(float(np.median(res["act_scale"]["graph"]) / np.median(res["unflagged"]["graph"])), 4)
    N.close()
print(json.dumps(out, indent=1))
