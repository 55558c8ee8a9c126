#!/usr/bin/env python3
"""What VP_ACT_SCALE costs AutoDrive on one MI355X: one-camera p50 / p99 (vp_infer: H2D of the frame, the replayed graph, D2H of the three floats, one
wait) and back-to-back frames/s (vp_enqueue, one wait at the end) of the flagged, calibrated engine and of the unflagged engine -- same process, same
box, latency plan, the protocol of tools/bench_autosteer.py, the two engines taking turns over three rounds -- the time of one vp_calibrate_range call,
and the errors of both engines against fp64 on the ordinary pair of tests/golden/autodrive_range.npz.  Needs a GPU: there is no fall-back.

python tools/bench_act_scale.py > profiles/act_scale.txt"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (first: one shared HIP runtime)

from autoware_vision_pilot_amd import lib, weights as vw
from oracle import autodrive, pre_post

G = np.load(os.path.join(ROOT, "tests", "golden", "autodrive_range.npz"))
blob = vw.pack_state_dict(autodrive.make_state_dict(int(G["weight_seed"])))
fr = [pre_post.synthetic_frame(1080, 1920, 200 + k, smooth=(k % 3 != 2)) for k in (0, 1, 3, 4)]
out = {"library": lib.version()}
engs = {"unflagged": lib.Engine("autodrive", blob, precision="fp16x3", plan_latency=True),
        "act_scale": lib.Engine("autodrive", blob, precision="fp16x3", plan_latency=True, act_scale=True)}
engs["act_scale"].infer_pair(fr[0], fr[1])
t0 = time.perf_counter()
engs["act_scale"].calibrate_range()
out["calibrate_range_one_call_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
exps = engs["act_scale"].act_scales()
out["exponents"] = {n: int(e) for (n, _, _, _), e in zip(engs["act_scale"].tensors(), exps)}
for tag, eng in engs.items():
    eng.infer_pair(fr[2], fr[3])
    got = eng.logits().reshape(3).astype(np.float64)
    out[f"{tag}_pair_b_err_vs_fp64_rel_to_max(1,|ref|)"] = float((np.abs(got - G["b_fp64"]) / np.maximum(1.0, np.abs(G["b_fp64"]))).max())
res = {tag: {"p50": [], "p99": [], "fps": []} for tag in engs}
for rnd in range(3):
    for tag, eng in engs.items():
        f = fr[0]
        for _ in range(100):
            eng.infer(f)
        t = []
        for _ in range(1000):
            t0 = time.perf_counter(); eng.infer(f); t.append((time.perf_counter() - t0) * 1e6)
        res[tag]["p50"].append(round(float(np.percentile(t, 50)), 1))
        res[tag]["p99"].append(round(float(np.percentile(t, 99)), 1))
        for _ in range(50):
            eng.enqueue()
        eng.sync()
        n = 2000
        t0 = time.perf_counter()
        for _ in range(n):
            eng.enqueue()
        eng.sync()
        res[tag]["fps"].append(round(n / (time.perf_counter() - t0), 1))
for tag in engs:
    out[f"{tag}_infer_one_camera_p50_us_rounds"] = res[tag]["p50"]
    out[f"{tag}_infer_one_camera_p99_us_rounds"] = res[tag]["p99"]
    out[f"{tag}_back_to_back_frames_per_s_rounds"] = res[tag]["fps"]
out["p50_ratio_act_scale_over_unflagged"] = round(float(np.median(res["act_scale"]["p50"]) / np.median(res["unflagged"]["p50"])), 4)
out["frames_per_s_ratio_act_scale_over_unflagged"] = round(float(np.median(res["act_scale"]["fps"]) / np.median(res["unflagged"]["fps"])), 4)
# where the difference sits: every launch alone (vp_profile_layers, device events, mean of 20), summed per kernel family
prof = {tag: eng.profile_layers(20) for tag, eng in engs.items()}
kern = engs["act_scale"].layer_kernels()
fam = lambda k: "conv (MFMA kernels + split-K finish)" if k.startswith("conv") else "other launches"
for f in sorted({fam(k) for k in kern}):
    idx = [i for i, k in enumerate(kern) if fam(k) == f]
    out[f"isolated_launch_sum_us [{f}] ({len(idx)} launches)"] = {tag: round(float(sum(prof[tag][i] for i in idx)) * 1e3, 1) for tag in engs}
worst = sorted(range(len(kern)), key=lambda i: prof["unflagged"][i] - prof["act_scale"][i])[:5]
out["largest_per_launch_increase_us"] = {engs["act_scale"].layers()[i][0] + " " + kern[i]: [round(float(prof["unflagged"][i]) * 1e3, 1), round(float(prof["act_scale"][i]) * 1e3, 1)] for i in worst}
for eng in engs.values():
    eng.close()
print(json.dumps(out, indent=1))
