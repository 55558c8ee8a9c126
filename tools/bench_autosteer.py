#!/usr/bin/env python3
"""The AutoSteer 2.0 lane-perception network (VP_AUTOSTEER) on one MI355X, both precisions: the per-launch table (vp_profile_layers: every launch
alone, device events), p50 / p99 latency of one camera (vp_infer: H2D of the 512 x 1024 frame, the replayed graph, D2H of the 128 floats, one wait),
back-to-back frames/s with the frame resident (vp_enqueue, one wait at the end), the head's share of the sum of launches, and the parity errors
against the restatement on the two fixture frames.  Needs a GPU: there is no fall-back.

python tools/bench_autosteer.py > profiles/autosteer_net.txt"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401  (first: one shared HIP runtime)

import autosteer_net_ref as ref
from autoware_vision_pilot_amd import lib, synthetic, weights as vw

G = np.load(os.path.join(ROOT, "tests", "golden", "autosteer_net.npz"))
sd = synthetic.make_autosteer_state_dict(int(G["weight_seed"]))
blob = vw.pack_state_dict(sd)
frames = [synthetic.synthetic_frame(ref.NET_H, ref.NET_W, int(s)) for s in G["frame_seeds"]]
wants = [ref.forward(sd, ref.preprocess(f))[0] for f in frames]
out = {"library": lib.version()}
for prec in ("fp16x3", "fp16"):
    eng = lib.Engine("autosteer", blob, precision=prec, plan_latency=True)
    for fi, (f, (xp, h)) in enumerate(zip(frames, wants)):
        eng.infer(f)
        got = eng.logits().reshape(2, 64)
        out[f"{prec}_frame{fi}_xp_max_abs_err"] = float(np.abs(got[0] - xp).max())
        out[f"{prec}_frame{fi}_h_vector_err_rel_to_max(1,|ref|)"] = float((np.abs(got[1] - h) / np.maximum(1.0, np.abs(h))).max())
        out[f"{prec}_frame{fi}_validity_decisions_equal"] = bool(np.array_equal(got[1] >= 0.5, h >= 0.5))
    f = frames[0]
    for _ in range(100):
        eng.infer(f)
    t = []
    for _ in range(1000):
        t0 = time.perf_counter(); eng.infer(f); t.append((time.perf_counter() - t0) * 1e6)
    out[f"{prec}_infer_one_camera_p50_us"] = round(float(np.percentile(t, 50)), 1)
    out[f"{prec}_infer_one_camera_p99_us"] = round(float(np.percentile(t, 99)), 1)
    g = []
    for _ in range(200):
        eng.timer_begin(); eng.enqueue(); g.append(eng.timer_end() * 1e3)
    out[f"{prec}_network_in_graph_p50_us"] = round(float(np.percentile(g, 50)), 1)
    for _ in range(50):
        eng.enqueue()
    eng.sync()
    n = 2000
    t0 = time.perf_counter()
    for _ in range(n):
        eng.enqueue()
    eng.sync()
    out[f"{prec}_back_to_back_frames_per_s"] = round(n / (time.perf_counter() - t0), 1)
    ms = eng.profile_layers(20)
    rows = list(zip(eng.layers(), eng.layer_kernels(), ms))
    print(f"# per-launch table, VP_AUTOSTEER {prec} | VP_PLAN_LATENCY (us, mean of 20 isolated launches)")
    for (name, _, _), tag, v in rows:
        print(f"{name:40s} {tag:44s} {v * 1e3:8.1f}")
    total = float(sum(ms)) * 1e3
    head = float(sum(v for (nm, _, _), v in zip(eng.layers(), ms) if nm.startswith("head."))) * 1e3
    out[f"{prec}_launches"] = len(rows)
    out[f"{prec}_sum_of_launches_us"] = round(total, 1)
    out[f"{prec}_backbone_launches_us"] = round(float(sum(v for (nm, _, _), v in zip(eng.layers(), ms) if nm.startswith("net."))) * 1e3, 1)
    out[f"{prec}_head_3_launches_us"] = round(head, 1)
    out[f"{prec}_head_share_of_sum_of_launches"] = round(head / total, 4)
    eng.close()
print(json.dumps(out, indent=1))
