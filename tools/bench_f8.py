#!/usr/bin/env python3
"""What VP_MFMA_FP8 does on one MI355X, for SceneSeg alone and for the SceneSeg + Scene3D pair (two engines that own their networks, one frame each per
step: the flag is refused for shared-prefix heads).  THE WEIGHTS ARE SYNTHETIC (the seeded state-dicts of BASELINE / tests/conftest.py) and so are the
frames.  Nothing is fixed in advance: the file records what was measured, a layer that got slower included.

  (a) vp_profile_layers time of every layer the kernel fits -- the one the dispatch rule moves (decode_layer_5) and, on a second flagged engine created
      under VP_PLAN_OVERRIDE "decode_layer_7=13;decode_layer_9=13", the two the rule leaves on their fp16 kernels -- against the unflagged VP_FP16
      engine (its plan is the one tests/golden/kernel_plan*.json pins), the engines profiled alternately, ROUNDS rounds of ITERS launches each; the
      layer's fp16 kernel and FLOPs.
  (b) frames/s and p50 of a frame (vp_infer: upload, graph replay, fetch, synchronise) of both engines, alternating, ROUNDS rounds of FRAMES frames behind
      WARM warm-up frames.
  (c) the vp_metric pair scores of both engines against a VP_FP16X3 engine (same synthetic frames and weights) over N_SCORE frames, after ONE
      vp_calibrate_fp8 on the first frame: IoU / flipped pixels for SceneSeg, mAE / mEL for Scene3D; the calibrated exponents.  The override engines
      of (a) are scored too: what all three layers on fp8 would cost.

python tools/bench_f8.py > profiles/f8_mfma.txt"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  -- first: one shared HIP runtime

from autoware_vision_pilot_amd import lib, synthetic, weights as vw
from oracle import weights

SEEDS = {"sceneseg": 0, "scene3d": 1}
H, W = 720, 1280
ROUNDS, ITERS, WARM, FRAMES, N_SCORE = 3, 20, 30, 200, 16


def engine(kind, precision="fp16", **kw):
    return lib.Engine(kind, vw.pack_state_dict(weights.make_state_dict(kind, SEEDS[kind])), precision=precision, **kw)


def layer_times(plain, f8):
    """(a): per moved layer {name, kernels, us per round of both engines, GFLOP}"""
    rows_p = list(zip(plain.layers(), plain.layer_kernels()))
    rows_f = list(zip(f8.layers(), f8.layer_kernels()))
    moved = [i for i, (_, k) in enumerate(rows_f) if k == "conv3x3_f8"]
    tp, tf = [], []
    for _ in range(ROUNDS):
        tp.append(plain.profile_layers(ITERS))
        tf.append(f8.profile_layers(ITERS))
    out = []
    for i in moved:
        us_p = [round(float(t[i]) * 1e3, 1) for t in tp]
        us_f = [round(float(t[i]) * 1e3, 1) for t in tf]
        out.append({"layer": rows_f[i][0][0], "fp16_kernel": rows_p[i][1], "gflop": round(rows_f[i][0][1] / 1e9, 2), "fp16_us": us_p, "f8_us": us_f,
                    "f8_over_fp16": round(float(np.median(us_f) / np.median(us_p)), 3),
                    "f8_tflops": round(rows_f[i][0][1] / (np.median(us_f) * 1e-6) / 1e12, 1), "fp16_tflops": round(rows_f[i][0][1] / (np.median(us_p) * 1e-6) / 1e12, 1)})
    total = {"all_layers_fp16_us": [round(float(t.sum()) * 1e3, 1) for t in tp], "all_layers_f8_us": [round(float(t.sum()) * 1e3, 1) for t in tf]}
    return out, total


def frame_rate(groups, frame):
    """(b): groups = {name: [engines run back to back per step]}; alternating rounds -> frames/s and p50 (ms) of a step per round"""
    out = {k: {"frames_per_s": [], "p50_ms": []} for k in groups}
    for engs in groups.values():
        for _ in range(WARM):
            for e in engs:
                e.infer(frame)
    for _ in range(ROUNDS):
        for name, engs in groups.items():
            ts = []
            for _ in range(FRAMES):
                t0 = time.perf_counter()
                for e in engs:
                    e.infer(frame)
                ts.append(time.perf_counter() - t0)
            out[name]["frames_per_s"].append(round(FRAMES / sum(ts), 1))
            out[name]["p50_ms"].append(round(float(np.percentile(ts, 50)) * 1e3, 3))
    return out


def scores(kind, engines, ref, frames):
    """(c): vp_metric pair scores of each engine against `ref` over the frames"""
    out = {}
    for name, eng in engines.items():
        m = lib.Metric(max_frames=len(frames))
        for f in frames:
            ref.infer(f)
            eng.infer(f)
            (m.add_depth_pair if kind == "scene3d" else m.add_seg_pair)(eng, ref)
        rec, s = m.fetch()
        if kind == "scene3d":
            out[name] = {"mae": s["mae"], "mel": s["mel"], "nan_frames": s["nan_frames"], "mae_max": float(np.nanmax(rec["mae"])), "mel_max": float(np.nanmax(rec["mel"]))}
        else:
            flipped = (rec["P"][:, :3].sum(1) + rec["G"][:, :3].sum(1) - 2 * rec["I"][:, :3].sum(1)) / 2
            out[name] = {"iou": [round(float(v), 5) for v in s["sceneseg_iou"]], "iou_full": s["sceneseg_iou_full"], "flipped_pixels_mean": float(flipped.mean()),
                         "flipped_pixels_max": float(flipped.max()), "pixels": int(rec["n"][0]), "nonfinite": int(rec["nonfinite"].sum())}
        m.close()
    return out


def main():
    if not torch.cuda.is_available():
        sys.exit("bench_f8.py needs a GPU")
    frames = [synthetic.synthetic_frame(H, W, 100 + i) for i in range(N_SCORE)]
    out = {"library": lib.version(), "weights": "SYNTHETIC (seeded state-dicts %s); frames: synthetic %d x %d" % (SEEDS, W, H),
           "rounds": ROUNDS, "profile_iters": ITERS, "warm_up_frames": WARM, "frames_per_round": FRAMES, "score_frames": N_SCORE}
    plain = {k: engine(k) for k in SEEDS}
    f8 = {k: engine(k, mfma_fp8=True) for k in SEEDS}
    lib.set_option("VP_PLAN_OVERRIDE", "decode_layer_7=13;decode_layer_9=13")
    try:
        wide = {k: engine(k, mfma_fp8=True) for k in SEEDS}
    finally:
        lib.clear_options()
    for k in SEEDS:
        plain[k].infer(frames[0])
        for e in (f8[k], wide[k]):
            e.infer(frames[0])
            e.calibrate_fp8(0)          # ONE calibration, on the first frame
    out["calibrated_qexp"] = {k: [(wide[k].layers()[l][0], q) for l, _, q in wide[k].fp8_layers()] for k in SEEDS}
    out["a_layer_times"] = {}
    for k in SEEDS:
        rows, _ = layer_times(plain[k], wide[k])
        _, total = layer_times(plain[k], f8[k])
        out["a_layer_times"][k] = {"rule_moves": [f8[k].layers()[l][0] for l, _, _ in f8[k].fp8_layers()], "layers": rows, **total}
    out["b_frames"] = frame_rate({"sceneseg_fp16": [plain["sceneseg"]], "sceneseg_f8": [f8["sceneseg"]],
                                  "pair_fp16": [plain["sceneseg"], plain["scene3d"]], "pair_f8": [f8["sceneseg"], f8["scene3d"]]}, frames[0])
    out["c_scores_against_fp16x3"] = {}
    for k in SEEDS:
        ref = engine(k, "fp16x3")
        out["c_scores_against_fp16x3"][k] = scores(k, {"fp16": plain[k], "fp16+mfma_fp8": f8[k], "fp16+mfma_fp8, decode_layer_7 / 9 too (override)": wide[k]}, ref, frames)
        ref.close()
    for d in (plain, f8, wide):
        for e in d.values():
            e.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
