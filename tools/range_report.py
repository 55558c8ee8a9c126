#!/usr/bin/env python3
"""Where a checkpoint's activations sit in the fp16 exponent range: vp_range_survey (include/vp_hip.h "RANGE SURVEY") over one network and a set of
frames, one TSV row per tensor the plan stores in HBM.  Run it when vp_infer answers VP_ERR_RANGE (the report names the first tensor that left the
range) and before a new checkpoint is deployed (headroom of a healthy run, share of values the low plane no longer resolves).  Needs a GPU.

  python tools/range_report.py sceneseg --weights model.vpw --frames a.png b.npy           a checkpoint (.vpw / .onnx) on frames of yours
  python tools/range_report.py domainseg --weight-seed 23 --frame-seeds 1                   seeded synthetic weights and frames

Frames: files readable with numpy (.npy: HxWx3 uint8, BGR) or Pillow (anything else, converted to BGR), or --frame-seeds with --frame-size.  The scene
networks and AutoDrive resize any frame, AutoSpeed letterboxes it, AutoSteer takes 512 x 1024 only.  AutoDrive pairs every frame with itself.
Counters are summed over the frames, the abs-max is the largest seen.  Columns: tensor index and name, c, h, w, VP_ACT_SCALE exponent, abs-max of the
STORED value, headroom = 15 - floor(log2 absmax) binades, non-finite and zero counts, element count, share of the non-zero values below 0.125 (two-plane
engines: the low plane's quantum is an fp16 subnormal there) and below 2^-14 (the high plane itself is subnormal), then the 40 bins floor(log2 |x|) =
-24 .. 15.  Not seen: values that only live on chip (the expanded tensor inside the fused MBConv kernels, the up-sampled tensor of a composed stage)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

SCENE_SEEDS = {"sceneseg": 0, "scene3d": 1, "egolanes": 2, "domainseg": 3}     # BASELINE's weight seeds; the other kinds: their golden files' seed


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("kind", choices=("sceneseg", "scene3d", "domainseg", "egolanes", "autodrive", "autospeed", "autosteer"))
    ap.add_argument("--weights", help=".vpw or .onnx file; without it: seeded synthetic weights (--weight-seed)")
    ap.add_argument("--weight-seed", type=int, default=None)
    ap.add_argument("--frames", nargs="*", default=[], help="frame files (.npy HxWx3 uint8 BGR, or an image Pillow reads)")
    ap.add_argument("--frame-seeds", type=int, nargs="*", default=[], help="seeded synthetic frames")
    ap.add_argument("--frame-size", type=int, nargs=2, default=None, metavar=("H", "W"), help="of the synthetic frames (default 720 1280; AutoSteer 512 1024)")
    ap.add_argument("--precision", choices=("fp16x3", "fp16"), default="fp16x3")
    ap.add_argument("--weights-fp8", action="store_true")
    ap.add_argument("--plan-latency", action="store_true")
    ap.add_argument("--no-header", action="store_true")
    return ap.parse_args(argv)


def load_frame(path):
    if path.endswith(".npy"):
        f = np.load(path)
    else:
        from PIL import Image

        f = np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1]
    if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
        raise SystemExit(f"{path}: a frame is HxWx3 uint8")
    return np.ascontiguousarray(f)


def synthetic_weights(kind, seed):
    from autoware_vision_pilot_amd import synthetic, weights as vw

    make = {"autodrive": synthetic.make_autodrive_state_dict, "autospeed": synthetic.make_autospeed_state_dict, "autosteer": synthetic.make_autosteer_state_dict}.get(kind)
    return vw.pack_state_dict(make(seed) if make else synthetic.make_state_dict(kind, seed))


def merge(total, recs):
    """sum the counters of one frame's records into the running ones, keep the largest abs-max"""
    if total is None:
        return [dict(r, bins=r["bins"].copy()) for r in recs]
    for t, r in zip(total, recs):
        for k in ("count", "nonfinite", "zeros"):
            t[k] += r[k]
        t["bins"] += r["bins"]
        t["absmax"] = max(t["absmax"], r["absmax"])
    return total


def rows(kind, label, total):
    from autoware_vision_pilot_amd import lib

    for i, r in enumerate(total):
        if r["count"] == 0:
            continue
        s = lib.range_summary(r)
        yield "\t".join([kind, label, str(i), r["name"], str(r["c"]), str(r["h"]), str(r["w"]), str(r["exp"]), "%.6g" % float(r["absmax"]),
                         "" if s["headroom"] is None else str(s["headroom"]), str(r["nonfinite"]), str(r["zeros"]), str(r["count"]),
                         "%.4f" % s["below_lo_normal"], "%.4f" % s["below_hi_normal"]] + [str(int(b)) for b in r["bins"]])


def header():
    from autoware_vision_pilot_amd import lib

    return "\t".join(["kind", "weights", "tensor", "name", "c", "h", "w", "exp", "absmax", "headroom", "nonfinite", "zeros", "count", "below_0.125", "below_2^-14"] +
                     ["e%d" % (lib.VP_RANGE_EXP_MIN + k) for k in range(lib.VP_RANGE_BINS)])


def survey_frames(eng, kind, frames):
    """-> summed records; a frame that trips the range probe is surveyed like any other (that is what the report is for)"""
    from autoware_vision_pilot_amd import lib

    det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8) if kind == "autospeed" else None
    total = None
    try:
        for f in frames:
            if det is not None:
                try:
                    eng.infer_tensor(det.preprocess(f)[0])
                except lib.VpRangeError:
                    pass
            else:
                eng.upload_frame(f)
            total = merge(total, eng.range_survey())
    finally:
        if det is not None:
            det.close()
    return total


def main(argv=None):
    args = parse_args(argv)
    import torch  # noqa: F401  (first: one shared HIP runtime)

    from autoware_vision_pilot_amd import lib, synthetic

    seed = args.weight_seed if args.weight_seed is not None else SCENE_SEEDS.get(args.kind, 5)
    weights = args.weights if args.weights else synthetic_weights(args.kind, seed)
    label = os.path.basename(args.weights) if args.weights else f"seed{seed}"
    frames = [load_frame(p) for p in args.frames]
    h, w = args.frame_size or ((512, 1024) if args.kind == "autosteer" else (720, 1280))
    frames += [synthetic.synthetic_frame(h, w, s) for s in args.frame_seeds]
    if not frames:
        raise SystemExit("no frames: --frames FILE ... or --frame-seeds N ...")
    eng = lib.Engine(args.kind, weights, precision=args.precision, weights_fp8=args.weights_fp8, plan_latency=args.plan_latency)
    try:
        total = survey_frames(eng, args.kind, frames)
    finally:
        eng.close()
    if not args.no_header:
        print(header())
    for line in rows(args.kind, label, total):
        print(line)
    bad = next((r for r in total if r["count"] and r["nonfinite"]), None)
    if bad is not None:
        print(f"# first tensor in plan order with a non-finite value: {bad['name']} ({bad['nonfinite']} of {bad['count']} elements over {len(frames)} frame(s))")
    else:
        print(f"# no non-finite value in any stored tensor over {len(frames)} frame(s)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
