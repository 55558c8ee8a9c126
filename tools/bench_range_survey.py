#!/usr/bin/env python3
"""What the range survey costs on one MI355X (profiles/range_survey.txt).  Needs a GPU: there is no fall-back.

  python tools/bench_range_survey.py                    host-clock time of one vp_range_survey per kind (the call ends in a device synchronise), beside
                                                        the time of a plain vp_infer on the same frame
  python tools/bench_range_survey.py --trace-target     SceneSeg fp16x3: a few surveys and nothing else -- the program to run under
                                                        rocprofv3 --kernel-trace --output-format csv -d DIR
  python tools/bench_range_survey.py --from-trace DIR   reads that trace: per survey, act_exp_hist_kernel beside act_absmax_kernel on the same tensors --
                                                        the largest tensor (the pair of dispatches with the longest abs-max launch) and the sum over all

act_absmax_kernel reads the same bytes with the same loads and keeps two registers: it is the yardstick for the histogram."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

KINDS = ("sceneseg", "scene3d", "domainseg", "egolanes", "autodrive", "autospeed", "autosteer")
SURVEYS = 7


def from_trace(root):
    rows = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows.sort()
    amax = [(e - s) / 1e3 for s, e, n in rows if "act_absmax_kernel" in n]
    hist = [(e - s) / 1e3 for s, e, n in rows if "act_exp_hist_kernel" in n]
    if not amax or len(amax) != len(hist) or len(amax) % SURVEYS:
        raise SystemExit(f"trace under {root}: {len(amax)} abs-max and {len(hist)} histogram dispatches, expected equal counts over {SURVEYS} surveys")
    per = len(amax) // SURVEYS
    out = {"surveys_in_trace": SURVEYS, "stored_tensors_per_survey": per, "first_survey_left_out": "warm-up"}
    big, tot = [], []
    for k in range(1, SURVEYS):
        a, h = amax[k * per:(k + 1) * per], hist[k * per:(k + 1) * per]
        i = int(np.argmax(a))
        big.append((a[i], h[i]))
        tot.append((sum(a), sum(h)))
    out["largest_tensor_absmax_us_per_survey"] = [round(a, 1) for a, _ in big]
    out["largest_tensor_exp_hist_us_per_survey"] = [round(h, 1) for _, h in big]
    out["largest_tensor_ratio_hist_over_absmax"] = round(float(np.median([h for _, h in big]) / np.median([a for a, _ in big])), 3)
    out["all_tensors_absmax_us_per_survey"] = [round(a, 1) for a, _ in tot]
    out["all_tensors_exp_hist_us_per_survey"] = [round(h, 1) for _, h in tot]
    out["all_tensors_ratio_hist_over_absmax"] = round(float(np.median([h for _, h in tot]) / np.median([a for a, _ in tot])), 3)
    return out


def engine_for(lib, kind):
    """-> (engine, feed): BASELINE's weight seeds and the 720p frame for the scene networks, the golden files' seeds for the other kinds"""
    from autoware_vision_pilot_amd import synthetic

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import range_report

    eng = lib.Engine(kind, range_report.synthetic_weights(kind, range_report.SCENE_SEEDS.get(kind, 5)), precision="fp16x3")
    if kind == "autospeed":
        det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
        x = det.preprocess(synthetic.synthetic_frame(720, 1280, 21))[0]
        det.close()
        return eng, lambda: eng.infer_tensor(x)
    frame = synthetic.synthetic_frame(512, 1024, 22) if kind == "autosteer" else synthetic.synthetic_frame(720, 1280, 1)
    return eng, lambda: eng.infer(frame)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-target", action="store_true")
    ap.add_argument("--from-trace")
    args = ap.parse_args()
    if args.from_trace:
        print(json.dumps(from_trace(args.from_trace), indent=1))
        return
    import torch  # noqa: F401  (first: one shared HIP runtime)

    from autoware_vision_pilot_amd import lib

    if args.trace_target:
        eng, feed = engine_for(lib, "sceneseg")
        feed()
        for _ in range(SURVEYS):
            eng.range_survey()
        eng.close()
        return
    out = {"library": lib.version(), "protocol": "per kind, fp16x3: 3 warm-up calls, then the median of 20 calls on the host clock (each call ends in a device synchronise)"}
    for kind in KINDS:
        eng, feed = engine_for(lib, kind)
        t = {"infer": [], "survey": []}
        for name, call in (("infer", feed), ("survey", eng.range_survey)):
            for i in range(23):
                t0 = time.perf_counter()
                call()
                if i >= 3:
                    t[name].append((time.perf_counter() - t0) * 1e3)
        s = eng.range_survey()
        out[kind] = {"tensors": len(s), "stored": sum(1 for r in s if r["count"]), "elements_measured": int(sum(r["count"] for r in s)),
                     "vp_infer_ms_p50": round(float(np.median(t["infer"])), 3), "vp_range_survey_ms_p50": round(float(np.median(t["survey"])), 3)}
        eng.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
