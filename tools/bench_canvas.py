#!/usr/bin/env python3
"""What one vp_canvas per camera frame costs against the separate visualisation calls it replaces, on one MI355X.  1280 x 720, the metric configuration
(SceneSeg base with Scene3D and DomainSeg heads, fp16) and the detector.  The networks run ONCE, outside the timed loops: what is timed is the
visualisation step alone, host to host, one thread, in alternating rounds of
  separate : vp_visualize_mask_bgr8 on the base + vp_visualize_depth_bgr8 on the Scene3D head -- two pictures, each a host synchronisation and a
             full-frame D2H.  The DomainSeg head's overlay is NOT in it (the call refuses a head) and neither are the boxes (drawn on the host there);
  canvas   : vp_canvas_begin + paste_depth(Scene3D head) + blend_mask(base) + blend_mask(DomainSeg head) + draw_detections + ONE vp_canvas_fetch -- one
             picture that holds all four overlays -- fetched as BGR8, and in a second case as NV12.
Launches and bytes of each way are counted from the code paths (engine_io.cpp), not measured.  No ratio is promised: the figures say what was measured.
Needs a GPU.

python tools/bench_canvas.py > profiles/canvas.txt

--display: a leg of its own (the legs above do not run): the production app's display frame (production_release/main.cpp:881-907) on a 1920 x 1080 camera,
EgoLanes on the (0, 420, W, H - 420) crop and the detector on the whole frame, fp16, networks run once beforehand.  Alternating rounds, same protocol, of
  display : vp_canvas_begin + draw_detections + overlay_lanes + ONE vp_canvas_fetch_resized to 1280 x 720, as BGR8 and as NV12;
  full    : what the library could do before that call existed: begin + draw_detections + blend_mask(VP_VIZ_EGOLANES) + the full-size vp_canvas_fetch,
            as BGR8 and as NV12 -- another picture (the 50 / 50 label blend) at another size: the host's resize to the display size is NOT in it.
No speed threshold: the figures say what was measured.

python tools/bench_canvas.py --display >> profiles/canvas.txt"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (first: one shared HIP runtime)

from autoware_vision_pilot_amd import lib, synthetic, weights as vw
from oracle import weights

ROUNDS, WARM, TIMED = 3, 40, 300


def display_leg():
    Hc, Wc, Hd, Wd = 1080, 1920, 720, 1280
    crop = (0, 420, Wc, Hc - 420)
    ego = lib.Engine("egolanes", vw.pack_state_dict(weights.make_state_dict("egolanes", 2)), precision="fp16")
    ego.set_decode_mode(lib.VP_DECODE_LANE_LABEL)
    spd = lib.Engine("autospeed", vw.pack_state_dict(synthetic.make_autospeed_state_dict(0)), precision="fp16")
    det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
    det.attach(spd)
    frame, canvas = lib.Frame(), lib.Canvas()
    frame.upload(synthetic.synthetic_frame(Hc, Wc, 21), "bgr8")
    ego.infer_frame(frame, crop)
    rows, _ = det.infer_frame(frame, 0.05, 0.45)
    rows = np.concatenate([rows[:60], np.array([(100.4, 50.2, 400.9, 300.1, 0.9, 1), (20, 400, 300.5, 1000, 0.8, 2), (900, 410, 1919.9, 1079.9, 0.7, 3)], np.float32)])
    threshold = float(np.median(ego.logits()))     # about half of the lane samples on: the overlay has work everywhere

    def display(fmt):
        canvas.begin(frame)
        canvas.draw_detections(rows)
        canvas.overlay_lanes(ego, threshold)
        return canvas.fetch(fmt, size=(Hd, Wd))

    def full(fmt):
        canvas.begin(frame)
        canvas.draw_detections(rows)
        canvas.blend_mask(ego, lib.VP_VIZ_EGOLANES)
        return canvas.fetch(fmt)

    cases = (("full_bgr8", lambda: full("bgr8")), ("display_bgr8", lambda: display("bgr8")), ("full_nv12", lambda: full("nv12")), ("display_nv12", lambda: display("nv12")))
    box_launches = (len(rows) + 63) // 64
    px, pxd = Hc * Wc, Hd * Wd
    out = {"library": lib.version(),
           "protocol": f"{ROUNDS} rounds alternating the cases; per (case, round) {WARM} warm-up + {TIMED} timed pictures, one thread; p50 / p99 in us per call of the case, "
                       f"host to host; {Wc} x {Hc} camera, display {Wd} x {Hd}; networks run once beforehand (fp16: EgoLanes on the crop {crop}, AutoSpeed detector); "
                       f"{len(rows)} boxes",
           "cases": {"display_bgr8": "begin + draw_detections + overlay_lanes + fetch_resized(BGR8, 720, 1280): the production display frame",
                     "display_nv12": "the same, fetched as NV12",
                     "full_bgr8": "begin + draw_detections + blend_mask(VP_VIZ_EGOLANES) + fetch(BGR8) at the camera's size: another picture; the host's resize is not timed",
                     "full_nv12": "the same, fetched as NV12"},
           "counted_from_the_code": {
               "display_bgr8": {"kernel_launches": box_launches + 2, "host_synchronisations": 1, "d2h_bytes": 3 * pxd, "d2d_bytes": 3 * px},
               "display_nv12": {"kernel_launches": box_launches + 3, "host_synchronisations": 1, "d2h_bytes": 3 * pxd // 2, "d2d_bytes": 3 * px},
               "full_bgr8": {"kernel_launches": box_launches + 1, "host_synchronisations": 1, "d2h_bytes": 3 * px, "d2d_bytes": 3 * px},
               "full_nv12": {"kernel_launches": box_launches + 2, "host_synchronisations": 1, "d2h_bytes": 3 * px // 2, "d2d_bytes": 3 * px}}}
    res = {}
    for _ in range(ROUNDS):
        for name, fn in cases:
            for _ in range(WARM):
                fn()
            t = []
            for _ in range(TIMED):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e6)
            res.setdefault(name, {"p50": [], "p99": []})
            res[name]["p50"].append(round(float(np.percentile(t, 50)), 1))
            res[name]["p99"].append(round(float(np.percentile(t, 99)), 1))
    for name, r in res.items():
        out[f"{name}_p50_us_rounds"] = r["p50"]
        out[f"{name}_p99_us_rounds"] = r["p99"]
    print(json.dumps(out, indent=1))
    canvas.close()
    frame.close()
    det.close()
    ego.close()
    spd.close()


if "--display" in sys.argv[1:]:
    display_leg()
    sys.exit(0)

H, W = 720, 1280

sd_seg = weights.make_state_dict("sceneseg", 0)
base = lib.Engine("sceneseg", vw.pack_state_dict(sd_seg), precision="fp16")
s3d = lib.Engine("scene3d", vw.pack_state_dict(weights.share_backbone(weights.make_state_dict("scene3d", 1), "scene3d", sd_seg, "sceneseg")), precision="fp16", base=base)
dom = lib.Engine("domainseg", vw.pack_state_dict(weights.share_backbone(weights.make_state_dict("domainseg", 3), "domainseg", sd_seg, "sceneseg", also_context_neck=True)),
                 precision="fp16", base=base)
spd = lib.Engine("autospeed", vw.pack_state_dict(synthetic.make_autospeed_state_dict(0)), precision="fp16")
det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
det.attach(spd)
frame, canvas = lib.Frame(), lib.Canvas()

bgr = synthetic.synthetic_frame(H, W, 21)
frame.upload(bgr, "bgr8")
base.infer_frame(frame)
s3d.infer_shared()
dom.infer_shared()
rows, _ = det.infer_frame(frame, 0.05, 0.45)
rows = np.concatenate([rows[:60], np.array([(100.4, 50.2, 400.9, 300.1, 0.9, 1), (20, 400, 300.5, 700, 0.8, 2), (900, 410, 1279.9, 719.9, 0.7, 3)], np.float32)])


def separate():
    base.visualize_mask(lib.VP_VIZ_SCENE, (H, W))
    s3d.visualize_depth(H, W)


def compose(fmt):
    canvas.begin(frame)
    canvas.paste_depth(s3d)
    canvas.blend_mask(base, lib.VP_VIZ_SCENE)
    canvas.blend_mask(dom, lib.VP_VIZ_DOMAIN)
    canvas.draw_detections(rows)
    return canvas.fetch(fmt)


CASES = (("separate", separate), ("canvas_bgr8", lambda: compose("bgr8")), ("canvas_nv12", lambda: compose("nv12")))
px = H * W
out = {"library": lib.version(),
       "protocol": f"{ROUNDS} rounds alternating the cases; per (case, round) {WARM} warm-up + {TIMED} timed pictures, one thread; p50 / p99 in us per call of the case, "
                   f"host to host; {W} x {H}; networks run once beforehand (fp16: SceneSeg base, Scene3D + DomainSeg heads, AutoSpeed detector); {len(rows)} boxes",
       "cases": {"separate": "vp_visualize_mask_bgr8(base) + vp_visualize_depth_bgr8(Scene3D head): 2 pictures, 2 overlays, no DomainSeg overlay, no boxes",
                 "canvas_bgr8": "begin + paste_depth + 2 x blend_mask + draw_detections + fetch(BGR8): 1 picture, 4 overlays",
                 "canvas_nv12": "the same, fetched as NV12"},
       "counted_from_the_code": {
           "separate": {"kernel_launches": 4, "small_h2d_copies": 4, "host_synchronisations": 2, "d2h_bytes": 2 * 3 * px, "d2d_bytes": 0},
           "canvas_bgr8": {"kernel_launches": 5 + (len(rows) + 63) // 64, "small_h2d_copies": 0, "host_synchronisations": 1, "d2h_bytes": 3 * px, "d2d_bytes": 3 * px + 8},
           "canvas_nv12": {"kernel_launches": 6 + (len(rows) + 63) // 64, "small_h2d_copies": 0, "host_synchronisations": 1, "d2h_bytes": 3 * px // 2, "d2d_bytes": 3 * px + 8}}}
res = {}
for rnd in range(ROUNDS):
    for name, fn in CASES:
        for _ in range(WARM):
            fn()
        t = []
        for _ in range(TIMED):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        res.setdefault(name, {"p50": [], "p99": []})
        res[name]["p50"].append(round(float(np.percentile(t, 50)), 1))
        res[name]["p99"].append(round(float(np.percentile(t, 99)), 1))
for name, r in res.items():
    out[f"{name}_p50_us_rounds"] = r["p50"]
    out[f"{name}_p99_us_rounds"] = r["p99"]
ref = float(np.median(res["separate"]["p50"]))
for name in ("canvas_bgr8", "canvas_nv12"):
    out[f"{name}_p50_over_separate"] = round(float(np.median(res[name]["p50"])) / ref, 4)
# where the time goes: the device part of the canvas way (everything but the fetch), and the fetch alone
for name, fn in (("canvas_draws_only", lambda: (canvas.begin(frame), canvas.paste_depth(s3d), canvas.blend_mask(base, 0), canvas.blend_mask(dom, 1), canvas.draw_detections(rows),
                                                 canvas.sync())), ("canvas_fetch_bgr8_only", lambda: canvas.fetch("bgr8")), ("canvas_fetch_nv12_only", lambda: canvas.fetch("nv12"))):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(TIMED):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    out[f"{name}_p50_us"] = round(float(np.percentile(t, 50)), 1)
print(json.dumps(out, indent=1))
canvas.close()
frame.close()
det.close()
for e in (s3d, dom, base, spd):
    e.close()
