#!/usr/bin/env python3
"""What one vp_frame for three networks saves on one MI355X.  The production application's trio on one camera frame (VisionPilot/production_release/
main.cpp): EgoLanes on the crop rows >= 420, AutoSpeed (detector) on the whole frame, SceneSeg on the whole frame; fp16 engines, latency plan.  One
process, alternating rounds on 1280 x 720 and 1920 x 1080 frames; p50 host to host PER FRAME (all three results on the host) of
  (a)  today's three entries on a host BGR8 buffer: vp_infer(crop view), vp_detect_infer, vp_infer -- the yardstick;
  (b)  one vp_frame_upload of the BGR8 buffer + vp_infer_frame, vp_detect_infer_frame, vp_infer_frame;
  (c)  the same from an NV12 and from a YUY2 buffer (no CPU colour conversion ahead of the boundary; what that conversion costs the host is NOT in (a)).
Each in two host shapes, one thread either way: "serial" -- one synchronous call after the other -- and "overlap" -- the two scene engines uploaded and
enqueued first (vp_upload_frame / vp_upload_from_frame + vp_enqueue), the detector's synchronous call, then vp_fetch_outputs twice -- so the three
networks share the GPU as the application's threads make them.  No ratio is promised: the figures say what was measured.  Needs a GPU.

python tools/bench_frame.py > profiles/frame_fanout.txt

python tools/bench_frame.py --convert: the upload leg alone, no engines -- vp_frame_upload + vp_frame_sync (staging copy, H2D, conversion kernel) of one
1280 x 720 frame from pageable host memory, p50 / p99 host to host, for every YUV format at the default colour standard and for NV12 / I420 under the
other three standards (the constants are kernel parameters: a standard should cost nothing)."""
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
SIZES = ((720, 1280), (1080, 1920))
CROP_Y = 420
CONF, IOU = 0.4, 0.65


def yuv_planes(bgr):
    """forward BT.601 (rounded) of a BGR frame: (NV12 planes, YUY2 plane) a camera would have delivered"""
    b, g, r = (bgr[:, :, i].astype(np.int64) for i in range(3))
    Y = np.clip((66 * r + 129 * g + 25 * b + 128) // 256 + 16, 0, 255).astype(np.uint8)
    U = np.clip((-38 * r - 74 * g + 112 * b + 128) // 256 + 128, 0, 255).astype(np.uint8)
    V = np.clip((112 * r - 94 * g - 18 * b + 128) // 256 + 128, 0, 255).astype(np.uint8)
    h, w = Y.shape
    nv12 = [np.ascontiguousarray(Y), np.ascontiguousarray(np.stack([U[0::2, 0::2], V[0::2, 0::2]], axis=2).reshape(h // 2, w))]
    yuy2 = [np.ascontiguousarray(np.stack([Y[:, 0::2], U[:, 0::2], Y[:, 1::2], V[:, 0::2]], axis=2).reshape(h, 2 * w))]
    return nv12, yuy2


def convert_leg(h=720, w=1280, warm=50, timed=500):
    bgr = synthetic.synthetic_frame(h, w, 21)
    nv12, yuy2 = yuv_planes(bgr)
    y, uv = nv12[0], nv12[1].reshape(h // 2, w // 2, 2)
    u, v = np.ascontiguousarray(uv[:, :, 0]), np.ascontiguousarray(uv[:, :, 1])
    q = yuy2[0].reshape(h, w // 2, 4)
    sources = {"nv12": nv12, "nv21": [y, np.ascontiguousarray(uv[:, :, ::-1]).reshape(h // 2, w)], "i420": [y, u, v], "yv12": [y, v, u], "yuy2": yuy2,
               "uyvy": [np.ascontiguousarray(q[:, :, [1, 0, 3, 2]]).reshape(h, 2 * w)], "bgr8": [bgr.reshape(h, 3 * w)]}
    default = ("bt601", "limited")
    cases = [(fmt, default) for fmt in sources] + [(fmt, std) for fmt in ("nv12", "i420") for std in (("bt601", "full"), ("bt709", "limited"), ("bt709", "full"))]
    res = {"library": lib.version(), "protocol": f"vp_frame_upload + vp_frame_sync of one {w} x {h} frame from pageable host memory; per case {warm} warm-up + {timed} "
                                                 "timed uploads, one thread, one process; p50 / p99 in us host to host"}
    f = lib.Frame()
    for fmt, std in cases:
        f.set_color(*std)
        src = sources[fmt]
        for _ in range(warm):
            f.upload(src, fmt, hw=(h, w))
            f.sync()
        t = []
        for _ in range(timed):
            t0 = time.perf_counter()
            f.upload(src, fmt, hw=(h, w))
            f.sync()
            t.append((time.perf_counter() - t0) * 1e6)
        res[f"{w}x{h}_upload_{fmt}_{std[0]}_{std[1]}_us"] = {"p50": round(float(np.percentile(t, 50)), 1), "p99": round(float(np.percentile(t, 99)), 1)}
    f.close()
    print(json.dumps(res, indent=1))


if "--convert" in sys.argv[1:]:
    convert_leg()
    sys.exit(0)

ego = lib.Engine("egolanes", vw.pack_state_dict(weights.make_state_dict("egolanes", 2)), precision="fp16", plan_latency=True)
seg = lib.Engine("sceneseg", vw.pack_state_dict(weights.make_state_dict("sceneseg", 0)), precision="fp16", plan_latency=True)
spd = lib.Engine("autospeed", vw.pack_state_dict(synthetic.make_autospeed_state_dict(0)), precision="fp16", plan_latency=True)
det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
det.attach(spd)
frame = lib.Frame()


def host_serial(bgr, _):
    ego.infer(bgr[CROP_Y:])
    det.infer(bgr, CONF, IOU)
    seg.infer(bgr)


def host_overlap(bgr, _):
    ego.upload_frame(bgr[CROP_Y:])
    ego.enqueue()
    seg.upload_frame(bgr)
    seg.enqueue()
    det.infer(bgr, CONF, IOU)
    ego.fetch_outputs()
    seg.fetch_outputs()


def frame_serial(src, fmt):
    frame.upload(src, fmt, hw=(H, W))
    ego.infer_frame(frame, (0, CROP_Y, W, H - CROP_Y))
    det.infer_frame(frame, CONF, IOU)
    seg.infer_frame(frame)


def frame_overlap(src, fmt):
    frame.upload(src, fmt, hw=(H, W))
    ego.upload_from_frame(frame, (0, CROP_Y, W, H - CROP_Y))
    ego.enqueue()
    seg.upload_from_frame(frame)
    seg.enqueue()
    det.infer_frame(frame, CONF, IOU)
    ego.fetch_outputs()
    seg.fetch_outputs()


out = {"library": lib.version(),
       "protocol": f"{ROUNDS} rounds alternating the frame sizes; per (size, case, round) {WARM} warm-up + {TIMED} timed frames, one thread; p50 / p99 in us per frame, "
                   "all three results on the host; fp16 engines, latency plan; EgoLanes on rows >= 420, AutoSpeed and SceneSeg on the whole frame",
       "cases": {"a": "vp_infer + vp_detect_infer + vp_infer on a host BGR8 buffer (yardstick)", "b": "vp_frame_upload(BGR8) + three consumers",
                 "c_nv12": "vp_frame_upload(NV12) + three consumers", "c_yuy2": "vp_frame_upload(YUY2) + three consumers"}}
res = {}
for rnd in range(ROUNDS):
    for H, W in SIZES:
        h, w = H, W
        bgr = synthetic.synthetic_frame(h, w, 21)
        nv12, yuy2 = yuv_planes(bgr)
        for shape, host_fn, frame_fn in (("serial", host_serial, frame_serial), ("overlap", host_overlap, frame_overlap)):
            for case, fn, src, fmt in (("a", host_fn, bgr, None), ("b", frame_fn, [bgr.reshape(h, 3 * w)], "bgr8"), ("c_nv12", frame_fn, nv12, "nv12"),
                                       ("c_yuy2", frame_fn, yuy2, "yuy2")):
                for _ in range(WARM):
                    fn(src, fmt)
                t = []
                for _ in range(TIMED):
                    t0 = time.perf_counter()
                    fn(src, fmt)
                    t.append((time.perf_counter() - t0) * 1e6)
                key = f"{w}x{h}_{case}_{shape}"
                res.setdefault(key, {"p50": [], "p99": []})
                res[key]["p50"].append(round(float(np.percentile(t, 50)), 1))
                res[key]["p99"].append(round(float(np.percentile(t, 99)), 1))
for key, r in res.items():
    out[f"{key}_p50_us_rounds"] = r["p50"]
    out[f"{key}_p99_us_rounds"] = r["p99"]
for h, w in SIZES:
    for shape in ("serial", "overlap"):
        base = float(np.median(res[f"{w}x{h}_a_{shape}"]["p50"]))
        for case in ("b", "c_nv12", "c_yuy2"):
            out[f"{w}x{h}_{case}_{shape}_p50_over_a"] = round(float(np.median(res[f"{w}x{h}_{case}_{shape}"]["p50"])) / base, 4)
print(json.dumps(out, indent=1))
frame.close()
det.close()
for e in (ego, seg, spd):
    e.close()
