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
other three standards (the constants are kernel parameters: a standard should cost nothing).

python tools/bench_frame.py --rectify > profiles/frame_rectify.txt: what vp_frame_set_rectify adds to an upload.  One 1920 x 1080 frame, NV12 and BGR8, taken
from DEVICE planes (vp_frame_upload_device: no H2D in the figure), rectified to the 1024 x 512 standard pose under a mild distortion, two-pass and
one-pass, next to the same upload without the setting.  The frame's stream is not visible across the C boundary, so no event can be recorded on it.
The device time per upload is taken behind a GATE instead: the first upload of a round names a producer stream that is busy with tens of milliseconds
of matrix products, the host queues N uploads while the frame's stream waits for that stream's event, and the host clock runs from the gate's
completion to vp_frame_sync -- the device then runs the N uploads back to back, and the quotient holds no host time (the tool checks that the gate
was still closed when the last upload was queued).  Bytes of the passes, from shapes: source picture read + map read (8 bytes an entry) + picture
written.

python tools/bench_frame.py --raw: the conversion of the upload-only formats next to NV12 in one run.  One 1920 x 1080 frame from device planes behind the
same gate: NV12 (the yardstick), RGGB8, RGGB12 in 16-bit words under the default raw setting and under black + gains + ccm + a 4096-entry LUT, P010 and
GRAY16; device time per upload, the bytes moved (source planes + 3 bytes a pixel) and the resulting GB/s.  Recorded in profiles/frame_raw.txt."""
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


class Gate:
    """tens of milliseconds of matrix products on a producer stream: the frame's stream waits behind its event while the host queues uploads"""

    def __init__(self, matmuls=6):
        self.stream = torch.cuda.Stream()
        self.a = torch.randn(8192, 8192, device="cuda")
        self.matmuls = matmuls
        torch.cuda.synchronize()
        self.close()
        self.stream.synchronize()

    def close(self):
        with torch.cuda.stream(self.stream):
            for _ in range(self.matmuls):
                self.a @ self.a

    def timed_uploads(self, f, ptrs, strides, fmt, h, w, rounds, queued):
        """per round: (host clock from the gate's completion to vp_frame_sync) / uploads and host time per upload call, in us; whether the gate was still
        closed when the last upload was queued in every round"""
        t, enq, held = [], [], True
        for _ in range(rounds):
            self.close()
            t0 = time.perf_counter()
            f.upload_device(ptrs, strides, fmt, h, w, producer_stream=self.stream.cuda_stream)
            for _ in range(queued - 1):
                f.upload_device(ptrs, strides, fmt, h, w)
            enq.append((time.perf_counter() - t0) * 1e6 / queued)
            held = held and not self.stream.query()
            self.stream.synchronize()
            t1 = time.perf_counter()
            f.sync()
            t.append((time.perf_counter() - t1) * 1e6 / queued)
        return t, enq, held


def rectify_leg(h=1080, w=1920, out_hw=(512, 1024), rounds=5, queued=300, gate_matmuls=6):
    K = np.array([[1400.0, 0.0, 960.0], [0.0, 1400.0, 540.0], [0.0, 0.0, 1.0]])
    dist = (-0.08, 0.01, 0.0005, -0.0003, 0.0)
    H = lib.rectify_homography({"pitch": 1.5, "yaw": -0.8, "roll": 0.4, "camera_height": 1.6, "intrinsic_matrix": K},
                               {"pitch": 0.0, "yaw": 0.0, "roll": 0.0, "camera_height": 1.45, "img_width": out_hw[1], "img_height": out_hw[0], "hfov": 70.0})
    bgr = synthetic.synthetic_frame(h, w, 21)
    nv12, _ = yuv_planes(bgr)
    dev = {"nv12": [torch.from_numpy(p).cuda() for p in nv12], "bgr8": [torch.from_numpy(bgr.reshape(h, 3 * w)).cuda()]}
    gate = Gate(gate_matmuls)
    oh, ow = out_hw
    raw, out = 3 * h * w, 3 * oh * ow
    pass_bytes = {"off": 0, "two_pass": (raw + 8 * h * w + raw) + (raw + 8 * oh * ow + out), "one_pass": raw + 8 * oh * ow + out}
    res = {"library": lib.version(),
           "protocol": f"vp_frame_upload_device of one {w} x {h} frame from device planes, rectified to {ow} x {oh}; per case {rounds} rounds; a round queues {queued} "
                       "uploads while the frame's stream waits for the producer stream's event behind a gate of matrix products, so the device runs them back to "
                       "back; us_per_upload = (host clock from the gate's completion to vp_frame_sync) / uploads, median, min and max of the rounds; "
                       "gate_held = the gate was still closed when the last upload was queued in every round (false: the figure holds host time and is "
                       "only an upper bound); enqueue_us = host time per upload call; passes_GBps = bytes of the passes (source read + map read + picture "
                       "written, from shapes) / (us_per_upload - that of the same upload without the setting)",
           "K": K.reshape(-1).tolist(), "dist": list(dist), "H": H.reshape(-1).tolist(), "pass_bytes": pass_bytes}
    f = lib.Frame()
    for fmt, planes in dev.items():
        ptrs, strides = [p.data_ptr() for p in planes], [p.stride(0) for p in planes]
        base = None
        for mode in ("off", "two_pass", "one_pass"):
            f.set_rectify(None) if mode == "off" else f.set_rectify(K, dist, H, out_hw, mode)
            for _ in range(20):   # the maps are built in the first of these
                f.upload_device(ptrs, strides, fmt, h, w)
            f.sync()
            t, enq, held = gate.timed_uploads(f, ptrs, strides, fmt, h, w, rounds, queued)
            us = float(np.median(t))
            rec = {"us_per_upload": round(us, 2), "min": round(min(t), 2), "max": round(max(t), 2), "gate_held": held, "enqueue_us": round(float(np.median(enq)), 2),
                   "picture_hw": list(f.hw())}
            if mode == "off":
                base = us
            else:
                rec["us_over_off"] = round(us - base, 2)
                rec["passes_GBps"] = round(pass_bytes[mode] / ((us - base) * 1e-6) / 1e9, 1) if us > base else None
            res[f"{fmt}_{mode}"] = rec
    f.close()
    print(json.dumps(res, indent=1))


def raw_leg(h=1080, w=1920, rounds=5, queued=300):
    def mosaic(rgb):   # RGGB
        raw = rgb[:, :, 1].copy()
        raw[0::2, 0::2] = rgb[0::2, 0::2, 0]
        raw[1::2, 1::2] = rgb[1::2, 1::2, 2]
        return raw

    bgr = synthetic.synthetic_frame(h, w, 21)
    nv12, _ = yuv_planes(bgr)
    raw8 = mosaic(bgr[:, :, ::-1])
    raw12 = (raw8.astype(np.uint16) << 4) | (raw8 >> 4)                  # 12 significant bits in 16-bit words
    p010 = [p.astype(np.uint16) << 8 for p in nv12]                       # MSB-aligned
    n = np.arange(4096) / 4095.0
    full = {"bits": 12, "black": 256, "gains": (520, 256, 410), "ccm": (1434, -307, -103, -205, 1331, -102, 51, -410, 1383),
            "lut": np.round(255.0 * n ** (1 / 2.2)).astype(np.uint8)}
    # (leg, format, planes, raw setting, source bytes a pixel)
    legs = (("nv12", "nv12", nv12, None, 1.5), ("rggb8", "bayer_rggb8", [raw8], {}, 1.0), ("rggb12", "bayer_rggb16", [raw12], {"bits": 12}, 2.0),
            ("rggb12_black_gains_ccm_lut", "bayer_rggb16", [raw12], full, 2.0), ("p010", "p010", p010, None, 3.0), ("gray16", "gray16", [p010[0]], None, 2.0))
    gate = Gate()
    res = {"library": lib.version(),
           "protocol": f"vp_frame_upload_device of one {w} x {h} frame from device planes; per leg {rounds} rounds; a round queues {queued} uploads while the frame's "
                       "stream waits for the producer stream's event behind a gate of matrix products, so the device runs them back to back; us_per_upload = (host "
                       "clock from the gate's completion to vp_frame_sync) / uploads, median, min and max of the rounds; gate_held = the gate was still closed when "
                       "the last upload was queued in every round; bytes = source planes read + 3 bytes a pixel written, from shapes; GBps = bytes / us_per_upload"}
    f = lib.Frame()
    for leg, fmt, planes, setting, src_px in legs:
        dev = [torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(p.shape[0], -1)).cuda() for p in planes]
        ptrs, strides = [p.data_ptr() for p in dev], [p.stride(0) for p in dev]
        if setting is not None:
            f.set_raw(**setting)
        for _ in range(20):
            f.upload_device(ptrs, strides, fmt, h, w)
        f.sync()
        t, enq, held = gate.timed_uploads(f, ptrs, strides, fmt, h, w, rounds, queued)
        us = float(np.median(t))
        moved = int((src_px + 3.0) * h * w)
        res[leg] = {"us_per_upload": round(us, 2), "min": round(min(t), 2), "max": round(max(t), 2), "gate_held": held, "enqueue_us": round(float(np.median(enq)), 2),
                    "bytes": moved, "GBps": round(moved / (us * 1e-6) / 1e9, 1)}
    f.close()
    print(json.dumps(res, indent=1))


if "--raw" in sys.argv[1:]:
    raw_leg()
    sys.exit(0)

if "--rectify" in sys.argv[1:]:
    rectify_leg()
    sys.exit(0)

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
