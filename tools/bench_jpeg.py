#!/usr/bin/env python3
"""What vp_canvas_fetch_jpeg costs against the uncompressed fetches and a host JPEG encoder, on one MI355X.  Canvases of 1280 x 720 and 640 x 320 with
two label masks drawn (vp_canvas_blend_mask_u8; drawn ONCE, outside the timed loops: what is timed is the fetch alone, host to host, one thread).  Per
canvas, in alternating rounds:
  fetch_jpeg(q, Ri)   q in {75, 90}, Ri in {1, 2, 4, 8}: the stream in host memory;
  fetch(BGR8), fetch(NV12): the same canvas's uncompressed fetches (the code path these had before the encoder existed; it is untouched);
  pillow(q)           PIL.Image.save(.., "JPEG", quality=q, subsampling=2) of the fetched picture on the host (RGB order prepared outside the timing):
                      libjpeg-turbo on one thread, standing for the libjpeg behind cv2.VideoWriter(.., "MJPG").write(frame).
Stream bytes are recorded against Pillow's.  Per-kernel device times come from a second process under `rocprofv3 --kernel-trace` (--kernels; skipped with
a note when the profiler is not there).  No speed threshold: the figures say what was measured.  Needs a GPU.

python tools/bench_jpeg.py --kernels > profiles/canvas_jpeg.txt"""
import csv
import glob
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (first: one shared HIP runtime)
from PIL import Image

from autoware_vision_pilot_amd import lib, synthetic

ROUNDS, WARM, TIMED = 3, 20, 100
SIZES = ((720, 1280), (320, 640))
QUALITIES = (75, 90)
RIS = (1, 2, 4, 8)
TRACE_CALLS = 20
KERNELS = ("jpeg_blocks_kernel", "jpeg_entropy_kernel<false>", "jpeg_scan_kernel", "jpeg_entropy_kernel<true>")   # a fetch's four launches, in order


def drawn_canvas(h, w):
    frame, canvas = lib.Frame(), lib.Canvas()
    frame.upload(synthetic.synthetic_frame(h, w, 21), "bgr8")
    canvas.begin(frame)
    rng = np.random.default_rng(5)
    for viz in (lib.VP_VIZ_SCENE, lib.VP_VIZ_DOMAIN):       # blocky label masks at a network's size, as an engine's would be
        mask = np.kron(rng.integers(0, 3, size=(10, 20), dtype=np.uint8), np.ones((32, 32), np.uint8))
        canvas.blend_mask_u8(mask, viz, (0, 0, w, h))
    canvas.sync()
    return frame, canvas


def timed(fn):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(TIMED):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return round(float(np.percentile(t, 50)), 1), round(float(np.percentile(t, 99)), 1)


def trace_child():
    """the fetches alone, in a fixed order, for the profiler: per size, quality and Ri TRACE_CALLS calls"""
    for h, w in SIZES:
        frame, canvas = drawn_canvas(h, w)
        for q in QUALITIES:
            for ri in RIS:
                for _ in range(TRACE_CALLS):
                    canvas.fetch_jpeg(q, ri)
        canvas.close()
        frame.close()


def kernel_times():
    """{config: {kernel: median us}} from a run of trace_child under rocprofv3, or a note why not"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return {"note": "rocprofv3 not found: per-kernel times not measured"}
    out = tempfile.mkdtemp(prefix="vp_jpeg_trace_")
    try:
        r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--trace-child"],
                           capture_output=True, text=True, timeout=600)
        rows = []
        for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
            with open(f) as fh:
                rows += [(int(x["Start_Timestamp"]), int(x["End_Timestamp"]), x["Kernel_Name"]) for x in csv.DictReader(fh)]
        rows = sorted(x for x in rows if "jpeg_" in x[2])
        configs = [(h, w, q, ri) for h, w in SIZES for q in QUALITIES for ri in RIS]
        if r.returncode != 0 or len(rows) != 4 * TRACE_CALLS * len(configs):
            return {"note": f"profiler run unusable (status {r.returncode}, {len(rows)} jpeg dispatches, {4 * TRACE_CALLS * len(configs)} expected): per-kernel times not measured"}
        res = {}
        for i, (h, w, q, ri) in enumerate(configs):
            part = rows[4 * TRACE_CALLS * i:4 * TRACE_CALLS * (i + 1)]
            entry = {}
            for k, name in enumerate(KERNELS):
                mine = part[k::4]
                assert all(name.split("<")[0] in x[2] for x in mine), (name, mine[0][2])
                entry[name] = round(float(np.median([(e - s) / 1e3 for s, e, _ in mine])), 1)
            entry["first_launch_start_to_last_end"] = round(float(np.median([(part[4 * j + 3][1] - part[4 * j][0]) / 1e3 for j in range(TRACE_CALLS)])), 1)
            res[f"{w}x{h} q{q} Ri{ri}"] = entry
        return res
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    out = {"library": lib.version(), "pillow": Image.__version__,
           "protocol": f"{ROUNDS} rounds alternating the cases; per (case, round) {WARM} warm-up + {TIMED} timed calls, one thread; p50 in us per call, host to host, "
                       f"median of the rounds (p99: the largest of the rounds); masks drawn once beforehand",
           "default_restart_mcus": int.from_bytes(lib.jpeg_header(16, 16, 75, 0)[-16:-14], "big")}   # the DRI segment's value, just ahead of SOS
    for h, w in SIZES:
        frame, canvas = drawn_canvas(h, w)
        bgr = canvas.fetch("bgr8")
        rgb = np.ascontiguousarray(bgr[..., ::-1])
        pil = Image.fromarray(rgb)

        def pillow(q):
            buf = io.BytesIO()
            pil.save(buf, "JPEG", quality=q, subsampling=2)
            return buf.getvalue()

        cases = [("fetch_bgr8", lambda: canvas.fetch("bgr8")), ("fetch_nv12", lambda: canvas.fetch("nv12"))]
        for q in QUALITIES:
            cases.append((f"pillow_q{q}", lambda q=q: pillow(q)))
            for ri in RIS:
                cases.append((f"fetch_jpeg_q{q}_ri{ri}", lambda q=q, ri=ri: canvas.fetch_jpeg(q, ri)))
        res = {}
        for _ in range(ROUNDS):
            for name, fn in cases:
                p50, p99 = timed(fn)
                res.setdefault(name, ([], []))
                res[name][0].append(p50)
                res[name][1].append(p99)
        size = {"p50_us": {k: float(np.median(v[0])) for k, v in res.items()}, "p99_us": {k: float(np.max(v[1])) for k, v in res.items()}, "bytes": {}}
        size["bytes"]["bgr8"], size["bytes"]["nv12"] = 3 * h * w, 3 * h * w // 2
        for q in QUALITIES:
            size["bytes"][f"pillow_q{q}"] = len(pillow(q))
            for ri in RIS:
                size["bytes"][f"fetch_jpeg_q{q}_ri{ri}"] = len(canvas.fetch_jpeg(q, ri))
            for ri in RIS:
                size["bytes"][f"q{q}_ri{ri}_over_ri8"] = round(size["bytes"][f"fetch_jpeg_q{q}_ri{ri}"] / size["bytes"][f"fetch_jpeg_q{q}_ri8"], 4)
            size["p50_us"][f"fetch_bgr8_plus_pillow_q{q}"] = round(size["p50_us"]["fetch_bgr8"] + size["p50_us"][f"pillow_q{q}"], 1)
        decoded = np.asarray(Image.open(io.BytesIO(canvas.fetch_jpeg(90, 0))).convert("RGB")).astype(np.float64)
        size["psnr_db_q90_against_the_picture"] = round(float(10 * np.log10(255.0 ** 2 / np.mean((decoded - rgb) ** 2))), 2)
        out[f"{w}x{h}"] = size
        canvas.close()
        frame.close()
    if "--kernels" in sys.argv[1:]:
        out["kernel_us_median_of_%d" % TRACE_CALLS] = kernel_times()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if "--trace-child" in sys.argv[1:]:
        trace_child()
    else:
        main()
