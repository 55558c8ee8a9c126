#!/usr/bin/env python3
"""What building the ground truth on the device costs and saves, on one MI355X: vp_metric_add_seg_label and vp_metric_add_depth_label on a 1920 x 1080
label (the ACDC box (0, 0, 1919, 990) for the colour label) against a resident engine pass (fp16 SceneSeg / Scene3D, synthetic weights), held against the
way of the commit before them: a VECTORISED numpy preparation of the same ground truth and statistics on the host, then vp_metric_add_seg / _add_depth.

Per sample, for either way:
  host to host   one sample alone: the call(s), then vp_metric_fetch -- what a loop that looks at every score pays;
  in stream      SAMPLES samples queued back to back, one vp_metric_fetch at the end, divided by SAMPLES -- what a dataset run pays.
The two ways take turns over ROUNDS rounds in one process (the protocol of tools/bench_act_scale_nets.py); the figures are the rounds' values and their
median.  The reference's own preparation is a per-pixel Python loop; a restatement of that loop is timed ONCE on the same crop and reported apart.
Needs a GPU: there is no fall-back.

python tools/bench_label.py > profiles/label.txt"""
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

H, W, BOX = 1080, 1920, (0, 0, 1919, 990)
ROUNDS, WARM, ALONE, SAMPLES = 3, 3, 10, 20


def nearest_index(src, dst):
    ifx = np.float64(1.0) / (np.float64(dst) / np.float64(src))
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * ifx).astype(np.int64), src - 1)


def host_colour(label, box, out_hw):
    """the vectorised host way: crop (the box lies inside this label), classify the full-resolution crop once, count, sample"""
    crop = label[box[1]:box[3], box[0]:box[2]]
    key = crop[..., 0].astype(np.uint32) | crop[..., 1].astype(np.uint32) << 8 | crop[..., 2].astype(np.uint32) << 16
    cls = np.full(key.shape, 255, np.uint8)
    for r, g, b, c in lib.SCENESEG_COLOURS[::-1].astype(np.uint32):
        cls[key == (r | g << 8 | b << 16)] = c
    freq = np.bincount(cls.reshape(-1), minlength=256)[:3]
    gt = cls[nearest_index(cls.shape[0], out_hw[0])][:, nearest_index(cls.shape[1], out_hw[1])]
    return np.ascontiguousarray(gt), freq


def host_depth(v, out_hw):
    g = (v - np.min(v)) / (np.max(v) - np.min(v))
    return np.ascontiguousarray(g[nearest_index(v.shape[0], out_hw[0])][:, nearest_index(v.shape[1], out_hw[1])], dtype=np.float32)


def python_loop(label, box):
    """a restatement of the per-pixel loop's shape: every pixel of the crop against the nine colours, three counters"""
    table = {tuple(int(v) for v in row[:3]): int(row[3]) for row in lib.SCENESEG_COLOURS}
    rows = label[box[1]:box[3], box[0]:box[2]].tolist()
    freq = [0, 0, 0]
    planes = [bytearray(len(rows) * len(rows[0])) for _ in range(3)]
    i = 0
    for row in rows:
        for px in row:
            c = table.get(tuple(px))
            if c is not None:
                planes[c][i] = 255
                freq[c] += 1
            i += 1
    return freq


def measure(ways, m):
    """ways: name -> callable that queues one sample; per round and way: host-to-host microseconds (median of ALONE) and in-stream microseconds per sample"""
    res = {name: {"alone": [], "stream": []} for name in ways}
    for _ in range(ROUNDS):
        for name, add in ways.items():
            for _ in range(WARM):
                add()
            m.fetch()
            m.reset()
            t = []
            for _ in range(ALONE):
                t0 = time.perf_counter()
                add()
                m.fetch()
                t.append((time.perf_counter() - t0) * 1e6)
            m.reset()
            res[name]["alone"].append(round(float(np.median(t)), 1))
            t0 = time.perf_counter()
            for _ in range(SAMPLES):
                add()
            m.fetch()
            res[name]["stream"].append(round((time.perf_counter() - t0) / SAMPLES * 1e6, 1))
            m.reset()
    return res


def main():
    rng = np.random.default_rng(5)
    label = lib.SCENESEG_COLOURS[rng.integers(0, 9, (H // 8, W // 8)), :3].repeat(8, axis=0).repeat(8, axis=1)   # 8 x 8 patches of the nine colours
    label = np.ascontiguousarray(label)
    depth32 = (rng.random((H, W)) * 80.0 + 0.5).astype(np.float32)
    depth64 = depth32.astype(np.float64)
    frame = synthetic.synthetic_frame(360, 640, 21)
    seg = lib.Engine("sceneseg", vw.pack_state_dict(weights.make_state_dict("sceneseg", 0)), precision="fp16")
    d3 = lib.Engine("scene3d", vw.pack_state_dict(weights.make_state_dict("scene3d", 1)), precision="fp16")
    seg.infer(frame)
    d3.infer(frame)
    out_hw = tuple(seg.output_dims()[-2:])
    m = lib.Metric(max_frames=64)
    out = {"library": lib.version(), "label": f"{W} x {H}, colour box {BOX}, ground truth {out_hw[1]} x {out_hw[0]}",
           "protocol": f"{ROUNDS} rounds, the ways taking turns; per round {WARM} warm-up, {ALONE} samples alone (median), then {SAMPLES} back to back with one fetch"}

    # the two ways give the same records
    gt, freq = host_colour(label, BOX, out_hw)
    m.add_seg_label(seg, label, crop=BOX)
    m.add_seg(seg, gt)
    rec, _ = m.fetch()
    lab = m.fetch_labels()
    assert rec[0:1].tobytes() == rec[1:2].tobytes() and tuple(lab[0]["freq"]) == tuple(freq), "the device's ground truth is the host's"
    m.reset()
    m.add_depth_label(d3, depth32)
    m.add_depth(d3, host_depth(depth32, out_hw))
    rec, _ = m.fetch()
    assert rec[0:1].tobytes() == rec[1:2].tobytes(), "the device's depth ground truth is the host's"
    m.reset()

    def host_seg():
        g, _ = host_colour(label, BOX, out_hw)
        m.add_seg(seg, g)

    res = measure({"device": lambda: m.add_seg_label(seg, label, crop=BOX), "host_numpy": host_seg}, m)
    for dtype, v in (("f32", depth32), ("f64", depth64)):
        r = measure({"device": lambda v=v: m.add_depth_label(d3, v), "host_numpy": lambda v=v: m.add_depth(d3, host_depth(v, out_hw))}, m)
        for way in r:
            out[f"depth_{dtype}_{way}_host_to_host_us_rounds"] = r[way]["alone"]
            out[f"depth_{dtype}_{way}_in_stream_us_per_sample_rounds"] = r[way]["stream"]
        out[f"depth_{dtype}_host_to_host_ratio_host_over_device"] = round(float(np.median(r["host_numpy"]["alone"]) / np.median(r["device"]["alone"])), 2)
        out[f"depth_{dtype}_in_stream_ratio_host_over_device"] = round(float(np.median(r["host_numpy"]["stream"]) / np.median(r["device"]["stream"])), 2)
    for way in res:
        out[f"colour_{way}_host_to_host_us_rounds"] = res[way]["alone"]
        out[f"colour_{way}_in_stream_us_per_sample_rounds"] = res[way]["stream"]
    out["colour_host_to_host_ratio_host_over_device"] = round(float(np.median(res["host_numpy"]["alone"]) / np.median(res["device"]["alone"])), 2)
    out["colour_in_stream_ratio_host_over_device"] = round(float(np.median(res["host_numpy"]["stream"]) / np.median(res["device"]["stream"])), 2)

    # what of the device way is the host's copy into the pinned slot: the same bytes through numpy
    t = []
    dst = np.empty_like(label)
    for _ in range(10):
        t0 = time.perf_counter()
        np.copyto(dst, label)
        t.append((time.perf_counter() - t0) * 1e6)
    out["host_copy_of_the_colour_label_us"] = round(float(np.median(t)), 1)

    t0 = time.perf_counter()
    loop_freq = python_loop(label, BOX)
    out["python_pixel_loop_once_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    assert tuple(loop_freq) == tuple(int(f) for f in freq)
    m.close()
    seg.close()
    d3.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
