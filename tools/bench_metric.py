#!/usr/bin/env python3
"""What vp_metric costs on one MI355X, against the same scores computed on the host.  THE WEIGHTS ARE SYNTHETIC (the seeded state-dicts of BASELINE /
tests/conftest.py): the agreement figures say how far the reduced-precision engines move the task scores on such weights, not on a trained checkpoint.
Nothing is fixed in advance: the file records what was measured.

  (a) device time per record: FRAMES add calls on an engine's resident logits (ground truth resident too) between two events on the ENGINE's stream --
      every add makes that stream wait for the metric's read, so the second event lies behind the last record; after WARM calls.  Segmentation (SceneSeg,
      3 x 320 x 640) and depth (Scene3D, 320 x 640).
  (b) the same scores on the host: vp_fetch_outputs (the D2H of the logits) + the restatement in torch on 16 threads (argmax cascade and counts;
      normalisation, torch.quantile, the four edge scales), per frame, wall clock.
  (c) SceneSeg fp16 frames/s, enqueue only, with and without an add_seg_pair per frame (the pair's reference is a second fp16 engine that ran once).
  (d) --agreement: fp16 against fp16x3, and fp8 weight storage where the kind has it, over 32 synthetic frames: per-class IoU, flipped pixels, mAE, mEL.
  (e) the depth chain's distance from the fp64 restatement on the general cases of tests/metric_cases.py, beside torch fp32's own distance and the bar.

  --lanes: the same four measurements for the lane part (EgoLanes and AutoSteer records): see lanes().

python tools/bench_metric.py > profiles/metric.txt;  python tools/bench_metric.py --agreement >> profiles/metric.txt
python tools/bench_metric.py --lanes > profiles/metric_lanes.txt"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.nn.functional as F

from autoware_vision_pilot_amd import lib, synthetic, weights as vw
from oracle import weights

SEEDS = {"sceneseg": 0, "scene3d": 1, "domainseg": 3}
WARM, FRAMES = 50, 400
H, W = 720, 1280


def engine(kind, precision, **kw):
    return lib.Engine(kind, vw.pack_state_dict(weights.make_state_dict(kind, SEEDS[kind])), precision=precision, **kw)


def host_seg(lg, gt):
    a, b, c = lg[0], lg[1], lg[2]
    first = (a >= b) & (a >= c)
    second = ~first & (b >= a) & (b >= c)
    third = ~first & ~second & (c >= a) & (c >= b)
    out = []
    for k, pred in enumerate((first, second, third)):
        t = gt == k
        i = int((pred & t).sum())
        out.append((i + 1) / (int(pred.sum()) + int(t.sum()) - i + 1))
    return out


GX = torch.tensor(((0.125, 0.0, -0.125), (0.25, 0.0, -0.25), (0.125, 0.0, -0.125))).view(1, 1, 3, 3)
GY = torch.tensor(((0.125, 0.25, 0.125), (0.0, 0.0, 0.0), (-0.125, -0.25, -0.125))).view(1, 1, 3, 3)


def host_depth(p, g):
    def ssi(t):
        return (t - t.min()) / (t.max() - t.mean())

    a, b = ssi(p)[None, None], ssi(g)[None, None]
    A = (a - b).abs()
    mae = A[A < torch.quantile(A, 0.9, interpolation="linear")].mean()
    mel = 0.0
    for s in range(4):
        d = a - b
        mel = mel + (F.conv2d(d, GX, padding=1).abs() + F.conv2d(d, GY, padding=1).abs()).mean()
        if s < 3:
            a, b = F.avg_pool2d(a, 2, stride=2), F.avg_pool2d(b, 2, stride=2)
    return float(mae), float(mel) / 4


def timed_adds(eng, add):
    for _ in range(WARM):
        add()
    eng.sync()
    eng.timer_begin()
    for _ in range(FRAMES):
        add()
    return eng.timer_end() * 1e3 / FRAMES


def costs():
    torch.set_num_threads(16)
    frame = synthetic.synthetic_frame(H, W, 21)
    seg, seg_ref, s3d = engine("sceneseg", "fp16"), engine("sceneseg", "fp16"), engine("scene3d", "fp16")
    for e in (seg, seg_ref, s3d):
        e.infer(frame)
    oh, ow = seg.output_dims()[-2:]
    rng = np.random.default_rng(0)
    gt = rng.integers(0, 3, (oh, ow)).astype(np.uint8)
    gd = (rng.random((oh, ow)) * 30 + 1).astype(np.float32)
    d_gt, d_gd = torch.from_numpy(gt).cuda(), torch.from_numpy(gd).cuda()
    torch.cuda.synchronize()
    m = lib.Metric(max_frames=WARM + FRAMES)
    out = {"library": lib.version(), "weights": "SYNTHETIC (seeded state-dicts); frame: synthetic 1280 x 720", "frames_per_measurement": FRAMES, "warm_up": WARM}
    # (a)
    a = {}
    for name, eng, add in (("seg_record_us", seg, lambda: m.add_seg(seg, d_gt.data_ptr(), "label", gt_device=True)),
                           ("seg_pair_record_us", seg, lambda: m.add_seg_pair(seg, seg_ref)),
                           ("depth_record_us", s3d, lambda: m.add_depth(s3d, d_gd.data_ptr(), gt_device=True))):
        rounds = []
        for _ in range(3):
            m.reset()
            rounds.append(round(timed_adds(eng, add), 2))
            m.fetch()
        a[name + "_rounds"] = rounds
    out["a_device_time_per_record"] = a
    # (b)
    b = {}
    tg, tgd = torch.from_numpy(gt), torch.from_numpy(gd)
    for name, eng, fn in (("seg_host_us", seg, lambda lg: host_seg(torch.from_numpy(lg), tg)), ("depth_host_us", s3d, lambda lg: host_depth(torch.from_numpy(lg[0]), tgd))):
        d2h, total = [], []
        for i in range(20 + 200):
            eng.enqueue()
            eng.sync()
            t0 = time.perf_counter()
            eng.fetch_outputs()
            lg = eng.logits()
            t1 = time.perf_counter()
            fn(lg)
            t2 = time.perf_counter()
            if i >= 20:
                d2h.append((t1 - t0) * 1e6)
                total.append((t2 - t0) * 1e6)
        b[name] = {"p50": round(float(np.percentile(total, 50)), 1), "p99": round(float(np.percentile(total, 99)), 1), "of_which_fetch_p50": round(float(np.percentile(d2h, 50)), 1)}
    out["b_host_time_per_frame_200_frames_16_threads"] = b
    # (c)
    c = {"without": [], "with_add_seg_pair": []}
    for _ in range(3):
        for key in ("without", "with_add_seg_pair"):
            m.reset()
            for _ in range(WARM):
                seg.enqueue()
            seg.sync()
            t0 = time.perf_counter()
            for _ in range(FRAMES):
                seg.enqueue()
                if key != "without":
                    m.add_seg_pair(seg, seg_ref)
            seg.sync()
            m.fetch()
            c[key].append(round(FRAMES / (time.perf_counter() - t0), 1))
    out["c_sceneseg_fp16_frames_per_s_rounds"] = c
    # (e)
    import metric_cases as mc

    lines = []
    for shape in mc.GENERAL_SHAPES:
        mc.check_depth_general(lib, shape, report=lines)
    out["e_depth_distance_from_fp64"] = lines
    print(json.dumps(out, indent=1))
    m.close()
    for e in (seg, seg_ref, s3d):
        e.close()


def agreement():
    n_frames = 32
    frames = [synthetic.synthetic_frame(H, W, 100 + i) for i in range(n_frames)]
    out = {"weights": "SYNTHETIC (seeded state-dicts, BASELINE's seeds %s); %d synthetic 1280 x 720 frames; the reference of every row is the fp16x3 engine's own prediction" % (SEEDS, n_frames)}
    for kind in ("sceneseg", "domainseg", "scene3d"):
        ref = engine(kind, "fp16x3")
        for name, kw in (("fp16", {}), ("fp16+fp8_weights", {"weights_fp8": True}), ("fp16x3+fp8_weights", {"weights_fp8": True})):
            try:
                eng = engine(kind, name.split("+")[0], **kw)
            except (lib.VpError, ValueError) as ex:
                out[f"{kind}_{name}"] = "not available: " + str(ex)[:120]
                continue
            m = lib.Metric(max_frames=n_frames)
            for f in frames:
                ref.infer(f)
                eng.infer(f)
                (m.add_depth_pair if kind == "scene3d" else m.add_seg_pair)(eng, ref)
            rec, s = m.fetch()
            if kind == "scene3d":
                out[f"{kind}_{name}"] = {"mae": s["mae"], "mel": s["mel"], "nan_frames": s["nan_frames"], "mae_max": float(np.nanmax(rec["mae"])), "mel_max": float(np.nanmax(rec["mel"]))}
            else:
                c = 3 if kind == "sceneseg" else 1
                flipped = (rec["P"][:, :c].sum(1) + rec["G"][:, :c].sum(1) - 2 * rec["I"][:, :c].sum(1)) / 2 if c == 3 else rec["P"][:, 0] + rec["G"][:, 0] - 2 * rec["I"][:, 0]
                out[f"{kind}_{name}"] = {"iou": list(s["sceneseg_iou"]) if c == 3 else [s["domainseg_iou"]], "iou_full": s["sceneseg_iou_full"] if c == 3 else s["domainseg_iou"],
                                         "flipped_pixels_mean": float(flipped.mean()), "flipped_pixels_max": float(flipped.max()), "pixels": int(rec["n"][0]),
                                         "nonfinite": int(rec["nonfinite"].sum())}
            m.close()
            eng.close()
        ref.close()
    print(json.dumps({"d_agreement": out}, indent=1))


def lanes():
    """--lanes: the lane part.  (a) device time per EgoLanes record (add_lanes on the resident logits with the ground truth resident, in each form, and the
    pair form) and per AutoSteer record (add_rows_pair: nothing comes from the host), as in costs() (a); (b) the same scores on the host: vp_fetch_outputs +
    the torch / numpy restatement of tests/metric_lanes_cases.py, per frame, wall clock, 16 threads; (c) EgoLanes fp16 frames/s, enqueue only, with and
    without an add_lanes_pair behind every pass; (d) the general cases' distance from the reference's fp64 run."""
    import metric_lanes_cases as lc

    torch.set_num_threads(16)
    ego, ego_ref = (lib.Engine("egolanes", vw.pack_state_dict(weights.make_state_dict("egolanes", 2)), precision="fp16") for _ in range(2))
    blob = vw.pack_state_dict(synthetic.make_autosteer_state_dict(0))
    st, st_ref = lib.Engine("autosteer", blob, precision="fp16"), lib.Engine("autosteer", blob, precision="fp16x3")
    frame, sframe = synthetic.synthetic_frame(H, W, 21), synthetic.synthetic_frame(512, 1024, 22)
    for e in (ego, ego_ref):
        e.infer(frame)
    for e in (st, st_ref):
        e.infer(sframe)
    oh, ow = ego.output_dims()[-2:]
    bits = lc.general_inputs((oh, ow), seed=3)[1]
    big, planes = lc.bits_4x(bits, 4), lc.planes_of_bits(bits)
    d_bits, d_big, d_planes = (torch.from_numpy(v).cuda() for v in (bits, big, planes))
    torch.cuda.synchronize()
    m = lib.Metric(max_frames=WARM + FRAMES)
    out = {"library": lib.version(), "weights": "SYNTHETIC (seeded state-dicts); frames: synthetic 1280 x 720 (EgoLanes, output %d x %d) and 1024 x 512 (AutoSteer)" % (oh, ow),
           "frames_per_measurement": FRAMES, "warm_up": WARM}
    a = {}
    for name, eng, add in (("lanes_record_bits_us", ego, lambda: m.add_lanes(ego, d_bits.data_ptr(), "bits", gt_device=True)),
                           ("lanes_record_bits4x_us", ego, lambda: m.add_lanes(ego, d_big.data_ptr(), "bits4x", gt_device=True)),
                           ("lanes_record_planes_us", ego, lambda: m.add_lanes(ego, d_planes.data_ptr(), "planes", gt_device=True)),
                           ("lanes_pair_record_us", ego, lambda: m.add_lanes_pair(ego, ego_ref)),
                           ("rows_pair_record_us", st, lambda: m.add_rows_pair(st, st_ref))):
        rounds = []
        for _ in range(3):
            m.reset()
            rounds.append(round(timed_adds(eng, add), 2))
            m.fetch_lanes()
            m.fetch_rows()
        a[name + "_rounds"] = rounds
    out["a_device_time_per_record"] = a
    b = {}
    txp, th = np.random.default_rng(1).random(64).astype(np.float32), np.ones(64, np.float32)
    for name, eng, fn in (("lanes_host_us", ego, lambda lg: lc.lanes_ref(lg, planes)), ("rows_host_us", st, lambda lg: lc.rows_ref(lg[0].reshape(-1), lg[1].reshape(-1), txp, th))):
        d2h, total = [], []
        for i in range(20 + 200):
            eng.enqueue()
            eng.sync()
            t0 = time.perf_counter()
            eng.fetch_outputs()
            lg = eng.logits()
            t1 = time.perf_counter()
            fn(lg)
            t2 = time.perf_counter()
            if i >= 20:
                d2h.append((t1 - t0) * 1e6)
                total.append((t2 - t0) * 1e6)
        b[name] = {"p50": round(float(np.percentile(total, 50)), 1), "p99": round(float(np.percentile(total, 99)), 1), "of_which_fetch_p50": round(float(np.percentile(d2h, 50)), 1)}
    out["b_host_time_per_frame_200_frames_16_threads"] = b
    c = {"without": [], "with_add_lanes_pair": []}
    for _ in range(3):
        for key in ("without", "with_add_lanes_pair"):
            m.reset()
            for _ in range(WARM):
                ego.enqueue()
            ego.sync()
            t0 = time.perf_counter()
            for _ in range(FRAMES):
                ego.enqueue()
                if key != "without":
                    m.add_lanes_pair(ego, ego_ref)
            ego.sync()
            m.fetch_lanes()
            c[key].append(round(FRAMES / (time.perf_counter() - t0), 1))
    out["c_egolanes_fp16_frames_per_s_rounds"] = c
    lines = []
    for shape in lc.GENERAL_SHAPES:
        lc.check_lanes_general(lib, shape, report=lines)
    out["d_lanes_distance_from_fp64"] = lines
    print(json.dumps(out, indent=1))
    m.close()
    for e in (ego, ego_ref, st, st_ref):
        e.close()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("bench_metric.py needs a GPU")
    if "--lanes" in sys.argv[1:]:
        lanes()
    else:
        agreement() if "--agreement" in sys.argv[1:] else costs()
