#!/usr/bin/env python3
"""Developer tool: host-to-host time of the AutoSpeed detector's device stages (vp_detect_preprocess: letterbox of a 1920x1080 BGR frame to
640x640 planes; vp_detect_postprocess: decode + per-class NMS of a [4 + classes][8400] tensor), p50 over 200 calls each.

python tools/bench_detect.py
python tools/bench_detect.py --network   the detector NETWORK as an engine of this library (VP_AUTOSPEED) instead: the per-launch table
    (vp_profile_layers), in-graph time per frame, vp_detect_infer host-to-host p50 / p99 over 1000 calls on a 1280 x 720 frame and, in the same run for
    scale, the AutoDrive engine's p50 and the two stages around a host-run network (512 x 1024 letterbox; decode + NMS of the network's own tensor).
python tools/bench_detect.py --python-wrapper   the Python wrapper's twin on a 1280 x 720 frame: infer.AutoSpeedNetworkInfer.inference p50, vp_detect_infer_pil
    and vp_detect_infer host-to-host p50 / p99 on the same handle and frame, the network's in-graph time, and the two letterboxes and decodes alone."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch  # noqa: F401
from autoware_vision_pilot_amd import lib
import _autospeed_cases as cases



def network():
    from autoware_vision_pilot_amd import synthetic, weights as vw

    frame = synthetic.synthetic_frame(720, 1280, 21)
    conf, iou = 0.4, 0.65
    out = {"library": lib.version()}
    for prec in ("fp16x3", "fp16"):
        eng = lib.Engine("autospeed", vw.pack_state_dict(synthetic.make_autospeed_state_dict(5)), precision=prec)
        det = lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
        det.attach(eng)
        for _ in range(30):
            d, n = det.infer(frame, conf, iou, cap=300)
        t = []
        for _ in range(1000):
            t0 = time.perf_counter(); det.infer(frame, conf, iou, cap=300); t.append((time.perf_counter() - t0) * 1e6)
        out[f"{prec}_detect_infer_1280x720_p50_us"] = round(float(np.percentile(t, 50)), 1)
        out[f"{prec}_detect_infer_1280x720_p99_us"] = round(float(np.percentile(t, 99)), 1)
        out[f"{prec}_detections_kept"] = int(n)
        g = []
        for _ in range(200):
            eng.timer_begin(); eng.enqueue(); g.append(eng.timer_end() * 1e3)
        out[f"{prec}_network_in_graph_p50_us"] = round(float(np.percentile(g, 50)), 1)
        ms = eng.profile_layers(20)
        rows = list(zip(eng.layers(), eng.layer_kernels(), ms))
        print(f"# per-launch table, VP_AUTOSPEED {prec} (us, mean of 20 isolated launches)")
        for (name, _, _), tag, v in rows:
            print(f"{name:40s} {tag:44s} {v * 1e3:8.1f}")
        out[f"{prec}_launches"] = len(rows)
        out[f"{prec}_sum_of_launches_us"] = round(float(sum(ms)) * 1e3, 1)
        out[f"{prec}_backbone_launches_us"] = round(float(sum(v for (nm, _, _), v in zip(eng.layers(), ms) if nm.startswith("net."))) * 1e3, 1)
        # the two-call form around a host-run network, same frame and the network's own tensor
        raw = eng.logits().reshape(8, 10752).copy()
        for key, fn in (("letterbox_1280x720_to_512x1024", lambda: det.preprocess(frame)), ("postprocess_own_raw", lambda: det.postprocess(raw, conf, iou))):
            for _ in range(20):
                fn()
            t = []
            for _ in range(200):
                t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e6)
            out[f"{prec}_{key}_p50_us"] = round(float(np.percentile(t, 50)), 1)
        det.close()
        eng.close()
        ad = lib.Engine("autodrive", vw.pack_state_dict(synthetic.make_autodrive_state_dict(0)), precision=prec)
        big = synthetic.synthetic_frame(1080, 1920, 3)
        for _ in range(30):
            ad.infer(big)
        t = []
        for _ in range(300):
            t0 = time.perf_counter(); ad.infer(big); t.append((time.perf_counter() - t0) * 1e6)
        out[f"{prec}_autodrive_infer_1920x1080_p50_us"] = round(float(np.percentile(t, 50)), 1)
        msa = ad.profile_layers(20)
        out[f"{prec}_autodrive_backbone_launches_us"] = round(float(sum(v for (nm, _, _), v in zip(ad.layers(), msa) if nm.startswith("backbone."))) * 1e3, 1)
        ad.close()
    print(json.dumps(out))


def python_wrapper():
    from PIL import Image

    from autoware_vision_pilot_amd import infer, synthetic, weights as vw

    bgr = synthetic.synthetic_frame(720, 1280, 21)
    rgb = np.ascontiguousarray(bgr[:, :, ::-1])
    image = Image.fromarray(rgb)
    out = {"library": lib.version()}

    def p(fn, n, warm=30):
        for _ in range(warm):
            fn()
        t = []
        for _ in range(n):
            t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e6)
        return round(float(np.percentile(t, 50)), 1), round(float(np.percentile(t, 99)), 1)

    for prec in ("fp16x3", "fp16"):
        twin = infer.AutoSpeedNetworkInfer(vw.pack_state_dict(synthetic.make_autospeed_state_dict(5)), precision=prec)
        det, eng = twin._detector, twin.model
        out[f"{prec}_rows_kept"] = len(twin.inference(image))
        out[f"{prec}_inference_1280x720_p50_us"], out[f"{prec}_inference_1280x720_p99_us"] = p(lambda: twin.inference(image), 1000)
        out[f"{prec}_detect_infer_pil_1280x720_p50_us"], out[f"{prec}_detect_infer_pil_1280x720_p99_us"] = p(lambda: det.infer_pil(rgb, 0.6, 0.45, cap=300), 1000)
        out[f"{prec}_detect_infer_1280x720_p50_us"], out[f"{prec}_detect_infer_1280x720_p99_us"] = p(lambda: det.infer(bgr, 0.6, 0.45, cap=300), 1000)
        g = []
        for _ in range(200):
            eng.timer_begin(); eng.enqueue(); g.append(eng.timer_end() * 1e3)
        out[f"{prec}_network_in_graph_p50_us"] = round(float(np.percentile(g, 50)), 1)
        raw = eng.logits().reshape(8, 10752).copy()
        out[f"{prec}_letterbox_pil_p50_us"] = p(lambda: det.preprocess_pil(rgb), 200, 20)[0]
        out[f"{prec}_letterbox_p50_us"] = p(lambda: det.preprocess(bgr), 200, 20)[0]
        out[f"{prec}_postprocess_agnostic_own_raw_p50_us"] = p(lambda: det.postprocess_agnostic(raw, 0.6, 0.45), 200, 20)[0]
        out[f"{prec}_postprocess_own_raw_p50_us"] = p(lambda: det.postprocess(raw, 0.6, 0.45), 200, 20)[0]
        det.close()
        eng.close()
    print(json.dumps(out))


if "--python-wrapper" in sys.argv[1:]:
    python_wrapper()
    sys.exit(0)
if "--network" in sys.argv[1:]:
    network()
    sys.exit(0)

det = lib.Detector(640, 640, 8400, 84)
frame = cases.frame(1080, 1920, 3)
out = {}
for _ in range(20):
    det.preprocess(frame)
t = []
for _ in range(200):
    t0 = time.perf_counter(); det.preprocess(frame); t.append((time.perf_counter() - t0) * 1e6)
out["preprocess_1920x1080_to_640x640_p50_us"] = round(float(np.percentile(t, 50)), 1)
for name, nc, p_obj in (("4_classes_8400_boxes", 4, 0.12), ("80_classes_8400_boxes", 80, 0.12), ("4_classes_dense", 4, 0.6)):
    raw = cases.raw_tensor(8400, nc, 11, p_obj=p_obj)
    for _ in range(20):
        d, n = det.postprocess(raw, 0.25, 0.45)
    t = []
    for _ in range(200):
        t0 = time.perf_counter(); d, n = det.postprocess(raw, 0.25, 0.45); t.append((time.perf_counter() - t0) * 1e6)
    out[f"postprocess_{name}_p50_us"] = round(float(np.percentile(t, 50)), 1)
    out[f"postprocess_{name}_candidates_kept"] = [int((np.nan_to_num(raw[4:]).max(axis=0) > 0.25).sum()), int(n)]
out["library"] = lib.version()
print(json.dumps(out))
