"""Pin tests/autospeed_py_ref.py against the reference's OWN Python wrapper and write tests/golden/autospeed_py.npz.

Runs only where the reference tree is readable:  python tools/pin_autospeed_py.py /path/to/reference
  1. Models/inference/auto_speed_infer.py is read into memory and executed as a module (importlib, nothing of it is written anywhere) with a stub
     `torchvision` in sys.modules: ops.nms is the restatement's nms (torchvision is not installed: torchvision.ops.nms stays PARITY UNPINNED),
     transforms.ToTensor is uint8 -> float32 / 255 and hands back a tensor whose .half() / .to() are identities -- the reference casts to fp16 only
     because it runs a half model on CUDA; the module here, like the engine, takes the fp32 tensor;
  2. an AutoSpeedNetworkInfer object gets the reference's own detector module on the synthetic checkpoint of tools/pin_autospeed_net.py as its model;
     its resize_letterbox, post_process_predictions and inference (the back-mapping) run on the frames below;
  3. every result must equal the restatement's at distance 0.0;
  4. the fixture conditions are asserted on the reference's results alone (see check_conditions); the thresholds are the reference's defaults when
     those meet them, else the first pair of a small grid that does -- recorded in the file;
  5. the vectors are written: frames (h, w, seed), geometry, a sparse sample of the letterboxed tensor, the module's raw at every 11th box and at
     every box near or above the threshold, kept rows.
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FRAMES = ((1080, 1920, 25), (500, 1400, 2))   # (h, w, seed) of synthetic.synthetic_frame, chosen so that the conditions hold: taller than 2:1 (pads left / right), wider (pads top / bottom)
BOX_STEP, TENSOR_STEP = 11, 197
MARGIN = 2e-3
CAND_BAND = 0.03
GRID = sorted(((round(0.53 + 0.005 * a, 3), round(0.30 + 0.01 * b, 2)) for a in range(35) for b in range(41)), key=lambda t: (abs(t[0] - 0.6) + abs(t[1] - 0.45), t))


def load_reference_wrapper(reference_root, ref):
    """the reference's auto_speed_infer module, executed from a source copy in memory under a stub torchvision"""
    import torch

    class _KeepsFp32(torch.Tensor):
        def half(self):
            return self

        def to(self, *a, **k):
            return self

    class ToTensor:
        def __call__(self, img):
            t = torch.from_numpy(np.asarray(img).astype(np.float32).transpose(2, 0, 1).copy()).div(255)
            return t.as_subclass(_KeepsFp32)

    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.ToTensor = ToTensor
    tv.ops = types.ModuleType("torchvision.ops")
    tv.ops.nms = lambda boxes, scores, iou: torch.from_numpy(ref.nms(boxes.numpy(), scores.numpy(), iou))
    saved = {k: sys.modules.get(k) for k in ("torchvision", "torchvision.transforms", "torchvision.ops")}
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tv.transforms, "torchvision.ops": tv.ops})
    try:
        path = os.path.join(reference_root, "Models", "inference", "auto_speed_infer.py")
        with open(path) as f:
            source = f.read()
        spec = importlib.util.spec_from_loader("reference_auto_speed_infer", loader=None, origin=path)
        mod = importlib.util.module_from_spec(spec)
        exec(compile(source, path, "exec"), mod.__dict__)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def check_conditions(ref, raw, rows, lb_rows, conf, iou, orig_w, orig_h):
    """On the reference's results: no sigmoid(score) within MARGIN of conf, no candidate pair's IoU within MARGIN of iou, 20 .. 2000 candidates;
    returns (a suppression happened between boxes of different classes, a kept box is clamped)."""
    score_gap, iou_gap, n = ref.candidate_iou_gap(raw, conf, iou)
    if not (score_gap > MARGIN and iou_gap > MARGIN and 20 <= n <= 2000 and len(rows) >= 3):
        return None
    every = ref.post_process(raw, conf, 2.0).numpy()          # all candidates, sorted: which of them did a kept box of ANOTHER class remove?
    kept = {tuple(r[:5]) for r in lb_rows}
    cross = False
    for j, r in enumerate(every):
        if tuple(r[:5]) in kept:
            continue
        for k in every[:j]:
            if tuple(k[:5]) in kept:
                iw = max(0.0, min(k[2], r[2]) - max(k[0], r[0]))
                ih = max(0.0, min(k[3], r[3]) - max(k[1], r[1]))
                ovr = iw * ih / ((k[2] - k[0]) * (k[3] - k[1]) + (r[2] - r[0]) * (r[3] - r[1]) - iw * ih)
                if ovr > iou:
                    cross |= k[5] != r[5]
                    break
    rows = np.asarray(rows, np.float32)
    clamped = bool(((rows[:, [0, 1]] == 0).any() or (rows[:, 2] == orig_w).any() or (rows[:, 3] == orig_h).any()))
    return cross, clamped, score_gap, iou_gap, n


def save_npz(path, arrays):
    """np.savez_compressed with a fixed entry date: the file regenerates byte for byte"""
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def main(reference_root):
    import torch
    from PIL import Image

    import autospeed_py_ref as ref
    import pin_autospeed_net as net_pin
    from autoware_vision_pilot_amd import synthetic

    mod = load_reference_wrapper(reference_root, ref)
    sd = synthetic.make_autospeed_state_dict(net_pin.WEIGHT_SEED)
    wrapper = object.__new__(mod.AutoSpeedNetworkInfer)       # __init__ only loads a checkpoint file (:6-13)
    wrapper.train_size = ref.TRAIN_SIZE
    wrapper.device = torch.device("cpu")
    wrapper.model = net_pin.reference_module(reference_root, sd)
    assert mod.AutoSpeedNetworkInfer.post_process_predictions.__defaults__ == (ref.CONF, ref.IOU)

    images, raws, tensors, geoms = [], [], [], []
    for h, w, seed in FRAMES:
        image = Image.fromarray(np.ascontiguousarray(synthetic.synthetic_frame(h, w, seed)[:, :, ::-1]))   # the synthetic frames are BGR
        padded, scale, pad_x, pad_y = wrapper.resize_letterbox(image)
        x, geom = ref.letterbox_pil(image)
        assert (scale, pad_x, pad_y) == geom and ref.letterbox_geometry(w, h)[0] == scale
        tensor, *_ = wrapper.image_to_tensor(image)
        assert tensor.dtype == torch.float32 and float((tensor[0] - torch.from_numpy(x)).abs().max()) == 0.0
        with torch.no_grad():
            raw = wrapper.model(tensor)[0].numpy()
        images.append(image), raws.append(raw), tensors.append(x), geoms.append(geom)

    # the thresholds: the grid pair nearest the reference's defaults that meets the conditions on the restatement's decode of the reference module's
    # raw (cheap); the reference's own bodies then run at that pair and the conditions are asserted on what THEY return
    pair = None
    for conf, iou in GRID:
        cs = []
        for (h, w, _), raw, geom in zip(FRAMES, raws, geoms):
            lb = ref.post_process(raw, conf, iou)
            rows = ref.back_map(lb, geom[0], geom[1], geom[2], w, h)
            cs.append(check_conditions(ref, raw, rows, lb.numpy(), conf, iou, w, h) if rows else None)
            if cs[-1] is None:
                break
        if cs[-1] is not None and any(c[0] for c in cs) and any(c[1] for c in cs):
            pair = (conf, iou)
            break
    assert pair is not None, "no threshold pair of the grid meets the conditions"
    conf, iou = pair
    wrapper.post_process_predictions = lambda t: mod.AutoSpeedNetworkInfer.post_process_predictions(wrapper, t, conf, iou)
    results, cross_any, clamp_any = [], False, False
    for (h, w, _), image, raw, geom in zip(FRAMES, images, raws, geoms):
        lb = mod.AutoSpeedNetworkInfer.post_process_predictions(wrapper, torch.from_numpy(raw)[None], conf, iou)
        want_lb = ref.post_process(raw, conf, iou)
        assert lb.shape == want_lb.shape and lb.numel() > 0 and float((lb - want_lb).abs().max()) == 0.0, "post_process differs from the reference's"
        rows = wrapper.inference(image)                      # letterbox, the module, post-process, the back-mapping: the reference's own bodies
        assert rows == ref.back_map(want_lb, geom[0], geom[1], geom[2], w, h), "the back-mapping differs from the reference's"
        c = check_conditions(ref, raw, rows, lb.numpy(), conf, iou, w, h)
        assert c is not None, "the reference's own results miss the margins"
        cross_any |= c[0]
        clamp_any |= c[1]
        results.append((np.array(rows, np.float32).reshape(-1, 6), c))
    assert cross_any, "no suppression between boxes of different classes"
    assert clamp_any, "no kept box is clamped"
    out = {"weight_seed": net_pin.WEIGHT_SEED, "frames": np.array(FRAMES), "conf": np.float64(conf), "iou": np.float64(iou), "box_step": BOX_STEP,
           "tensor_step": TENSOR_STEP}
    for fi, ((h, w, seed), raw, x, geom, (rows, c)) in enumerate(zip(FRAMES, raws, tensors, geoms, results)):
        print(f"frame {fi} ({h}x{w}, seed {seed}): distance 0.0; geometry {geom}; {c[4]} candidates, {len(rows)} kept; score gap {c[2]:.4f}, IoU gap {c[3]:.4f}; "
              f"cross-class suppression {c[0]}, clamped {c[1]}")
        out[f"geom_{fi}"] = np.array([geom[0], geom[1], geom[2]], np.float64)
        out[f"tensor_{fi}"] = x.ravel()[::TENSOR_STEP].copy()
        out[f"raw_{fi}"] = raw[:, ::BOX_STEP].copy()
        out[f"rows_{fi}"] = rows
        # every column whose best sigmoid score comes within CAND_BAND of the threshold or above it, in box order: the kept rows follow from these alone
        near = np.flatnonzero(torch.from_numpy(raw[4:]).sigmoid().numpy().max(axis=0) > conf - CAND_BAND)
        out[f"cand_idx_{fi}"] = near.astype(np.int32)
        out[f"cand_raw_{fi}"] = raw[:, near].copy()
    print(f"thresholds: conf {conf}, iou {iou}" + ("" if (conf, iou) == (ref.CONF, ref.IOU) else "  (the defaults 0.6 / 0.45 do not meet the conditions)"))
    path = os.path.join(ROOT, "tests", "golden", "autospeed_py.npz")
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
