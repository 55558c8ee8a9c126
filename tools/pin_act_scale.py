#!/usr/bin/env python3
"""Pin the VP_ACT_SCALE range case against the reference's OWN AutoDrive nn.Module: (re)generates tests/golden/autodrive_range.npz.

Runs only where the reference checkout exists (VP_REFERENCE, default /root/reference); everything else uses the committed fixture.
Usage:  python tools/pin_act_scale.py [--out PATH]

The weight seed is the one whose all-0 -> all-255 frame pair trips the range guard in tests/test_gpu_parity_sweep_r5.py (seed 25, "RANGE GUARD" rows of
profiles/r0*_parity_sweep.tsv).  Three pairs -- that one and two ordinary synthetic pairs -- go through the reference module in fp32 and in fp64, with the
fp32 weights and with the fp8(e4m3)-dequantised weights; the file holds data only: the three outputs per pair / precision / weight form and the fp64
abs-max of every backbone stage output (to locate a failure).  Printed: |fp32 - fp64| / max(1, |fp64|) per output -- the number that decides which bar
tests/test_gpu_act_scale.py::test_range_case applies."""
import argparse
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("VP_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

WEIGHT_SEED = 25
PAIRS = ("range", "a", "b")          # all-0 -> all-255; synthetic frames 200 -> 201; 203 -> 204 (the sweep's frames)
STAGES = ("p1", "p2", "p3", "p4", "p5")
GOLDEN = os.path.join(ROOT, "tests", "golden", "autodrive_range.npz")


def pair_frames(name):
    from oracle import pre_post

    if name == "range":
        return np.zeros((1080, 1920, 3), dtype=np.uint8), np.full((1080, 1920, 3), 255, dtype=np.uint8)
    i = {"a": 0, "b": 3}[name]
    return tuple(pre_post.synthetic_frame(1080, 1920, 200 + k, smooth=(k % 3 != 2)) for k in (i, i + 1))


def save_npz(path, arrays):
    """np.savez without the wall-clock time stamps of its zip entries: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    sys.path.insert(0, REFERENCE)
    from Models.model_components.autodrive.autodrive_network import AutoDrive
    from oracle import autodrive, pre_post

    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {"weight_seed": np.int64(WEIGHT_SEED)}
    for wtag, quant in (("", False), ("fp8_", True)):
        sd_np = autodrive.make_state_dict(WEIGHT_SEED)
        if quant:
            sd_np = autodrive.quantize_fp8_e4m3(sd_np)
        for name in PAIRS:
            xs = [pre_post.preprocess(f, input_is_bgr=True, planes_rgb=True, out_h=512, out_w=1024, resize="pil_bilinear") for f in pair_frames(name)]
            res = {}
            for dt in (torch.float32, torch.float64):
                m = AutoDrive().eval()
                missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=False)
                assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
                m = m.to(dt)
                amax = {}
                hooks = [getattr(m.backbone, s).register_forward_hook(lambda mod, i, o, s=s: amax.__setitem__(s, max(amax.get(s, 0.0), float(o.abs().max()))))
                         for s in STAGES]
                with torch.no_grad():
                    y = m(torch.from_numpy(xs[0]).to(dt), torch.from_numpy(xs[1]).to(dt))
                for h in hooks:
                    h.remove()
                res[dt] = np.array([float(v) for v in y], dtype=np.float64)
                if dt == torch.float64 and not quant:
                    out[f"{name}_stage_absmax_fp64"] = np.array([amax[s] for s in STAGES], dtype=np.float64)
            out[f"{wtag}{name}_fp32"] = res[torch.float32].astype(np.float32)
            out[f"{wtag}{name}_fp64"] = res[torch.float64]
            rel = np.abs(res[torch.float32] - res[torch.float64]) / np.maximum(1.0, np.abs(res[torch.float64]))
            print(f"{wtag or 'fp32_weights_'}{name}: fp64 {res[torch.float64].tolist()}  |fp32 - fp64| / max(1, |fp64|) = {rel.tolist()}")
    save_npz(args.out, out)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
