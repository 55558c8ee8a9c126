#!/usr/bin/env python3
"""Pin the class-agnostic decode + NMS (vp_detect_postprocess_agnostic) to the library as it is built now: writes the rows and the two counts of
tests/autospeed_py_cases.pin_cases() -- the hand-built cases, the fixture columns, the case of more than 1024 candidates in full and cut to 1100 boxes.

  python tools/pin_detect_agnostic.py                    the CPU emulation (tests/emul) -> tests/golden/detect_agnostic_parent.npz
  python tools/pin_detect_agnostic.py --device --out F   the device library -> F (to compare two builds on one GPU, score column included)
  python tools/pin_detect_agnostic.py --compare A B      every array of two such files, bit for bit

tests/golden/detect_agnostic_parent.npz was written with the two-kernel library that preceded the one-kernel form (detect_nms_kernel) and is what
tests/test_autospeed_py_emulated.py and tests/test_gpu_autospeed_py.py hold that kernel to: do not regenerate it from a later build."""
import argparse
import ctypes as ct
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emul"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def compare(a, b):
    fa, fb = np.load(a), np.load(b)
    bad = sorted(set(fa.files) ^ set(fb.files))
    for k in sorted(set(fa.files) & set(fb.files)):
        same = fa[k].shape == fb[k].shape and np.array_equal(fa[k].view(np.uint32), fb[k].view(np.uint32))
        if not same and k.endswith("_rows") and fa[k].shape == fb[k].shape:
            cols = sorted(set(np.nonzero(fa[k].view(np.uint32) != fb[k].view(np.uint32))[1].tolist()))
            print(f"{k}: DIFFERENT in columns {cols}")
        elif not same:
            print(f"{k}: DIFFERENT")
        bad += [] if same else [k]
    print(f"{len(fa.files)} arrays, {len(bad)} different" + ("" if bad else ": bit-identical, score column included"))
    return 1 if bad else 0


def main():
    import autospeed_py_cases as cases
    from pin_autospeed_py import save_npz

    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--out", default=cases.PIN)
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    if args.device:
        import torch  # noqa: F401  (first: one shared HIP runtime)
    from autoware_vision_pilot_amd import lib

    if not args.device:
        import build as emul_build

        so = ct.CDLL(emul_build.build(), mode=os.RTLD_LOCAL | os.RTLD_NOW)
        for name, (res, argtypes) in lib._SIGS.items():
            fn = getattr(so, name)
            fn.restype, fn.argtypes = res, argtypes
        lib._lib = so
    det = lib.Detector(cases.NET_H, cases.NET_W, max_boxes=cases.LARGE_BOXES, max_attrs=8)
    out = {}
    for key, case in cases.pin_cases().items():
        rows, counts = cases.pin_record(det, *case)
        out[key + "_rows"], out[key + "_counts"] = rows, counts
        print(f"{key}: {case[0].shape[1]} boxes, counts {counts.tolist()}")
    det.close()
    save_npz(args.out, out)
    print(args.out, os.path.getsize(args.out), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
