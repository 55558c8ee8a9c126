#!/usr/bin/env python3
"""Pin the label cases: (re)generates tests/golden/label_cases.npz from the reference's OWN loaders, on the CPU.

Usage:  python tools/pin_label.py [--out PATH]

Runs only where the reference checkout is present (VP_REFERENCE, default /root/reference).
  Colour labels: LoadDataSceneSeg.extractROI and createGroundTruth (Models/data_utils/load_data_scene_seg.py) on tiny synthetic RGB labels.  The class is
    created without its constructor (which lists a dataset directory); the two methods read `dataset` only.  Stored per case: the label, the dataset
    name, the three full-resolution planes (background, foreground, road; 0 / 255), the frequencies the class weights were made from and the weights.
  Boxes: extractROI's crop size for every dataset name on one image size.
  Depth labels: LoadDataScene3D.getItemVal (load_data_scene_3d.py) on .npy files written to a temporary directory, float32 and float64; stored: the
    plane and what getItemVal returned.
The nearest resize behind the loaders (albumentations / cv2) is absent from this environment and stays unpinned."""
import argparse
import os
import sys
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("VP_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import label_cases as lc  # noqa: E402

# name -> (dataset, h, w, seed): COMMA10K drops a column and keeps 70 % of the rows, BDD100K's and IDDAW's boxes exceed a small image (PIL pads),
# MAPILLARY has no crop
SEG_PINS = {"comma": ("COMMA10K", 30, 41, 11), "bdd": ("BDD100K", 24, 36, 12), "iddaw": ("IDDAW", 500, 30, 13), "mapillary": ("MAPILLARY", 19, 23, 14)}
DEPTH_PINS = ("random", "negative_and_zero", "constant", "one_nan", "one_inf")
ROI_HW = (40, 50)


def load_reference():
    path = os.path.join(REFERENCE, "Models")
    if not os.path.exists(os.path.join(path, "data_utils", "load_data_scene_seg.py")):
        raise SystemExit("the reference checkout is not present at %s (VP_REFERENCE)" % REFERENCE)
    sys.path.insert(0, path)
    from data_utils.load_data_scene_3d import LoadDataScene3D
    from data_utils.load_data_scene_seg import LoadDataSceneSeg

    return LoadDataSceneSeg, LoadDataScene3D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=lc.GOLDEN)
    args = ap.parse_args()
    Seg, Depth = load_reference()
    data = {}
    for name, (dataset, h, w, seed) in SEG_PINS.items():
        label = lc.palette_image(h, w, seed, stray=0.1)
        loader = object.__new__(Seg)
        loader.dataset = dataset
        _, roi = loader.extractROI(Image.fromarray(label, "RGB"), Image.fromarray(label, "RGB"))
        truth, weights = loader.createGroundTruth(roi)
        planes = np.stack(truth[1:4])
        freq = np.array([int((p == 255).sum()) for p in planes], np.int64)
        n = roi.size[0] * roi.size[1]
        assert [n / (f + 5120) for f in freq] == list(weights), "the planes hold the frequencies the weights were made from"
        k = "seg_" + name
        data[k + "_label"], data[k + "_dataset"], data[k + "_planes"], data[k + "_freq"], data[k + "_weights"] = label, np.array(dataset), planes, freq, np.array(weights, np.float64)
        print("%-10s %-9s crop %4d x %4d freq %s" % (name, dataset, planes.shape[1], planes.shape[2], freq.tolist()))
    for dataset in lc.ROI_DATASETS:
        loader = object.__new__(Seg)
        loader.dataset = dataset
        blank = Image.new("RGB", (ROI_HW[1], ROI_HW[0]))
        _, roi = loader.extractROI(blank, blank)
        data["roi_" + dataset] = np.array(roi.size, np.int64)   # (width, height)
    with tempfile.TemporaryDirectory() as tmp:
        Image.new("RGB", (4, 4)).save(os.path.join(tmp, "image.png"))
        for name in DEPTH_PINS:
            for tag, dtype in (("f32", np.float32), ("f64", np.float64)):
                v = lc.depth_case(name, dtype)
                np.save(os.path.join(tmp, "label.npy"), v)
                loader = object.__new__(Depth)
                loader.val_images, loader.val_labels = [os.path.join(tmp, "image.png")], [os.path.join(tmp, "label.npy")]
                with np.errstate(all="ignore"):
                    _, truth = loader.getItemVal(0)
                assert truth.dtype == dtype and truth.shape == v.shape + (1,)
                k = "depth_%s_%s" % (name, tag)
                data[k + "_label"], data[k + "_truth"] = v, truth[..., 0]
                print("%-24s %s finite %d of %d" % (name, tag, int(np.isfinite(truth).sum()), truth.size))
    np.savez_compressed(args.out, **data)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
