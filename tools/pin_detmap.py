#!/usr/bin/env python3
"""Pin the detector-validation cases: (re)generates tests/golden/detmap.npz from the reference's OWN code.

Usage:  python tools/pin_detmap.py [--out PATH]

Runs only where the reference checkout is present (VP_REFERENCE, default /root/reference).  It imports the reference's
Models/training/auto_speed_util.py and runs its non_max_suppression, compute_metric and compute_ap on the float32 inputs of tests/detmap_cases.py
(generated, never stored: the file keeps a hash of each).  The one thing restated is torchvision.ops.nms, which the module imports and this
environment does not pin: a stand-in module provides it as a stable descending sort and the greedy rule of include/vp_hip.h (iw = fmax(0, fmin - fmax),
inter / (area_i + area_j - inter) > iou) -- this project's own restatement, the caveat tests/autospeed_py_ref.py already states.

Written per frame: the kept rows, the tp words (bit t = compute_metric's column t), {candidates, ranked, kept}; for the dataset (every frame, under the
trainer's bookkeeping of auto_speed_trainer.py:208-219) compute_ap's six results and the grid index its smooth(...).argmax() chose.

Asserted for every case, by the reference's results alone: no two candidates of a frame have equal scores; no two eligible pairs of a frame have equal
IoU; no two kept rows of the dataset have equal conf; the two largest values of the smoothed F1 curve differ by more than 1e-9."""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("VP_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import detmap_cases as dc  # noqa: E402
import detmap_ref as dr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "detmap.npz")


def nms_stand_in(boxes, scores, thr):
    """torchvision.ops.nms restated: indices of the kept boxes in descending score order"""
    order = torch.argsort(scores, descending=True, stable=True)
    b = boxes[order]
    n = b.shape[0]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = torch.zeros(n, dtype=torch.bool)
    keep = []
    zero = torch.zeros((), dtype=b.dtype)
    for k in range(n):
        if dead[k]:
            continue
        keep.append(k)
        r = b[k + 1:]
        iw = torch.fmax(zero, torch.fmin(b[k, 2], r[:, 2]) - torch.fmax(b[k, 0], r[:, 0]))
        ih = torch.fmax(zero, torch.fmin(b[k, 3], r[:, 3]) - torch.fmax(b[k, 1], r[:, 1]))
        inter = iw * ih
        dead[k + 1:] |= inter / ((area[k] + area[k + 1:]) - inter) > thr
    return order[torch.tensor(keep, dtype=torch.long)]


def load_reference():
    path = os.path.join(REFERENCE, "Models", "training")
    if not os.path.exists(os.path.join(path, "auto_speed_util.py")):
        raise SystemExit("the reference checkout is not present at %s (VP_REFERENCE)" % REFERENCE)
    tv = types.ModuleType("torchvision")
    tv.ops = types.ModuleType("torchvision.ops")
    tv.ops.nms = nms_stand_in
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.ops"] = tv.ops
    sys.path.insert(0, path)
    import auto_speed_util as util

    return util


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    util = load_reference()
    chosen = []
    smooth = util.smooth

    def spy(y, f=0.05):                                   # compute_ap does not return the index it chose
        out = smooth(y, f)
        chosen.append(np.array(out))
        return out

    util.smooth = spy
    iou_v = torch.from_numpy(dc.IOU_V.copy())
    assert torch.equal(iou_v, torch.linspace(0.5, 0.95, 10)), "the table's bits are torch.linspace(0.5, 0.95, 10)"
    scale = torch.tensor((dc.NET_W, dc.NET_H, dc.NET_W, dc.NET_H))
    data = {"frames": np.array(dc.FRAMES), "iou_v_bits": dc.bits(dc.IOU_V)}
    metrics = []
    for name in dc.FRAMES:
        raw, labels = dc.frame(name)
        x = torch.from_numpy(raw)[None]
        sc = raw[4:]
        with np.errstate(invalid="ignore"):
            cand = sc[sc > dc.CONF]
        assert np.unique(cand).size == cand.size, name + ": equal scores among the candidates"
        out = util.non_max_suppression(x.clone(), dc.CONF, dc.IOU)[0]
        cls = torch.from_numpy(labels[:, 0:1].copy())
        box = torch.from_numpy(labels[:, 1:].copy())
        metric = torch.zeros(out.shape[0], 10, dtype=torch.bool)
        if out.shape[0] and cls.shape[0]:
            target = torch.cat((cls, util.wh2xy(box) * scale), 1)
            assert np.array_equal(dc.bits(target.numpy()), dc.bits(dc.labels_px(labels))), name + ": the label corners"
            metric = util.compute_metric(out[:, :6], target, iou_v)
            # eligible pairs at the lowest threshold: all distinct IoUs (by the restatement's IoU; the fixture holds the reference's tp words)
            iou = torch.from_numpy(dr.pair_iou(out[:, :6].numpy(), target.numpy()))
            el = iou[(iou >= iou_v[0]) & (target[:, 0:1] == out[:, 5])].numpy()
            assert np.unique(el).size == el.size, name + ": equal IoUs among the eligible pairs"
        if out.shape[0]:                                  # the trainer's bookkeeping
            metrics.append((metric, out[:, 4], out[:, 5], cls.squeeze(-1)))
        elif cls.shape[0]:
            metrics.append((metric, *torch.zeros((2, 0)), cls.squeeze(-1)))
        tp = (metric.numpy().astype(np.uint32) << np.arange(10, dtype=np.uint32)[None, :]).sum(1).astype(np.uint32)
        with np.errstate(invalid="ignore"):
            n_cand = int((sc > dc.CONF).sum())
        data[name + "_rows"] = out[:, :6].numpy().astype(np.float32)
        data[name + "_tp"] = tp
        data[name + "_counts"] = np.array((n_cand, min(n_cand, dc.MAX_NMS), out.shape[0]), np.uint32)
        data[name + "_sha256"] = np.array(dc.digest(raw, labels))
        print("%-14s candidates %6d kept %4d labels %d tp@50 %d" % (name, n_cand, out.shape[0], labels.shape[0], int((tp & 1).sum())))
    m = [torch.cat(x, 0).numpy() for x in zip(*metrics)]
    assert np.unique(m[1]).size == m[1].size, "equal conf among the dataset's kept rows"
    assert m[0].any()
    tp, fp, m_pre, m_rec, map50, mean_ap = util.compute_ap(*m)
    curve = chosen[-1]
    top = np.sort(curve)[-2:]
    assert top[1] - top[0] > 1e-9, "the smoothed F1 curve's two largest values are closer than 1e-9"
    classes = np.unique(m[3])
    det_classes = np.unique(m[2])
    assert classes.size >= 3 and np.setdiff1d(classes, det_classes).size >= 1 and np.setdiff1d(det_classes, classes).size >= 1
    data.update(ds_tp=np.asarray(tp, np.float64), ds_fp=np.asarray(fp, np.float64), ds_scores=np.array((m_pre, m_rec, map50, mean_ap), np.float64),
                ds_grid_index=np.array(int(curve.argmax())), ds_classes=classes.astype(np.float32), ds_rows=np.array(m[1].size), ds_labels=np.array(m[3].size))
    print("dataset: rows %d labels %d classes %s  P %.6f R %.6f mAP50 %.6f mAP %.6f  index %d" % (m[1].size, m[3].size, classes.tolist(), m_pre, m_rec, map50, mean_ap, int(curve.argmax())))
    np.savez_compressed(args.out, **data)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
