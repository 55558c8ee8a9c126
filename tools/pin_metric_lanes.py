#!/usr/bin/env python3
"""Pin the lane-metric cases: (re)generates tests/golden/metric_lanes.npz from the reference's OWN code, on the CPU.

Usage:  python tools/pin_metric_lanes.py [--out PATH]

Runs only where the reference checkout is present (VP_REFERENCE, default /root/reference).
  Lane masks: the EgoLanesTrainer methods calc_ego_lanes_loss, calc_multi_scale_edge_loss, calc_segmentation_loss and calc_edge_loss
    (Models/training/ego_lanes_trainer.py) are bound to a stub object that holds the two gradient filters, the prediction and the ground truth; the
    module's imports that this environment lacks or that the four methods never touch (torchvision, cv2, tensorboard, matplotlib, the trainer's own
    package imports) are stand-in modules.  Each case of tests/metric_lanes_cases.py runs twice: in float32, the trainer's arithmetic, and with every
    tensor in float64.  The per-plane parts are the same methods called per plane.
  compute_vector_ap (Models/training/auto_steer_util.py) runs on the AP cases.
The per-line stage of the AutoSteer trainer's val() needs CUDA and a dataset: it is restated in tests/metric_lanes_cases.py, not pinned."""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("VP_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metric_lanes_cases as lc  # noqa: E402


def stand_in(name, **attrs):
    parts = name.split(".")
    for i in range(1, len(parts) + 1):
        full = ".".join(parts[:i])
        if full not in sys.modules:
            sys.modules[full] = types.ModuleType(full)
        if i > 1:
            setattr(sys.modules[".".join(parts[:i - 1])], parts[i - 1], sys.modules[full])
    for k, v in attrs.items():
        setattr(sys.modules[name], k, v)


def load_reference():
    path = os.path.join(REFERENCE, "Models", "training")
    if not os.path.exists(os.path.join(path, "ego_lanes_trainer.py")):
        raise SystemExit("the reference checkout is not present at %s (VP_REFERENCE)" % REFERENCE)
    stand_in("torchvision", transforms=types.SimpleNamespace())
    stand_in("torchvision.transforms")
    stand_in("cv2")
    stand_in("torch.utils.tensorboard", SummaryWriter=object)
    stand_in("matplotlib")
    stand_in("matplotlib.pyplot")
    stand_in("model_components")
    stand_in("model_components.ego_lanes_network", EgoLanesNetwork=object)
    stand_in("data_utils")
    stand_in("data_utils.augmentations", Augmentations=object)
    stand_in("data_utils.load_data_ego_lanes", VALID_DATASET_LIST=())
    sys.path.insert(0, path)
    import auto_steer_util
    import ego_lanes_trainer

    return ego_lanes_trainer.EgoLanesTrainer, auto_steer_util


class Stub:
    """what the four loss methods read of a trainer"""

    def __init__(self, Trainer, logits, planes, dtype):
        for name in ("calc_ego_lanes_loss", "calc_multi_scale_edge_loss", "calc_segmentation_loss", "calc_edge_loss"):
            setattr(self, name, types.MethodType(getattr(Trainer, name), self))
        self.gx_filter = torch.tensor(lc.GX, dtype=dtype).view(1, 1, 3, 3)
        self.gy_filter = torch.tensor(lc.GY, dtype=dtype).view(1, 1, 3, 3)
        self.pred_binary_seg_tensor = torch.as_tensor(logits, dtype=dtype)[None]
        self.egolanes_tensor = torch.as_tensor(planes, dtype=dtype)[None]


def run(Trainer, logits, planes, dtype):
    """the record's values by the trainer's methods: the frame score from calc_ego_lanes_loss; per plane the BCE, the plane loss as the method adds it, and
    the five edge losses from calc_edge_loss on the trainer's own pyramid (its relu, Threshold and AvgPool2d objects)"""
    s = Stub(Trainer, logits, planes, dtype)
    out = {"bce": [], "edge": [], "loss": [], "score": s.calc_ego_lanes_loss().item()}
    down, thr = torch.nn.AvgPool2d(2, stride=2), torch.nn.Threshold(0.0, 1.0, inplace=False)
    for c in range(3):
        pred, gt = s.pred_binary_seg_tensor[:, c], s.egolanes_tensor[:, c]
        bce = s.calc_segmentation_loss(pred, gt)
        multi = s.calc_multi_scale_edge_loss(pred, gt)
        r = torch.relu(pred)
        a, b = thr(r), gt
        e = [s.calc_edge_loss(r, gt)]
        for _ in range(4):
            a, b = down(a), down(b)
            e.append(s.calc_edge_loss(a, b))
        assert ((e[0] + e[1] + e[2] + e[3] + e[4]) / 5 - multi).abs().item() == 0.0, "the five scales are calc_multi_scale_edge_loss's"
        out["bce"].append(bce.item())
        out["edge"].append([v.item() for v in e])
        out["loss"].append((multi + bce).item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=lc.GOLDEN)
    args = ap.parse_args()
    Trainer, util = load_reference()
    data = {}
    for prefix, shapes, make in (("exact_", lc.EXACT_SHAPES, lc.exact_inputs), ("general_", lc.GENERAL_SHAPES, lc.general_inputs)):
        for shape in shapes:
            lg, bits = make(shape)
            planes = lc.planes_of_bits(bits)
            r32, r64 = run(Trainer, lg, planes, torch.float32), run(Trainer, lg, planes, torch.float64)
            own = lc.lanes_ref(lg, planes, torch.float64)
            assert np.allclose(lc.pack(own), lc.pack(r64), rtol=1e-12, atol=0), "the restatement is the trainer's arithmetic"
            k = prefix + lc.key(shape)
            data[k + "_logits"], data[k + "_bits"], data[k + "_ref32"], data[k + "_ref64"] = lg, bits, lc.pack(r32), lc.pack(r64)
            print("%-16s score fp32 %.7f fp64 %.9f |diff| %.2e  worst edge diff %.2e" % (k, r32["score"], r64["score"], abs(r32["score"] - r64["score"]),
                                                                                   np.abs(np.array(r32["edge"]) - np.array(r64["edge"])).max()))
    for name in lc.AP_CASES:
        tp, conf = lc.ap_inputs(name)
        tp_dict = {t: [int((w >> k) & 1) for w in tp] for k, t in enumerate(lc.THR)}
        fp_dict = {t: [1 - v for v in tp_dict[t]] for t in lc.THR}
        target = [np.zeros(64, np.float32)] * tp.size                      # compute_vector_ap reads its length only
        m_pre, m_rec, mean_ap, map50 = util.compute_vector_ap(tp_dict, fp_dict, [float(c) for c in conf], target)
        data["ap_" + name] = np.array((m_pre, m_rec, mean_ap, map50), np.float64)
        data["ap_" + name + "_tp"], data["ap_" + name + "_conf"] = tp, conf
        print("ap %-5s P %.9f R %.9f mAP %.9f mAP50 %.9f" % (name, m_pre, m_rec, mean_ap, map50))
    np.savez_compressed(args.out, **data)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
