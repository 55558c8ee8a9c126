"""Pin tests/autospeed_net_ref.py against the reference's OWN detector module and write tests/golden/autospeed_net.npz.

Runs only where the reference tree is importable:  python tools/pin_autospeed_net.py /path/to/reference
  1. AutoSpeedNetwork().build_model('n', 4), load_state_dict(strict=True) of synthetic.make_autospeed_state_dict (+ zero num_batches_tracked), eval();
  2. its output on the letterboxed tensors of the synthetic frames below must equal the restatement's at distance 0.0 (raw and neck taps: the
     taps come from the module's own fpn by a forward hook);
  3. the frames meet the conditions the detection tests rely on (candidate count, no score or IoU within 2e-3 of a threshold);
  4. the vectors are written: raw of the module at every 11th box, sub-sampled neck taps, the kept detections of oracle/autospeed.py's decode of the
     module's raw, seeds and thresholds.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WEIGHT_SEED = 5
FRAMES = ((720, 1280, 21), (1080, 1920, 25))   # (h, w, seed) of synthetic.synthetic_frame: chosen so that check_conditions holds
CONF, IOU = 0.4, 0.65   # thresholds the fixture frames clear by the margin below (searched over a small grid)
BOX_STEP, TAP_STEP = 11, 197
MARGIN = 2e-3


def check_conditions(raw, geom, hw):
    """20..2000 candidates above CONF, no class score within MARGIN of CONF, no same-class candidate pair with an IoU within MARGIN of IOU."""
    from oracle import autospeed

    best = raw[4:].max(axis=0)
    n = int((best >= CONF).sum())
    assert 20 <= n <= 2000, n
    assert np.abs(raw[4:] - np.float32(CONF)).min() > MARGIN, float(np.abs(raw[4:] - np.float32(CONF)).min())
    det = autospeed.postprocess(raw, CONF, 2.0, geom[0], geom[1], geom[2], hw[1], hw[0])   # IoU threshold above 1: every candidate, sorted
    gap = 1.0
    for i in range(len(det)):
        for j in range(i + 1, len(det)):
            if det[i, 5] == det[j, 5]:
                gap = min(gap, abs(float(autospeed.iou(det[i, :4], det[j, :4])) - IOU))
    assert gap > MARGIN, gap
    return n, gap


def reference_module(reference_root, sd):
    """the reference's own AutoSpeedNetwork ('n', the synthetic class count) with the state dict `sd` loaded strictly, in eval mode"""
    import torch

    from autoware_vision_pilot_amd import synthetic

    sys.path.insert(0, reference_root)
    from Models.model_components.auto_speed.auto_speed_network import AutoSpeedNetwork

    model = AutoSpeedNetwork().build_model("n", synthetic.AS_NUM_CLASSES)
    want_keys = [k for k in model.state_dict() if not k.endswith("num_batches_tracked")]
    assert want_keys == list(sd), "key list / order differs from the reference module's"
    assert len(model.state_dict()) == 375 and sum(k.startswith("net.") for k in model.state_dict()) == 116
    full = {k: torch.from_numpy(v) for k, v in sd.items()}
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            full[k] = torch.zeros_like(v)
    model.load_state_dict(full, strict=True)
    model.eval()
    return model


def main(reference_root):
    import torch

    import autospeed_net_ref as ref
    from autoware_vision_pilot_amd import synthetic
    from oracle import autospeed

    sd = synthetic.make_autospeed_state_dict(WEIGHT_SEED)
    model = reference_module(reference_root, sd)
    taps = {}
    model.fpn.register_forward_hook(lambda m, i, o: taps.update(fpn=[t.detach().clone() for t in o]))
    out = {"weight_seed": WEIGHT_SEED, "frames": np.array(FRAMES), "conf": np.float32(CONF), "iou": np.float32(IOU), "box_step": BOX_STEP, "tap_step": TAP_STEP}
    for fi, (h, w, seed) in enumerate(FRAMES):
        frame = synthetic.synthetic_frame(h, w, seed)
        x, geom = autospeed.preprocess(frame, ref.NET_H, ref.NET_W)
        with torch.no_grad():
            raw_mod = model(torch.from_numpy(x)[None])[0].numpy()
        raw_ref, taps_ref = ref.forward(sd, x)
        d = float(np.abs(raw_mod - raw_ref).max())
        assert d == 0.0, f"restatement differs from the module: {d}"
        for a, b in zip(taps["fpn"], taps_ref):
            assert float(np.abs(a[0].numpy() - b).max()) == 0.0
        n, gap = check_conditions(raw_mod, geom, (h, w))
        det = autospeed.postprocess(raw_mod, CONF, IOU, geom[0], geom[1], geom[2], w, h)
        print(f"frame {fi} ({h}x{w}, seed {seed}): distance 0.0, {n} candidates, {len(det)} kept, IoU gap {gap:.4f}, max score {raw_mod[4:].max():.3f}")
        out[f"raw_{fi}"] = raw_mod[:, ::BOX_STEP].copy()
        for name, t in zip(("p3", "p4", "p5"), taps_ref):
            out[f"{name}_{fi}"] = t.ravel()[::TAP_STEP].copy()
        out[f"det_{fi}"] = det
    path = os.path.join(ROOT, "tests", "golden", "autospeed_net.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
