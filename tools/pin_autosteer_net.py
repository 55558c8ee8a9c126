"""Pin tests/autosteer_net_ref.py against the reference's OWN AutoSteer 2.0 module and write tests/golden/autosteer_net.npz.

Runs only where the reference tree is importable:  python tools/pin_autosteer_net.py /path/to/reference [--search]
  1. AutoSteerNetwork().build_model('n'), load_state_dict(strict=True) of synthetic.make_autosteer_state_dict (+ zero num_batches_tracked), eval();
  2. its outputs on the u8 / 255 RGB planes of the synthetic 512 x 1024 frames below must equal the restatement's at distance 0.0 -- xp, h_vector, and
     the neck's h1 / h2 outputs and the head's `features` tensor, taken from the module by forward hooks;
  3. the reference's outputs meet the conditions the engine tests rely on (check_conditions);
  4. the vectors are written: both outputs in full, sub-sampled taps, seeds.
--search prints the grid points (head gains x frame seeds) at which the conditions hold; the gains in synthetic.py and FRAMES below are one of them.
"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WEIGHT_SEED = 5
FRAME_SEEDS = (22, 23)   # synthetic.synthetic_frame(512, 1024, seed): chosen so that check_conditions holds
TAP_STEP = 4099          # a prime: the sub-sampled taps walk through every channel and column
MARGIN = 2e-3
TAPS = ("fpn.h1.conv2", "fpn.h2.conv2", "features")


def conditions(xp, h):
    """xp spread over the rows (std >= 0.05, max - min >= 0.2); h_vector with >= 8 rows on each side of 0.5 and none within MARGIN of it, so that the
    `>= 0.5` decision of visualizations/AutoSteer/video_visualization.py:29 is the same for an engine within 1e-3."""
    return (float(xp.std()) >= 0.05 and float(xp.max() - xp.min()) >= 0.2 and int((h >= 0.5).sum()) >= 8 and int((h < 0.5).sum()) >= 8 and
            float(np.abs(h - 0.5).min()) > MARGIN)


def search():
    """Head gains x frame seeds: the features do not depend on the head gains, so they are computed once per frame."""
    import torch

    import autosteer_net_ref as ref
    from autoware_vision_pilot_amd import synthetic

    feats = {}
    for fs in range(21, 27):
        _, taps = ref.forward(synthetic.make_autosteer_state_dict(WEIGHT_SEED), ref.preprocess(synthetic.synthetic_frame(ref.NET_H, ref.NET_W, fs)))
        feats[fs] = torch.from_numpy(taps["features"])[None]
    for c1, c2, h1, h2, h2b in itertools.product((6.0, 12.0), (2.0, 4.0, 8.0), (1.0, 2.0), (1.0, 2.0, 4.0), (-0.5, 0.0, 0.5, 1.0)):
        sd = ref.to_torch(synthetic.make_autosteer_state_dict(WEIGHT_SEED, {"c1": c1, "c2": c2, "h1": h1, "h2": h2, "h2_bias": h2b}))
        good = []
        for fs, f in feats.items():
            with torch.no_grad():
                xp, h = ref.head(sd, f)
            if conditions(xp.reshape(-1).numpy(), h.reshape(-1).numpy()):
                good.append(fs)
        if len(good) >= 2:
            print(f"c1 {c1} c2 {c2} h1 {h1} h2 {h2} h2_bias {h2b}: frame seeds {good}")


def main(reference_root):
    import torch

    import autosteer_net_ref as ref
    from autoware_vision_pilot_amd import synthetic

    sys.path.insert(0, reference_root)
    from Models.model_components.auto_steer.auto_steer_network import AutoSteerNetwork

    sd = synthetic.make_autosteer_state_dict(WEIGHT_SEED)
    model = AutoSteerNetwork().build_model("n")
    want_keys = [k for k in model.state_dict() if not k.endswith("num_batches_tracked")]
    assert want_keys == list(sd), "key list / order differs from the reference module's"
    full = {k: torch.from_numpy(v) for k, v in sd.items()}
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            full[k] = torch.zeros_like(v)
    model.load_state_dict(full, strict=True)
    model.eval()
    taps = {}
    model.fpn.h1.register_forward_hook(lambda m, i, o: taps.update({"fpn.h1.conv2": o.detach().clone()}))
    model.fpn.h2.register_forward_hook(lambda m, i, o: taps.update({"fpn.h2.conv2": o.detach().clone()}))
    model.head.c1.register_forward_hook(lambda m, i, o: taps.update({"features": i[0].detach().clone()}))
    out = {"weight_seed": WEIGHT_SEED, "frame_seeds": np.array(FRAME_SEEDS), "tap_step": TAP_STEP}
    for fi, seed in enumerate(FRAME_SEEDS):
        frame = synthetic.synthetic_frame(ref.NET_H, ref.NET_W, seed)
        x = ref.preprocess(frame)
        t = torch.from_numpy(np.ascontiguousarray(frame[:, :, ::-1])).permute(2, 0, 1).float().div(255)   # torchvision to_tensor's arithmetic
        assert np.array_equal(t.numpy(), x)
        with torch.no_grad():
            xp_mod, h_mod = (o.reshape(-1).numpy() for o in model(t[None]))
        (xp_ref, h_ref), taps_ref = ref.forward(sd, x)
        d = max(float(np.abs(xp_mod - xp_ref).max()), float(np.abs(h_mod - h_ref).max()))
        assert d == 0.0, f"restatement differs from the module: {d}"
        for name in TAPS:
            assert float(np.abs(taps[name][0].numpy() - taps_ref[name]).max()) == 0.0, name
        assert conditions(xp_mod, h_mod), (xp_mod, h_mod)
        print(f"frame {fi} (seed {seed}): distance 0.0; xp std {xp_mod.std():.3f} range {xp_mod.min():.3f} .. {xp_mod.max():.3f}; h_vector {int((h_mod >= 0.5).sum())} rows "
              f">= 0.5, {int((h_mod < 0.5).sum())} below, nearest to 0.5 at {np.abs(h_mod - 0.5).min():.4f}")
        out[f"xp_{fi}"], out[f"h_{fi}"] = xp_mod, h_mod
        for name in TAPS:
            out[f"{name}_{fi}"] = taps_ref[name].ravel()[::TAP_STEP].copy()
    path = os.path.join(ROOT, "tests", "golden", "autosteer_net.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[2] == "--search":
        search()
    elif len(sys.argv) == 2:
        main(sys.argv[1])
    else:
        sys.exit(__doc__)
