#!/usr/bin/env python3
"""Pin the VP_ACT_SCALE cases of the AutoSpeed and AutoSteer engines: (re)generates tests/golden/act_scale_nets.npz.

Usage:  python tools/pin_act_scale_nets.py [--out PATH] [--no-reference]

Everything is computed on the CPU by the restatements tests/autospeed_net_ref.py / tests/autosteer_net_ref.py (each pinned at distance 0.0 against the
reference's own nn.Module by tools/pin_autospeed_net.py / pin_autosteer_net.py).  Where the reference checkout is importable (VP_REFERENCE, default
/root/reference) the range-case outputs are checked against those modules again, at distance 0.0, with the ill-scaled checkpoint loaded
(--no-reference: never; the bytes written are the same either way).  The file holds seeds, the recipe and expected vectors only -- no frames, no
checkpoints.  Per network:

  ordinary case  the weight seed and the first frame of the network's existing golden file (autospeed_net.npz / autosteer_net.npz, which stay the
                 reference of that case); the head inputs are added here, sub-sampled, because those files do not hold the detector's.
  range case     an ill-scaled checkpoint the fp32 reference answers: BatchNorm weight and bias of ONE Conv block of the backbone (BLOCKS, first to
                 last) times 2^k, with the smallest k for which (a) some intermediate of the fp32 run exceeds 65504 and (b) every BN-folded weight
                 stays inside the fp16 range (the load is not refused); asserted here together with: every reference output is finite.  Intermediates
                 = the output of every Conv / CTX block and attention stage the restatement names (what the engines store).  Recorded: the block, k,
                 the first tensor beyond range and its abs-max, and the reference's own fp32-against-fp64 distance of every compared vector.
  compared       the last stored tensors in front of the head (AutoSteer: `features`; AutoSpeed: box / cls inputs of the three levels), distance
                 relative to the tensor's abs-max; and the final outputs where their fp32-against-fp64 distance is below 4e-4 (0.4 of the 1e-3 bar: the
                 precedent of autodrive_range.npz) -- a saturated row softmax / sigmoid makes a final output discontinuous, and such a vector is listed
                 in `<net>_left_out` BY NAME.  If a block leaves no head input comparable the next block is tried; no bar is widened.
"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

GOLDEN = os.path.join(ROOT, "tests", "golden", "act_scale_nets.npz")
WEIGHT_SEED = 5                                  # tools/pin_autospeed_net.py / pin_autosteer_net.py
FRAMES = {"autospeed": (720, 1280, 21), "autosteer": (512, 1024, 22)}   # (h, w, seed): frame 0 of the two golden files
BLOCKS = ("net.p1", "net.p2.0", "net.p3.0", "net.p4.0", "net.p5.0")      # the backbone's first Conv block, then the stages' own
K_MAX = 24
FP16_MAX = 65504.0
DIST_MAX = 4e-4                                  # the reference's own fp32-against-fp64 distance must stay below 0.4 of the 1e-3 bar
TAP_STEP = 197                                   # a prime: the sub-sampled taps walk through every channel and column
BOX_STEP = 11                                    # the detector's final rows at every 11th anchor, as autospeed_net.npz holds them
HEAD_INPUTS = {"autosteer": ("features",), "autospeed": tuple(f"head.{b}.{i}.{j}" for i in range(3) for b, j in (("box", 2), ("cls", 4)))}
FINALS = {"autosteer": ("xp", "h_vector"), "autospeed": ("raw_box", "raw_cls")}


def save_npz(path, arrays):
    """np.savez without the wall-clock time stamps of its zip entries: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def state_dict(net):
    from autoware_vision_pilot_amd import synthetic

    return (synthetic.make_autospeed_state_dict if net == "autospeed" else synthetic.make_autosteer_state_dict)(WEIGHT_SEED)


def network_input(net):
    """The fp32 planes the network reads: the detector's letterboxed tensor, the lane network's u8 / 255 planes."""
    import autosteer_net_ref
    from autoware_vision_pilot_amd import synthetic
    from oracle import autospeed

    h, w, seed = FRAMES[net]
    frame = synthetic.synthetic_frame(h, w, seed)
    return autospeed.preprocess(frame, 512, 1024)[0] if net == "autospeed" else autosteer_net_ref.preprocess(frame)


def ill_scaled(sd, block, k):
    out = dict(sd)
    for s in (".norm.weight", ".norm.bias"):
        out[block + s] = (sd[block + s] * np.float32(2.0 ** k)).astype(np.float32)
    return out


def folded_weight_absmax(sd):
    """max |w * gamma / sqrt(var + eps)| over every Conv + BatchNorm block: what the engine splits into fp16 planes at load."""
    from oracle.autodrive import BN_EPS

    worst = 0.0
    for key in sd:
        if key.endswith(".norm.weight"):
            p = key[:-len(".norm.weight")]
            g = sd[key].astype(np.float64) / np.sqrt(sd[p + ".norm.running_var"].astype(np.float64) + BN_EPS)
            worst = max(worst, float(np.abs(sd[p + ".conv.weight"].astype(np.float64) * g.reshape(-1, 1, 1, 1)).max()))
    return worst


class Recorder:
    """abs-max of every named intermediate, in network order: the restatements' Conv and CTX blocks are wrapped while a forward runs."""

    def __init__(self):
        self.seen = []

    def __enter__(self):
        import autospeed_net_ref
        import autosteer_net_ref
        from oracle import autodrive

        self.mods = (autodrive, autospeed_net_ref, autosteer_net_ref)
        self.saved = [(m, n, getattr(m, n)) for m in self.mods for n in ("_conv_bn_act", "ctx_block") if hasattr(m, n)]
        conv, ctx = autodrive._conv_bn_act, autodrive.ctx_block

        def conv_rec(sd, p, x, *a, **kw):
            y = conv(sd, p, x, *a, **kw)
            self.seen.append((p, float(y.abs().max())))
            return y

        def ctx_rec(sd, p, x, h, w):
            y = ctx(sd, p, x, h, w)
            self.seen.append((p + ".ctx2", float(y.abs().max())))
            return y

        for m, n, _ in self.saved:
            setattr(m, n, conv_rec if n == "_conv_bn_act" else ctx_rec)
        return self

    def __exit__(self, *exc):
        for m, n, f in self.saved:
            setattr(m, n, f)


def run(net, sd, x, dtype):
    """-> ({name: numpy array} of head inputs and final outputs, [(intermediate, abs-max)] in network order)"""
    import autospeed_net_ref as sp
    import autosteer_net_ref as st

    tsd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in sd.items()}
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).reshape(1, 3, 512, 1024).to(dtype)
    out = {}
    with torch.no_grad(), Recorder() as rec:
        if net == "autosteer":
            p2, p3, _ = st.neck(tsd, *st.backbone(tsd, xt))
            feat = st.features(tsd, p2, p3)
            rec.seen.append(("features", float(feat.abs().max())))
            xp, hgt = st.head(tsd, feat)
            out = {"features": feat[0], "xp": xp.reshape(-1), "h_vector": hgt.reshape(-1)}
        else:
            levels = sp.head_levels(tsd, list(sp.neck(tsd, *sp.backbone(tsd, xt))))
            raw = sp.decode(tsd, levels)[0]
            for i, lv in enumerate(levels):
                out[f"head.box.{i}.2"], out[f"head.cls.{i}.4"] = lv[0, :64], lv[0, 64:]
                rec.seen += [(f"head.box.{i}.2", float(lv[0, :64].abs().max())), (f"head.cls.{i}.4", float(lv[0, 64:].abs().max()))]
            out["raw_box"], out["raw_cls"] = raw[:4], raw[4:]
    return {k: v.numpy() for k, v in out.items()}, rec.seen


def distance(net, name, a, b):
    """|a - b| relative to the tensor's abs-max for a head input, to max(1, |b|) per element for a final output"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    if name in HEAD_INPUTS[net]:
        return float(np.abs(a - b).max() / np.abs(b).max())
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def range_case(net, sd, x, log=print):
    """the first block, and for it the smallest k, that meets the recipe's conditions -> (block, k, fp32 vectors, fp64 vectors, first beyond, its abs-max)"""
    for block in BLOCKS:
        for k in range(1, K_MAX + 1):
            sdk = ill_scaled(sd, block, k)
            if folded_weight_absmax(sdk) > FP16_MAX:
                log(f"{net}: {block} k = {k}: a folded weight leaves the fp16 range -- next block")
                break
            v32, seen = run(net, sdk, x, torch.float32)
            beyond = [(n, a) for n, a in seen if not a <= FP16_MAX]
            if not beyond:
                continue
            if not all(np.isfinite(v).all() for v in v32.values()):
                log(f"{net}: {block} k = {k}: the fp32 reference is not finite -- next block")
                break
            v64, _ = run(net, sdk, x, torch.float64)
            dist = {n: distance(net, n, v32[n], v64[n]) for n in v32}
            if not all(dist[n] < DIST_MAX for n in HEAD_INPUTS[net]):
                log(f"{net}: {block} k = {k}: head inputs not comparable {dist} -- next block")
                break
            return block, k, v32, dist, beyond[0]
    raise AssertionError(f"{net}: no block of {BLOCKS} gives a range case")


def check_against_reference(net, sd, x, v32):
    """the ill-scaled checkpoint through the reference's OWN module: the restatement's final outputs at distance 0.0"""
    sys.path.insert(0, REFERENCE)
    if net == "autospeed":
        from autoware_vision_pilot_amd import synthetic
        from Models.model_components.auto_speed.auto_speed_network import AutoSpeedNetwork

        model = AutoSpeedNetwork().build_model("n", synthetic.AS_NUM_CLASSES)
    else:
        from Models.model_components.auto_steer.auto_steer_network import AutoSteerNetwork

        model = AutoSteerNetwork().build_model("n")
    full = {k: torch.from_numpy(v) for k, v in sd.items()}
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            full[k] = torch.zeros_like(v)
    model.load_state_dict(full, strict=True)
    model.eval()
    with torch.no_grad():
        y = model(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).reshape(1, 3, 512, 1024))
    if net == "autospeed":
        got = {"raw_box": y[0, :4].numpy(), "raw_cls": y[0, 4:].numpy()}
    else:
        got = {"xp": y[0].reshape(-1).numpy(), "h_vector": y[1].reshape(-1).numpy()}
    for n, g in got.items():
        assert np.array_equal(g, v32[n]), f"{net}: the restatement's {n} differs from the reference module's on the ill-scaled checkpoint"


def compute(log=print, with_reference=False):
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {"weight_seed": np.int64(WEIGHT_SEED), "tap_step": np.int64(TAP_STEP), "box_step": np.int64(BOX_STEP), "blocks": np.array(BLOCKS)}
    for net in ("autospeed", "autosteer"):
        sd, x = state_dict(net), network_input(net)
        out[f"{net}_frame"] = np.array(FRAMES[net], dtype=np.int64)
        v32, seen = run(net, sd, x, torch.float32)
        assert all(a <= FP16_MAX for _, a in seen), "the ordinary case stays inside the fp16 range"
        for n in HEAD_INPUTS[net]:
            out[f"{net}_ordinary_{n}"] = v32[n].ravel()[::TAP_STEP].astype(np.float32)
            out[f"{net}_ordinary_{n}_absmax"] = np.float32(np.abs(v32[n]).max())
        block, k, r32, dist, (first, first_amax) = range_case(net, sd, x, log)
        assert folded_weight_absmax(ill_scaled(sd, block, k)) <= FP16_MAX and first_amax > FP16_MAX and all(np.isfinite(v).all() for v in r32.values())
        if with_reference:
            check_against_reference(net, ill_scaled(sd, block, k), x, r32)
        compared = list(HEAD_INPUTS[net]) + [n for n in FINALS[net] if dist[n] < DIST_MAX]
        left_out = [n for n in FINALS[net] if not dist[n] < DIST_MAX]
        assert set(HEAD_INPUTS[net]) <= set(compared)
        out[f"{net}_block"], out[f"{net}_k"] = np.array(block), np.int64(k)
        out[f"{net}_first_beyond"], out[f"{net}_first_beyond_absmax"] = np.array(first), np.float64(first_amax)
        out[f"{net}_compared"], out[f"{net}_left_out"] = np.array(compared), np.array(left_out, dtype="<U16")
        for n in HEAD_INPUTS[net] + FINALS[net]:
            out[f"{net}_dist_{n}"] = np.float64(dist[n])
        for n in compared:
            full = r32[n].astype(np.float32)
            out[f"{net}_range_{n}"] = full.ravel()[::TAP_STEP].copy() if n in HEAD_INPUTS[net] else (full[:, ::BOX_STEP].copy() if full.ndim == 2 else full)
            if n in HEAD_INPUTS[net]:
                out[f"{net}_range_{n}_absmax"] = np.float32(np.abs(full).max())
        log(f"{net}: block {block}, k = {k}; first beyond range: {first} (abs-max {first_amax:.4g}); fp32 against fp64: " +
            ", ".join(f"{n} {dist[n]:.2e}" for n in dist) + f"; compared {compared}; left out {left_out}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--no-reference", action="store_true", help="restatement only, even where the reference checkout is importable")
    args = ap.parse_args()
    have_ref = not args.no_reference and os.path.isdir(os.path.join(REFERENCE, "Models", "model_components", "auto_steer"))
    if not have_ref and not args.no_reference:
        print("the reference checkout is not on this machine: restatement only")
    save_npz(args.out, compute(with_reference=have_ref))
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
