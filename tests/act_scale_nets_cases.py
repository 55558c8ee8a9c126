"""VP_ACT_SCALE for the detector and the lane network: the cases shared by the emulated (tests/test_act_scale_nets_host.py) and the device
(tests/test_gpu_act_scale_nets.py) suites -- the four hand-written kernels with exponents at the smallest shapes at which they can go wrong, the tie
groups of the two plans, and the whole-engine checks.  TEST INFRASTRUCTURE ONLY.

Inputs keep BOTH planes normal under every exponent used (EXPS: 0 and the two of tests/test_gpu_act_scale.py, 6 and -3): hi in +-(16, 32), lo in
+-[2^-8, 2^-7) (below half an ulp of hi), so split(x * 2^-s) == split(x) * 2^-s plane for plane and a scaled launch sees, after its multiplication,
exactly the fp32 values the unflagged launch sees.  Hence the two kernels with fp32 outputs are compared BIT FOR BIT against the unflagged launch on the
true values; pair outputs are compared as (hi + lo) * 2^s sums under the kernel's own bar (2e-5, tests/autosteer_cases.py), since a re-split is ambiguous
at half-ulp ties."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

EXPS = (0, 6, -3)
X3_BAR = 2e-5           # tests/autosteer_cases.py
NET_BAR = 1e-3          # the networks' parity bar: 1e-3 * max(1, |ref|)
TARGET = 12
GOLDEN = os.path.join(HERE, "golden", "act_scale_nets.npz")
f32 = np.float32


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def normal_pairs(rng, shape):
    """fp32 values that ARE (hi, lo) pairs with both planes normal for every exponent of EXPS (see the module text)"""
    hi = (rng.uniform(16.5, 31.5, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float16).astype(f32)
    lo = (rng.uniform(2.0 ** -8, 0.98 * 2.0 ** -7, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float16).astype(f32)
    x = hi + lo
    assert np.array_equal(x.astype(np.float16).astype(f32), hi)
    return x


def planes(x):
    hi = x.astype(np.float16)
    return hi, (x - hi.astype(f32)).astype(np.float16)


def sums(hi, lo):
    return hi.astype(f32) + lo.astype(f32)


# ------------------------------------------------------------------------------------------------ the four kernels
def check_upsample2_cat(lib, nch, exp):
    """2x4 -> 4x8, `nch` channels from each source at non-zero offsets: the stored planes are the moved stored planes, bit for bit"""
    rng = np.random.default_rng(10 + nch)
    a, b = normal_pairs(rng, (32, 2, 4)), normal_pairs(rng, (32, 4, 8))
    hi, lo = lib.op_upsample2_cat_scaled(a, b, a_off=8, a_nch=nch, b_off=16, b_nch=nch, exp=exp)
    want = np.concatenate([a[8:8 + nch].repeat(2, axis=1).repeat(2, axis=2), b[16:16 + nch]]) * f32(2.0 ** -exp)
    wh, wl = planes(want)
    assert hi.shape == (2 * nch, 4, 8)
    assert np.array_equal(hi.view(np.uint16), wh.view(np.uint16)) and np.array_equal(lo.view(np.uint16), wl.view(np.uint16))


def check_rowpair(lib, cin, replicate, in_exp, out_exp):
    """H = 5 (the odd last row is ignored), W = 8, into channels 32 .. 63 of a 96-channel destination (an alias slice at a non-zero offset)"""
    rng = np.random.default_rng(100 * cin + replicate)
    h, w = 5, 8
    x = normal_pairs(rng, (cin, h, w))
    wt = (rng.normal(0, 1, (32, cin, 2, 1)) * np.sqrt(2.0 / (2 * cin)) * 4.0).astype(f32)   # outputs of a few hundred: SiLU's both sides
    b = rng.normal(0, 10.0, 32).astype(f32)
    d = lambda t: torch.from_numpy(np.asarray(t, np.float64))   # noqa: E731
    want = F.silu(F.conv2d(d(x)[None], d(wt), d(b), stride=(2, 1)))[0].numpy()
    fct = 2 if replicate else 1
    ho, wo = (h // 2) * fct, w * fct
    if replicate:
        want = want.repeat(2, axis=1).repeat(2, axis=2)
    init = normal_pairs(rng, (96, ho, wo))
    plain_hi, plain_lo = lib.op_rowpair_conv(x, wt, b, replicate=replicate, dst=init, dst_off=32)
    hi, lo = lib.op_rowpair_conv(x, wt, b, replicate=replicate, dst=init, dst_off=32, in_exp=in_exp, out_exp=out_exp)
    if in_exp == 0 and out_exp == 0:   # the flagged launch with zero exponents IS the unflagged one
        assert np.array_equal(hi.view(np.uint16), plain_hi.view(np.uint16)) and np.array_equal(lo.view(np.uint16), plain_lo.view(np.uint16))
    got = sums(hi, lo).astype(np.float64) * 2.0 ** out_exp
    err = rel(got[32:64], want)
    print(f"rowpair_conv cin={cin} replicate={replicate} exps ({in_exp}, {out_exp}): {err:.2e} against fp64, "
          f"{rel(got[32:64], sums(plain_hi, plain_lo)[32:64].astype(np.float64)):.2e} against the unflagged launch")
    assert np.isfinite(got).all() and err <= X3_BAR, err
    if replicate:
        for plane in (hi, lo):
            s = plane[32:64].view(np.uint16)
            assert all(np.array_equal(s[:, 0::2, 0::2], s[:, dy::2, dx::2]) for dy in (0, 1) for dx in (0, 1))
    ih, il = planes(init * f32(2.0 ** -out_exp))   # the rest of the destination: untouched
    for sl in (slice(0, 32), slice(64, 96)):
        assert np.array_equal(hi[sl].view(np.uint16), ih[sl].view(np.uint16)) and np.array_equal(lo[sl].view(np.uint16), il[sl].view(np.uint16))


def check_lane_rows(lib, cin, in_exp):
    """H = 2, W = 256: xp / h_vector of the scaled launch equal the unflagged launch's on the true values, bit for bit; both within the bar of fp64"""
    import autosteer_cases

    rng = np.random.default_rng(7 + cin)
    feat = normal_pairs(rng, (cin, 2, 256))
    g = 1.0 / (24.0 * np.sqrt(9.0 * cin))
    kw = dict(c1_w=(rng.normal(0, 3.0 * g, (cin, 3, 3))).astype(f32), c1_b=f32(0.1), c2_w=(rng.normal(0, 2.0 * g, (cin, 3, 3))).astype(f32), c2_b=f32(-0.2),
              h1_w=rng.normal(0, 0.5, 16).astype(f32), h1_b=f32(0.3), h2_w=rng.normal(0, 0.5, 16).astype(f32), h2_b=f32(0.1))
    plain = lib.op_lane_rows_head(feat, **kw)
    got = lib.op_lane_rows_head(feat, in_exp=in_exp, **kw)
    want = autosteer_cases._lane_ref(feat, kw["c1_w"], kw["c1_b"], kw["c2_w"], kw["c2_b"], kw["h1_w"], kw["h1_b"], kw["h2_w"], kw["h2_b"])
    print(f"lane_rows_head cin={cin} in_exp={in_exp}: {rel(got, want):.2e} against fp64; xp {got[0]}")
    assert np.isfinite(got).all() and rel(plain, want) <= X3_BAR and 0.05 < got[0].min() and got[0].max() < 0.95   # not a saturated row softmax
    assert np.array_equal(bits(got), bits(plain))


def check_detect(lib, nc, exps):
    """three levels of 4x8, 2x4 and 1x2 cells: the scaled launch's fp32 rows equal the unflagged launch's on the true values, bit for bit"""
    import autospeed_net_ref as ref

    rng = np.random.default_rng(20 + nc)
    h0, w0 = 4, 8
    total = sum((h0 >> l) * (w0 >> l) for l in range(3))
    box, cls = normal_pairs(rng, (64, total)), normal_pairs(rng, (nc, total))
    plain = lib.op_detect_head_decode(box, cls, h0, w0)
    got = lib.op_detect_head_decode(box, cls, h0, w0, exps=exps)
    levels, off = [], 0
    for l in range(3):
        h, w = h0 >> l, w0 >> l
        levels.append(torch.from_numpy(np.concatenate([box[:, off:off + h * w], cls[:, off:off + h * w]]).reshape(1, 64 + nc, h, w)).double())
        off += h * w
    want = ref.decode({"head.dfl.conv.weight": torch.arange(16, dtype=torch.float64).view(1, 16, 1, 1)}, levels)[0].numpy()
    assert got.shape == want.shape and np.isfinite(got).all() and rel(plain, want) <= 1e-5    # the bar of the kernel's own test
    assert np.array_equal(bits(got), bits(plain)), exps


# ------------------------------------------------------------------------------------------------ tie groups of the two plans
def tie_groups(net, names):
    """The tensors that share one exponent, by the builders' rules: alias slices of one tensor, copies, max-pools, convex combinations, and the movers
    (upsample2_cat ties both sources and the result)."""
    P = "net.p5."
    groups = [[P + "2.cv1", P + "2.cat"], [P + "3.cv1", P + "3.y", P + "3.middle_block.conv2.1"], [P + "3.middle_block.conv1." + s for s in ("qkv", "attn", "v")]]
    for h in (("fpn.h1", "fpn.h2") if net == "autosteer" else ("fpn.h1", "fpn.h2", "fpn.h4", "fpn.h6")):
        g = [h + s for s in (".cat", ".conv1", ".y1", ".res_m.0")]
        if h != "fpn.h6":
            g.append(h + ".y1@cat")
        else:   # C3K inside: its own concatenation, the branch stored into it and the chain copied into it
            groups.append([h + ".res_m.0.cat", h + ".res_m.0.conv2", h + ".res_m.0.res_m.1.conv2"])
        groups.append(g)
    if net == "autosteer":
        groups += [["net.p5.3.cv2", "fpn.cat1", "net.p4.1.ctx2"], ["fpn.h1.conv2", "fpn.cat2", "net.p3.1.ctx2"], ["features", "head.v1", "head.v2"]]
    else:
        groups += [["fpn.cat4", "net.p5.3.cv2", "fpn.h5", "fpn.cat1", "net.p4.1.ctx2"], ["fpn.cat3", "fpn.h3", "fpn.h1.conv2", "fpn.cat2", "net.p3.1.ctx2"]]
    tied = [n for g in groups for n in g]
    assert len(tied) == len(set(tied)) and set(tied) <= set(names), set(tied) - set(names)
    return groups


def check_tie_groups(eng, net):
    """vp_set_act_scales refuses a table in which ONE member of a group differs, and accepts it for every tensor outside the groups: the groups above are
    the plan's, no more and no less."""
    import pytest

    names = [t[0] for t in eng.tensors()]
    groups = tie_groups(net, names)
    tied = {n for g in groups for n in g}
    base = eng.act_scales()
    for i, n in enumerate(names):
        t = base.copy()
        t[i] += 1
        if n in tied:
            with pytest.raises(ValueError, match="tied"):
                eng.set_act_scales(t)
        else:
            eng.set_act_scales(t)
    for g in groups:   # ... and accepts a group that moves together
        t = base.copy()
        t[[names.index(n) for n in g]] += 1
        eng.set_act_scales(t)
    eng.reset_range()


def check_band(net, names, exps, stored, target=TARGET):
    """No stored tensor beyond 2^target; an untied tensor's stored abs-max lies in [2^(target - 1), 2^target); the members of a tie group share one exponent
    and the group's LARGEST member lies in the band (the smaller ones cannot: that is what sharing an exponent means)."""
    lo, hi = 2.0 ** (target - 1), 2.0 ** target
    groups = tie_groups(net, names)
    tied = {n for g in groups for n in g}
    for g in groups:
        idx = [names.index(n) for n in g]
        assert len({int(exps[i]) for i in idx}) == 1, (g, [int(exps[i]) for i in idx])
        assert all(stored[i] < hi for i in idx) and lo <= max(stored[i] for i in idx), (g, [stored[i] for i in idx])
    for i, n in enumerate(names):
        if n not in tied:
            assert lo <= stored[i] < hi, (n, int(exps[i]), stored[i])


def stored_absmax(eng):
    """per tensor: abs-max of the STORED values (vp_tensor_read gives true values: times 2^-s, exact); asserts that none is non-finite"""
    exps = eng.act_scales()
    out = []
    for i in range(len(exps)):
        t = eng.tensor_read(i)
        assert np.isfinite(t).all(), eng.tensors()[i][0]
        out.append(float(np.abs(t).max()) * 2.0 ** -int(exps[i]))
    return np.array(out)


# ------------------------------------------------------------------------------------------------ whole engines (512 x 1024)
class Net:
    """One network kind: engines, the fixture frame and how a frame goes in (AutoSteer: vp_infer; AutoSpeed: vp_detect_infer on an attached detector)."""

    def __init__(self, lib, net):
        import pin_act_scale_nets as pin
        from autoware_vision_pilot_amd import synthetic

        self.lib, self.net, self.pin = lib, net, pin
        self.fix = np.load(GOLDEN)
        h, w, seed = (int(v) for v in self.fix[f"{net}_frame"])
        self.frame = synthetic.synthetic_frame(h, w, seed)
        self.sd = pin.state_dict(net)
        self.gold = np.load(os.path.join(HERE, "golden", f"{net}_net.npz"))
        self.open = []

    def blob(self, case):
        from autoware_vision_pilot_amd import weights as vw

        sd = self.sd if case == "ordinary" else self.pin.ill_scaled(self.sd, str(self.fix[f"{self.net}_block"]), int(self.fix[f"{self.net}_k"]))
        return vw.pack_state_dict(sd)

    def engine(self, blob, **kw):
        eng = self.lib.Engine(self.net, blob, precision="fp16x3", **kw)
        self.open.append(eng)
        if self.net == "autosteer":
            eng.set_input_format(self.lib.VP_BGR8, self.lib.VP_PLANES_RGB)
            return eng, None
        det = self.lib.Detector(512, 1024, max_boxes=10752, max_attrs=8)
        self.open.append(det)
        det.attach(eng)
        return eng, det

    def run(self, eng, det):
        """-> (output tensor, detections or None)"""
        if det is None:
            eng.infer(self.frame)
            return eng.logits().copy(), None
        d, n = det.infer(self.frame, float(self.gold["conf"]), float(self.gold["iou"]))
        return eng.logits().copy(), d[:n].copy()

    def close(self):
        for o in reversed(self.open):
            o.close()
        self.open = []


def check_zero_exponents(N, latency):
    """plan hash and every output of the uncalibrated flagged engine equal the unflagged engine's, bit for bit"""
    blob = N.blob("ordinary")
    plain, flagged = N.engine(blob, plan_latency=latency), N.engine(blob, plan_latency=latency, act_scale=True)
    assert flagged[0].plan_hash() == plain[0].plan_hash() and not flagged[0].act_scales().any()
    (out_p, det_p), (out_f, det_f) = N.run(*plain), N.run(*flagged)
    assert np.array_equal(bits(out_f), bits(out_p))
    if det_p is not None:
        assert np.array_equal(bits(det_f), bits(det_p))
    N.close()


def check_ordinary_band_and_table(N, latency=False):
    """ordinary case within the networks' bar of the golden reference; the band; a shipped table gives the same bits; reset gives the first bits again.
    latency: all three engines on VP_PLAN_LATENCY, whose split-K choices then run through the scaled runtime epilogue"""
    net, fix, gold = N.net, N.fix, N.gold
    blob = N.blob("ordinary")
    plain, a, b = (N.engine(blob, plan_latency=latency, **kw) for kw in ({}, {"act_scale": True}, {"act_scale": True}))
    out_p, det_p = N.run(*plain)
    first, _ = N.run(*a)
    assert np.array_equal(bits(first), bits(out_p))
    h0 = a[0].plan_hash()
    a[0].calibrate_range()
    assert a[0].plan_hash() == h0 == plain[0].plan_hash()   # exponents are data, not plan
    exps = a[0].act_scales()
    assert (exps != 0).any()
    out, det = N.run(*a)
    names = [t[0] for t in a[0].tensors()]
    check_band(net, names, exps, stored_absmax(a[0]))
    if net == "autosteer":
        got, want = out.reshape(2, 64), np.stack([gold["xp_0"], gold["h_0"]])
        print(f"autosteer ordinary (latency plan: {latency}): xp {rel(got[0], want[0]):.2e}, h_vector {rel(got[1], want[1]):.2e} (unflagged {rel(out_p.reshape(2, 64), want):.2e})")
        assert rel(got, want) <= NET_BAR
        assert np.array_equal(got[1] >= 0.5, want[1] >= 0.5)      # the validity decision of every row
    else:
        got, want = out.reshape(8, 10752)[:, ::int(gold["box_step"])], gold["raw_0"]
        print(f"autospeed ordinary (latency plan: {latency}): raw {rel(got, want):.2e} (unflagged {rel(out_p.reshape(8, 10752)[:, ::int(gold['box_step'])], want):.2e}); {len(det)} detections")
        assert rel(got, want) <= NET_BAR
        assert len(det) == len(det_p) == len(gold["det_0"]) and np.array_equal(det[:, 5], det_p[:, 5])
        assert rel(det[:, :5], det_p[:, :5]) <= NET_BAR and rel(det[:, :5], gold["det_0"][:, :5]) <= NET_BAR
    step = int(fix["tap_step"])
    for n in N.pin.HEAD_INPUTS[net]:
        t = a[0].tensor_read(names.index(n)).ravel()[::step]
        assert np.abs(t - fix[f"{net}_ordinary_{n}"]).max() <= NET_BAR * float(fix[f"{net}_ordinary_{n}_absmax"]), n
    again, _ = N.run(*a)     # the replayed graph behind a calibration is bit-stable
    assert np.array_equal(bits(again), bits(out))
    b[0].set_act_scales(exps)
    assert np.array_equal(b[0].act_scales(), exps)
    shipped, det_b = N.run(*b)
    assert np.array_equal(bits(shipped), bits(out))
    if det is not None:
        assert np.array_equal(bits(det_b), bits(det))
    a[0].reset_range()
    assert not a[0].act_scales().any()
    back, _ = N.run(*a)
    assert np.array_equal(bits(back), bits(out_p))
    N.close()


def check_range_case(N):
    """The ill-scaled checkpoint of the fixture: the unflagged engine reports VP_ERR_RANGE (the probe reads the output tensor, which the overflow reaches in
    both networks -- and a head input read back is non-finite as well); the calibrated engine meets the fixture's vectors."""
    net, fix, lib = N.net, N.fix, N.lib
    blob = N.blob("range")
    plain, a = N.engine(blob), N.engine(blob, act_scale=True)
    import pytest

    with pytest.raises(lib.VpRangeError):
        N.run(*plain)
    names = [t[0] for t in plain[0].tensors()]
    assert not np.isfinite(plain[0].tensor_read(names.index(N.pin.HEAD_INPUTS[net][0]))).all()
    with pytest.raises(lib.VpRangeError):      # zero exponents: the unflagged engine's launches
        N.run(*a)
    a[0].calibrate_range()
    out, _ = N.run(*a)
    assert np.isfinite(out).all()
    exps = a[0].act_scales()
    first = str(fix[f"{net}_first_beyond"])
    assert exps[names.index(first)] > 0, (first, int(exps[names.index(first)]))
    check_band(net, names, exps, stored_absmax(a[0]))
    step = int(fix["tap_step"])
    compared = [str(n) for n in fix[f"{net}_compared"]]
    assert set(N.pin.HEAD_INPUTS[net]) <= set(compared)
    finals = {"xp": lambda o: o.reshape(2, 64)[0], "h_vector": lambda o: o.reshape(2, 64)[1],
              "raw_box": lambda o: o.reshape(8, 10752)[:4, ::int(fix["box_step"])], "raw_cls": lambda o: o.reshape(8, 10752)[4:, ::int(fix["box_step"])]}
    for n in compared:
        want = fix[f"{net}_range_{n}"]
        if n in N.pin.HEAD_INPUTS[net]:
            got = a[0].tensor_read(names.index(n)).ravel()[::step]
            err = float(np.abs(got - want).max() / float(fix[f"{net}_range_{n}_absmax"]))
        else:
            err = rel(finals[n](out), want)
        print(f"{net} range case (block {fix[f'{net}_block']}, k = {int(fix[f'{net}_k'])}): {n} {err:.2e}")
        assert err <= NET_BAR, (n, err)
    N.close()
