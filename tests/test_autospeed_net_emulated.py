"""The AutoSpeed detector network (VP_AUTOSPEED) on the CPU: the real engine and kernels on the HIP-on-CPU emulation (tests/emul)
against tests/autospeed_net_ref.py, the restatement pinned to the reference's own module (tests/golden/autospeed_net.npz); the three new kernels
alone; the plan against tests/golden/kernel_plan_autospeed.json; the backbone launches against AutoDrive's."""
import ctypes as ct
import ctypes.util
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
GOLDEN = os.path.join(HERE, "golden", "autospeed_net.npz")


@pytest.fixture(scope="module")
def emu_lib():
    import build as emul_build

    from autoware_vision_pilot_amd import lib

    if not os.path.exists(emul_build.CLANG):
        pytest.skip("host clang++ of the ROCm toolchain not found")
    so = ct.CDLL(emul_build.build(), mode=os.RTLD_LOCAL | os.RTLD_NOW)     # never RTLD_GLOBAL: same symbol names as libvp_hip.so
    for name, (res, args) in lib._SIGS.items():
        fn = getattr(so, name)
        fn.restype, fn.argtypes = res, args
    saved = lib._lib
    lib._lib = so
    yield lib
    lib._lib = saved


def _rel(got, ref):
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def test_autospeed_engine_end_to_end_on_cpu(emu_lib):
    """kind 5, fp16x3, one frame: raw and the neck taps within 1e-3 * max(1, |ref|) of the restatement, and of the reference module's own vectors."""
    import autospeed_net_ref as ref
    from autoware_vision_pilot_amd import synthetic, weights as vw
    from oracle import autospeed

    g = np.load(GOLDEN)
    h, w, seed = (int(v) for v in g["frames"][0])
    sd = synthetic.make_autospeed_state_dict(int(g["weight_seed"]))
    x, _ = autospeed.preprocess(synthetic.synthetic_frame(h, w, seed), ref.NET_H, ref.NET_W)
    want, taps = ref.forward(sd, x)
    eng = emu_lib.Engine("autospeed", vw.pack_state_dict(sd), precision="fp16x3")
    try:
        assert eng.input_hw() == (512, 1024)
        eng.infer_tensor(x)                                   # eager pass
        got = eng.logits()
        assert eng.output_shape() == (1, 8, 1, 10752) and got.size == want.size
        got = got.reshape(want.shape)
        err = _rel(got, want)
        print(f"raw: {err:.2e}")
        assert err <= 1e-3
        assert _rel(got[:, ::int(g["box_step"])], g["raw_0"]) <= 1e-3        # the reference module itself
        names = [n for n, *_ in eng.tensors()]
        for tap, key, t in zip(("fpn.h2.conv2", "fpn.h4.conv2", "fpn.h6.conv2"), ("p3", "p4", "p5"), taps):
            gt = eng.tensor_read(names.index(tap))
            assert gt.shape == t.shape and _rel(gt, t) <= 1e-3, tap
            assert _rel(gt.ravel()[::int(g["tap_step"])], g[key + "_0"]) <= 1e-3, tap
        eng.infer_tensor(x)                                   # graph capture + replay: the same bits
        assert np.array_equal(eng.logits().reshape(want.shape), got)
        with pytest.raises(emu_lib.VpError, match="vp_detect_infer"):
            eng.infer(np.zeros((720, 1280, 3), np.uint8))
    finally:
        eng.close()


def test_refusals_at_creation(emu_lib):
    from autoware_vision_pilot_amd import synthetic, weights as vw

    sd = synthetic.make_autospeed_state_dict(1)
    blob = vw.pack_state_dict(sd)
    with pytest.raises(ValueError, match="VP_WEIGHTS_FP8"):
        emu_lib.Engine("autospeed", blob, precision="fp16", weights_fp8=True)
    with pytest.raises(ValueError):
        emu_lib.Engine("autospeed", blob, precision="fp16", frames=2)
    bad = dict(sd)
    bad["head.dfl.conv.weight"] = sd["head.dfl.conv.weight"] * np.float32(2)
    with pytest.raises(emu_lib.VpError, match="DFL"):
        emu_lib.Engine("autospeed", vw.pack_state_dict(bad), precision="fp16")


def test_plan_is_the_committed_one_and_backbone_launches_are_autodrives(emu_lib):
    """Every launch of the detector engine (name, kernel tag, launch geometry; both precisions, default and latency plan) against
    tests/golden/kernel_plan_autospeed.json; the launches of the shared backbone carry AutoDrive's tags and launch strings, entry by entry."""
    from dump_kernel_plan import autospeed_plan

    want = json.load(open(os.path.join(HERE, "golden", "kernel_plan_autospeed.json")))
    got = autospeed_plan(emu_lib)
    assert sorted(got) == sorted(want)
    for key in want:
        assert [list(r) for r in got[key]] == want[key], key
    for prec in ("fp16x3", "fp16"):
        ad = [r for r in got[f"autodrive/{prec}"] if r[0].startswith("backbone.")]
        sp = [r for r in got[f"autospeed/{prec}"] if r[0].startswith("net.")]
        assert len(ad) == len(sp) == 38
        assert [[r[0][len("backbone."):], r[1], r[2]] for r in ad] == [[r[0][len("net."):], r[1], r[2]] for r in sp]
        n = [r[0] for r in got[f"autospeed/{prec}"]]
        assert n[0] == "net.p1" and n[-2:] == ["head.decode", "finite_probe"] and "preprocess" not in n


def test_detect_head_decode_kernel_against_fp64(emu_lib):
    """detect_head_decode_kernel alone: random logits, rows with one dominant bin, all-equal bins -- against torch fp64 at 1e-5 * max(1, |ref|).
    Inputs are rounded through the (hi, lo) pair first, so the comparison sees the kernel's arithmetic only."""
    import torch

    import autospeed_net_ref as ref

    rng = np.random.default_rng(3)
    h0, w0, nc = 8, 16, 4
    total = sum((h0 >> l) * (w0 >> l) for l in range(3))
    box = rng.normal(0, 3, size=(64, total)).astype(np.float32)
    box[:16, 1] = 0.0
    box[5, 1] = 40.0                                          # one dominant bin: the expectation is (almost) the bin index
    box[16:32, 2] = 1.25                                      # all-equal bins (the top side of anchor 2): 7.5
    box[32:48, 3] = -60000.0
    box[48:, 4] = np.linspace(-30, 30, 16)
    cls = rng.normal(0, 4, size=(nc, total)).astype(np.float32)
    cls[0, 0], cls[1, 0] = 30.0, -30.0
    hi = box.astype(np.float16).astype(np.float32)
    box = hi + (box - hi).astype(np.float16).astype(np.float32)
    hi = cls.astype(np.float16).astype(np.float32)
    cls = hi + (cls - hi).astype(np.float16).astype(np.float32)
    got = emu_lib.op_detect_head_decode(box, cls, h0, w0, precision="fp16x3")
    levels, off = [], 0
    for l in range(3):
        h, w = h0 >> l, w0 >> l
        lv = np.concatenate([box[:, off:off + h * w], cls[:, off:off + h * w]]).reshape(1, 64 + nc, h, w)
        levels.append(torch.from_numpy(lv).double())
        off += h * w
    sd = {"head.dfl.conv.weight": torch.arange(16, dtype=torch.float64).view(1, 16, 1, 1)}
    want = ref.decode(sd, levels)[0].numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    assert float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()) <= 1e-5
    # the distances themselves, recovered from the box rows (level 0: stride 8, anchor i of row 0 at (i + 0.5, 0.5)); channels 0..15 are the left
    # side's bins, 16..31 the top side's (auto_speed_head.py:61-64: a = anchor - (left, top), b = anchor + (right, bottom))
    left_1 = (1.5 - got[0, 1] / 8.0) + got[2, 1] / 16.0         # one dominant bin (logit 40 against 0): the bin index, 5
    top_2 = (0.5 - got[1, 2] / 8.0) + got[3, 2] / 16.0          # all-equal bins: sum(j / 16) = 7.5
    print(f"dominant bin: left {left_1!r}; all-equal bins: top {top_2!r}")
    assert abs(left_1 - 5.0) <= 1e-5 and abs(top_2 - 7.5) <= 1e-5


def _planes(x):
    hi = x.astype(np.float16)
    return hi, (x - hi.astype(np.float32)).astype(np.float16)


@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
def test_upsample2_cat_kernel_bit_exact(emu_lib, precision):
    rng = np.random.default_rng(4)
    a = rng.normal(0, 2, size=(64, 5, 7)).astype(np.float32)
    b = rng.normal(0, 2, size=(40, 10, 14)).astype(np.float32)
    hi, lo = emu_lib.op_upsample2_cat(a, b, precision=precision)
    want = np.concatenate([a.repeat(2, axis=1).repeat(2, axis=2), b])
    wh, wl = _planes(want)
    assert np.array_equal(hi.view(np.uint16), wh.view(np.uint16))
    assert np.array_equal(lo.view(np.uint16), wl.view(np.uint16) if precision == "fp16x3" else np.zeros_like(wl.view(np.uint16)))


@pytest.mark.parametrize("act,with_add", [(2, False), (0, True), (2, True), (0, False)])
def test_dwconv_activated_kernel_bit_exact(emu_lib, act, with_add):
    """dwconv_plain_kernel with its optional activation and optional add against numpy in the kernel's own order: fp32 fma over the taps in
    (ky, kx) order starting from the bias, SiLU as x / (1 + expf(-x)), then the add, then the (hi, lo) split -- on (hi, lo) inputs, both planes
    bit for bit in every case.  The emulation's expf is the C library's, so the reference calls that same function (numpy's exp may differ from it
    in the last bit); the fp32 negation, addition and division around it are correctly rounded in numpy as in C."""
    rng = np.random.default_rng(5)
    c, h, w = 80, 6, 9
    x = rng.normal(0, 1.5, size=(c, h, w)).astype(np.float32)
    xh, xl = _planes(x)
    x = xh.astype(np.float32) + xl.astype(np.float32)
    wt = rng.normal(0, 0.4, size=(c, 3, 3)).astype(np.float32)
    bias = rng.normal(0, 0.2, size=c).astype(np.float32)
    add = None
    if with_add:
        add = rng.normal(0, 1, size=(c, h, w)).astype(np.float32)
        ah, al = _planes(add)
        add = ah.astype(np.float32) + al.astype(np.float32)
    hi, lo = emu_lib.op_dwconv3x3(x, wt, bias, act=act, add=add, precision="fp16x3")
    acc = np.broadcast_to(bias[:, None, None], (c, h, w)).astype(np.float64)          # fp32 fma == fp64 product + sum rounded once to fp32
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    inside = np.pad(np.ones((h, w), bool), 1)
    for ky in range(3):
        for kx in range(3):
            tap = xp[:, ky:ky + h, kx:kx + w].astype(np.float64) * wt[:, ky, kx].astype(np.float64)[:, None, None]
            nxt = (acc + tap).astype(np.float32).astype(np.float64)
            acc = np.where(inside[ky:ky + h, kx:kx + w][None], nxt, acc)            # taps outside the map are skipped, not added as zeros
    v = acc.astype(np.float32)
    if act == 2:
        libm = ct.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        libm.expf.restype, libm.expf.argtypes = ct.c_float, [ct.c_float]
        e = np.array([libm.expf(float(t)) for t in (-v).ravel()], np.float32).reshape(v.shape)
        v = (v / (np.float32(1) + e)).astype(np.float32)
    if with_add:
        v = (v + add).astype(np.float32)
    wh, wl = _planes(v)
    assert np.array_equal(hi.view(np.uint16), wh.view(np.uint16)) and np.array_equal(lo.view(np.uint16), wl.view(np.uint16))
