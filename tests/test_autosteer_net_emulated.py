"""The AutoSteer 2.0 lane-perception network (VP_AUTOSTEER) on the CPU: the real engine and kernels on the HIP-on-CPU emulation (tests/emul) against
tests/autosteer_net_ref.py, the restatement pinned to the reference's own module (tests/golden/autosteer_net.npz); the two new kernels alone; the
preprocess to the bit; the plan against tests/golden/kernel_plan_autosteer.json; the backbone launches against AutoDrive's; the refusals."""
import ctypes as ct
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
GOLDEN = os.path.join(HERE, "golden", "autosteer_net.npz")


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


@pytest.fixture(scope="module")
def blob5():
    from autoware_vision_pilot_amd import synthetic, weights as vw

    sd = synthetic.make_autosteer_state_dict(int(np.load(GOLDEN)["weight_seed"]))
    return sd, vw.pack_state_dict(sd)


def _rel(got, ref):
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def test_autosteer_engine_end_to_end_on_cpu(emu_lib, blob5):
    """kind 6, fp16x3, fixture frame 0 through the frame entry: xp, h_vector and the fpn.h1 / fpn.h2 / features tensors within 1e-3 * max(1, |ref|) of the
    restatement and of the reference module's own vectors; a second pass (graph capture + replay) gives the same bits."""
    import autosteer_net_ref as ref
    from autoware_vision_pilot_amd import synthetic

    g = np.load(GOLDEN)
    sd, blob = blob5
    frame = synthetic.synthetic_frame(ref.NET_H, ref.NET_W, int(g["frame_seeds"][0]))
    (xp, h), taps = ref.forward(sd, ref.preprocess(frame))
    eng = emu_lib.Engine("autosteer", blob, precision="fp16x3")
    try:
        assert eng.input_hw() == (512, 1024)
        eng.infer(frame)                                      # eager pass
        assert eng.output_shape() == (1, 2, 64, 1)
        got = eng.logits().reshape(2, 64)
        ex, eh = _rel(got[0], xp), _rel(got[1], h)
        print(f"xp: {ex:.2e}  h_vector: {eh:.2e}")
        assert ex <= 1e-3 and eh <= 1e-3
        assert _rel(got[0], g["xp_0"]) <= 1e-3 and _rel(got[1], g["h_0"]) <= 1e-3        # the reference module itself
        assert np.array_equal(got[1] >= 0.5, g["h_0"] >= 0.5)
        names = [n for n, *_ in eng.tensors()]
        for tap in ("fpn.h1.conv2", "fpn.h2.conv2", "features"):
            gt = eng.tensor_read(names.index(tap))
            assert gt.shape == taps[tap].shape, tap
            err = _rel(gt, taps[tap])
            print(f"{tap}: {err:.2e}")
            assert err <= 1e-3, tap
            assert _rel(gt.ravel()[::int(g["tap_step"])], g[f"{tap}_0"]) <= 1e-3, tap
        eng.infer(frame)                                      # graph capture + replay: the same bits
        assert np.array_equal(eng.logits().reshape(2, 64).view(np.uint32), got.view(np.uint32))
        with pytest.raises(ValueError, match="512 x 1024"):
            eng.infer(np.zeros((720, 1280, 3), np.uint8))
    finally:
        eng.close()


def test_lane_rows_head_kernel_against_fp64(emu_lib):
    import autosteer_cases

    autosteer_cases.check_lane_rows(emu_lib)


@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
@pytest.mark.parametrize("h,w", [(4, 5), (6, 16)])
@pytest.mark.parametrize("replicate", [False, True])
def test_rowpair_conv_kernel_against_fp64(emu_lib, precision, h, w, replicate):
    import autosteer_cases

    autosteer_cases.check_rowpair(emu_lib, precision, h, w, replicate)


@pytest.mark.parametrize("fmt", ["bgr", "rgb"])
def test_preprocess_is_u8_over_255_to_the_bit(emu_lib, blob5, fmt):
    """A 512 x 1024 frame holding all 256 byte values in every channel (each channel a different arrangement): vp_input_tensor after vp_infer equals
    numpy's float32(u8) / float32(255) bit for bit, as R, G, B planes, for BGR and for RGB input bytes."""
    rng = np.random.default_rng(7)
    frame = np.stack([rng.permutation(np.arange(512 * 1024, dtype=np.int64) % 256).astype(np.uint8).reshape(512, 1024) for _ in range(3)], axis=-1)
    assert all(len(np.unique(frame[..., c])) == 256 for c in range(3))
    eng = emu_lib.Engine("autosteer", blob5[1], precision="fp16")
    try:
        eng.set_input_format(emu_lib.VP_BGR8 if fmt == "bgr" else emu_lib.VP_RGB8, emu_lib.VP_PLANES_RGB)
        eng.infer(frame)
        got = eng.input_tensor().reshape(3, 512, 1024)
    finally:
        eng.close()
    rgb = frame[:, :, ::-1] if fmt == "bgr" else frame
    want = rgb.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_plan_is_the_committed_one_and_backbone_launches_are_autodrives(emu_lib):
    """Every launch of the engine (name, kernel tag, launch geometry; both precisions, default and latency plan) against
    tests/golden/kernel_plan_autosteer.json; the 38 launches of the shared backbone carry AutoDrive's tags and launch strings, entry by entry."""
    from dump_kernel_plan import autosteer_plan

    want = json.load(open(os.path.join(HERE, "golden", "kernel_plan_autosteer.json")))
    got = autosteer_plan(emu_lib)
    assert sorted(got) == sorted(want) and len(want) == 4
    for key in want:
        assert [list(r) for r in got[key]] == want[key], key
    ad_plan = json.load(open(os.path.join(HERE, "golden", "kernel_plan_autospeed.json")))
    for prec in ("fp16x3", "fp16"):
        ad = [r for r in ad_plan[f"autodrive/{prec}"] if r[0].startswith("backbone.")]
        st = [r for r in got[f"autosteer/{prec}"] if r[0].startswith("net.")]
        assert len(ad) == len(st) == 38
        assert [[r[0][len("backbone."):], r[1], r[2]] for r in ad] == [[r[0][len("net."):], r[1], r[2]] for r in st]
        n = [r[0] for r in got[f"autosteer/{prec}"]]
        assert n[:2] == ["preprocess", "net.p1"] and n[-4:] == ["head.v2", "head.v1", "head.lanes+height", "finite_probe"]
        assert [r[1] for r in got[f"autosteer/{prec}"][-4:-1]] == ["rowpair_conv<up2>", "rowpair_conv", "lane_rows_head"]


def test_refusals(emu_lib, blob5):
    from autoware_vision_pilot_amd import weights as vw

    sd, blob = blob5
    with pytest.raises(ValueError, match="VP_WEIGHTS_FP8"):
        emu_lib.Engine("autosteer", blob, precision="fp16", weights_fp8=True)
    with pytest.raises(ValueError):
        emu_lib.Engine("autosteer", blob, precision="fp16", frames=2)
    base = emu_lib.Engine("autosteer", blob, precision="fp16")
    try:
        with pytest.raises(ValueError, match="VP_AUTOSTEER"):
            emu_lib.Engine("autosteer", blob, precision="fp16", base=base)
        with pytest.raises(ValueError, match="512 x 1024"):
            base.infer(np.zeros((720, 1280, 3), np.uint8))
    finally:
        base.close()
    bad = dict(sd)
    bad["head.v1.weight"] = np.ascontiguousarray(sd["head.v1.weight"][:16])
    bad["head.v1.bias"] = np.ascontiguousarray(sd["head.v1.bias"][:16])
    with pytest.raises(emu_lib.VpError, match="head.v1.weight"):
        emu_lib.Engine("autosteer", vw.pack_state_dict(bad), precision="fp16")
