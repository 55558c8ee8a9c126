"""VP_ACT_SCALE without a GPU: the C ABI and the Python constants, the golden file of the range case against its generator, and the mechanism itself on the
CPU-emulated engine (tests/emul: the real kernel and engine sources on the HIP-on-CPU shim) -- the GPU twins are tests/test_gpu_act_scale.py tests 1, 3, 6, 7."""
import ctypes as ct
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
sys.path.insert(0, HERE)
import abi  # noqa: E402
GOLDEN = os.path.join(HERE, "golden", "autodrive_range.npz")
NEW_SYMBOLS = ("vp_calibrate_range", "vp_reset_range", "vp_act_scales", "vp_set_act_scales", "vp_op_absmax", "vp_op_conv2d_scaled")


def test_abi_exports_the_act_scale_symbols():
    from autoware_vision_pilot_amd import lib

    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in lib.EXPORTED_SYMBOLS and s in exported, s


def test_python_constants_match_the_header():
    from autoware_vision_pilot_amd import lib

    header = open(abi.HEADER).read()
    for name in ("VP_ACT_SCALE", "VP_WEIGHTS_FP8", "VP_PLAN_LATENCY"):
        m = re.search(r"\b%s = (\d+)" % name, header)
        assert m and int(m.group(1)) == getattr(lib, name), name
    assert lib.VP_ACT_SCALE == 64


def test_golden_regenerates_byte_identical(tmp_path):
    ref = os.environ.get("VP_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "Models", "model_components", "autodrive")):
        pytest.skip("the reference checkout is not on this machine")
    out = tmp_path / "autodrive_range.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pin_act_scale.py"), "--out", str(out)], check=True, capture_output=True)
    assert out.read_bytes() == open(GOLDEN, "rb").read()


# ------------------------------------------------------------------------------------------------ the emulated engine
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


def _split(v):
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(np.float32)).astype(np.float16)


def test_absmax_kernel_on_cpu(emu_lib):
    rng = np.random.default_rng(3)
    v = rng.standard_normal((5, 7, 64)).astype(np.float32) * 100
    hi, lo = _split(v)
    hi[..., 40:] = np.float16(60000.0)      # padding: must not count
    hi[1, 2, 3] = np.float16(-65504.0)
    lo[1, 2, 3] = 0
    hi[0, 0, 0] = np.float16(np.inf)
    hi[4, 6, 39] = np.float16(np.nan)
    val = hi[..., :40].astype(np.float32) + lo[..., :40].astype(np.float32)
    fin = np.isfinite(val)
    got = emu_lib.op_absmax(hi, lo, 40)
    assert got == (np.float32(np.abs(val[fin]).max()), int((~fin).sum())) and got == emu_lib.op_absmax(hi, lo, 40)
    assert emu_lib.op_absmax(np.zeros((1, 1, 64), np.float16), None, 64) == (np.float32(0), 0)


def test_conv2d_scaled_on_cpu(emu_lib):
    """3x3 + SiLU + the CTX gate (RES_MULADD) with an input that does not fit fp16 unscaled; zero exponents give op_conv2d's planes."""
    import torch

    rng = np.random.default_rng(5)
    cin, cout, h, w = 32, 32, 8, 16
    x = (rng.standard_normal((cin, h, w)) * 3e5).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin) * 1e-3).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    res = rng.uniform(0.01, 0.12, (cout, h, w)).astype(np.float32)
    y = torch.nn.functional.silu(torch.nn.functional.conv2d(torch.from_numpy(x).double()[None], torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=1))[0]
    r = torch.from_numpy(res).double()
    ref = (y * r + r).numpy()
    out_exp = int(np.ceil(np.log2(np.abs(ref).max()))) - 12
    hi, lo = emu_lib.op_conv2d_scaled(x, wt, b, ks=3, act=2, res=res, res_mode=2, in_exp=6, res_exp=-3, out_exp=out_exp)
    got = (hi.astype(np.float32) + lo.astype(np.float32)).astype(np.float64) * 2.0 ** out_exp
    assert np.abs(hi.astype(np.float32)).max() < 2.0 ** 12 + 1
    assert (np.abs(got - ref) <= 2e-5 * np.maximum(1.0, np.abs(ref))).all(), float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
    xs = (x / 3e5).astype(np.float32)
    h0, l0 = emu_lib.op_conv2d_scaled(xs, wt, b, ks=3, act=2, res=res, res_mode=2)
    plain = emu_lib.op_conv2d(xs, wt, b, ks=3, act=2, res=res, res_mode=2, precision=emu_lib.VP_FP16X3)
    # op_conv2d hands back fp32(hi) + fp32(lo) of the planes it stored (exact: 22 bits): equal sums <=> equal planes up to the one ambiguity a re-split
    # of the sum has (a lo of exactly half an ulp of hi), so the sums are what is compared, bit for bit
    assert np.array_equal((h0.astype(np.float32) + l0.astype(np.float32)).view(np.uint32), plain.view(np.uint32))


def test_autodrive_act_scale_on_cpu(emu_lib):
    """Tests 3, 6 and 7 of tests/test_gpu_act_scale.py on the emulated engine: zero exponents = the unflagged engine's bits; calibration puts every tie
    group's stored abs-max into the band, leaves the outputs at the parity bar and is reproduced by a shipped table; reset returns the first bits."""
    from autoware_vision_pilot_amd import synthetic, weights as vw
    from test_gpu_act_scale import _check_band      # the band rule and the tie groups: one statement for both suites

    g = np.load(os.path.join(HERE, "golden", "autodrive.npz"))
    frames = [synthetic.synthetic_frame(1080, 1920, int(s)) for s in g["frame_seeds"]]
    blob = vw.pack_state_dict(synthetic.make_autodrive_state_dict(int(g["weight_seed"])))
    plain = emu_lib.Engine("autodrive", blob, precision="fp16x3")
    a = emu_lib.Engine("autodrive", blob, precision="fp16x3", act_scale=True)
    b = emu_lib.Engine("autodrive", blob, precision="fp16x3", act_scale=True)
    try:
        plain.infer_pair(frames[0], frames[1])
        want = plain.logits().reshape(3).copy()
        a.infer_pair(frames[0], frames[1])
        assert np.array_equal(a.logits().reshape(3).view(np.uint32), want.view(np.uint32))
        assert a.plan_hash() == plain.plan_hash() and not a.act_scales().any()
        a.infer_pair(frames[1], frames[1])
        a.calibrate_range()
        assert a.plan_hash() == plain.plan_hash()
        exps = a.act_scales()
        assert (exps != 0).any() and (exps < 0).any(), exps
        a.infer_pair(frames[1], frames[1])
        names = [t[0] for t in a.tensors()]
        stored = np.array([float(np.abs(a.tensor_read(i)).max()) * 2.0 ** -int(exps[i]) for i in range(len(names))])
        _check_band(names, exps, stored)
        a.infer_pair(frames[0], frames[1])
        got = a.logits().reshape(3).copy()
        assert np.abs(got - g["fp32_out"]).max() <= 1e-3, (got, g["fp32_out"])
        b.set_act_scales(exps)
        b.infer_pair(frames[0], frames[1])
        assert np.array_equal(b.logits().reshape(3).view(np.uint32), got.view(np.uint32))
        with pytest.raises(ValueError):
            b.set_act_scales(exps[:-1])
        bad = exps.copy()
        i_cat, i_cv2 = names.index("head.cat"), names.index("backbone.p5.3.cv2")
        bad[i_cv2] = bad[i_cat] + 1
        with pytest.raises(ValueError, match="tied"):
            b.set_act_scales(bad)
        a.reset_range()
        a.infer_pair(frames[0], frames[1])
        assert np.array_equal(a.logits().reshape(3).view(np.uint32), want.view(np.uint32))
    finally:
        plain.close()
        a.close()
        b.close()

