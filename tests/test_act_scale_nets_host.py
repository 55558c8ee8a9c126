"""VP_ACT_SCALE for the AutoSpeed and AutoSteer engines without a GPU: the C ABI, creation and refusals, the fixture against its generator, and -- on the
CPU-emulated engine (tests/emul: the real kernel and engine sources on the HIP-on-CPU shim) -- the four hand-written kernels with exponents, the tie
groups of both plans, and the lane network end to end.  The GPU twin is tests/test_gpu_act_scale_nets.py; the cases are tests/act_scale_nets_cases.py."""
import ctypes as ct
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
sys.path.insert(0, HERE)
import abi  # noqa: E402
import act_scale_nets_cases as cases  # noqa: E402

NEW_SYMBOLS = ("vp_op_upsample2_cat_scaled", "vp_op_detect_head_decode_scaled", "vp_op_rowpair_conv_scaled", "vp_op_lane_rows_head_scaled")


def test_abi_exports_the_new_operator_entries():
    from autoware_vision_pilot_amd import lib

    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in lib.EXPORTED_SYMBOLS and s in exported, s


def test_fixture_reproduces_from_the_pin_tools_restatement():
    """every array of tests/golden/act_scale_nets.npz from tools/pin_act_scale_nets.py's own computation (the restatements; no reference checkout needed),
    and the conditions the recipe sets"""
    import pin_act_scale_nets as pin

    fix = np.load(cases.GOLDEN)
    got = pin.compute(log=lambda *a: None)
    assert sorted(got) == sorted(fix.files)
    for k in fix.files:
        a, b = np.asarray(got[k]), fix[k]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
    for net in ("autospeed", "autosteer"):
        assert float(fix[f"{net}_first_beyond_absmax"]) > 65504.0 and set(pin.HEAD_INPUTS[net]) <= {str(n) for n in fix[f"{net}_compared"]}
        for n in fix[f"{net}_compared"]:
            assert float(fix[f"{net}_dist_{n}"]) < 4e-4 and np.isfinite(fix[f"{net}_range_{n}"]).all()
        sd = pin.ill_scaled(pin.state_dict(net), str(fix[f"{net}_block"]), int(fix[f"{net}_k"]))
        assert pin.folded_weight_absmax(sd) <= 65504.0


def test_fixture_regenerates_byte_identical(tmp_path):
    """--no-reference: the tool run must not depend on anything outside the repository (the bytes are the same with the reference checked as well)"""
    out = tmp_path / "act_scale_nets.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pin_act_scale_nets.py"), "--out", str(out), "--no-reference"], check=True, capture_output=True)
    assert out.read_bytes() == open(cases.GOLDEN, "rb").read()


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


@pytest.mark.parametrize("exp", cases.EXPS)
@pytest.mark.parametrize("nch", [8, 16])
def test_upsample2_cat_on_cpu(emu_lib, nch, exp):
    cases.check_upsample2_cat(emu_lib, nch, exp)


@pytest.mark.parametrize("in_exp,out_exp", [(0, 0), (6, -3), (-3, 6), (6, 0), (0, -3)])
@pytest.mark.parametrize("replicate", [False, True])
@pytest.mark.parametrize("cin", [8, 64])
def test_rowpair_conv_on_cpu(emu_lib, cin, replicate, in_exp, out_exp):
    cases.check_rowpair(emu_lib, cin, replicate, in_exp, out_exp)


@pytest.mark.parametrize("in_exp", cases.EXPS)
@pytest.mark.parametrize("cin", [8, 64])
def test_lane_rows_head_on_cpu(emu_lib, cin, in_exp):
    cases.check_lane_rows(emu_lib, cin, in_exp)


@pytest.mark.parametrize("exps", [(0,) * 6, (6, -3, -3, 6, 6, 6), (-3, 0, 6, -3, 0, 6)])
@pytest.mark.parametrize("nc", [1, 4])
def test_detect_head_decode_on_cpu(emu_lib, nc, exps):
    cases.check_detect(emu_lib, nc, exps)


@pytest.fixture(scope="module")
def blobs():
    from autoware_vision_pilot_amd import synthetic, weights as vw

    return {"autospeed": vw.pack_state_dict(synthetic.make_autospeed_state_dict(5)), "autosteer": vw.pack_state_dict(synthetic.make_autosteer_state_dict(5)),
            "sceneseg": None}


@pytest.mark.parametrize("net", ["autospeed", "autosteer"])
def test_creation_refusals_and_tie_groups_on_cpu(emu_lib, blobs, net):
    """VP_FP16X3 | VP_ACT_SCALE [| VP_PLAN_LATENCY] creates with the unflagged plan; VP_FP16, VP_WEIGHTS_FP8, shared and batched creation stay refused with
    their texts; vp_set_act_scales refuses a table that splits a tie group."""
    lib = emu_lib
    plain = lib.Engine(net, blobs[net], precision="fp16x3")
    for latency in (False, True):
        eng = lib.Engine(net, blobs[net], precision="fp16x3", act_scale=True, plan_latency=latency)
        if not latency:
            assert eng.plan_hash() == plain.plan_hash() and not eng.act_scales().any() and len(eng.act_scales()) == len(eng.tensors())
            cases.check_tie_groups(eng, net)
        eng.close()
    with pytest.raises(ValueError, match="VP_ACT_SCALE needs VP_FP16X3"):
        lib.Engine(net, blobs[net], precision="fp16", act_scale=True)
    with pytest.raises(ValueError, match="VP_WEIGHTS_FP8"):
        lib.Engine(net, blobs[net], precision="fp16x3", act_scale=True, weights_fp8=True)
    with pytest.raises(ValueError, match="shared-prefix and batched creation are not supported"):
        lib.Engine(net, blobs[net], precision="fp16x3", act_scale=True, base=plain)
    with pytest.raises(ValueError, match="shared-prefix and batched creation are not supported"):
        lib.Engine(net, blobs[net], precision="fp16x3", act_scale=True, frames=2)
    with pytest.raises(ValueError, match="VP_ACT_SCALE only"):
        plain.calibrate_range()
    plain.close()


def test_scene_kinds_stay_refused_and_the_text_names_what_is_supported(emu_lib):
    from autoware_vision_pilot_amd import weights as vw
    from oracle import weights

    blob = vw.pack_state_dict(weights.make_state_dict("sceneseg", 0))
    with pytest.raises(ValueError, match="VP_AUTODRIVE, VP_AUTOSPEED and VP_AUTOSTEER"):
        emu_lib.Engine("sceneseg", blob, precision="fp16x3", act_scale=True)


def test_autosteer_act_scale_end_to_end_on_cpu(emu_lib):
    """the lane network on the emulated engine: zero exponents = the unflagged bits, calibration on the resident frame, the band, the bar, the shipped
    table, reset (the GPU suite runs the same check, the detector and the range case of both networks)"""
    cases.check_ordinary_band_and_table(cases.Net(emu_lib, "autosteer"))
