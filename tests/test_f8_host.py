"""VP_MFMA_FP8 without a GPU: the C ABI and the Python constant, the host quantiser against the numpy restatement over every fp16 bit pattern, the
dispatch rule through the plans of the CPU-emulated engine (tests/emul), and every refusal of the flag and of the four exponent entries."""
import ctypes as ct
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emul"))
sys.path.insert(0, HERE)
import abi  # noqa: E402
import f8_cases as fc  # noqa: E402

NEW_SYMBOLS = ("vp_calibrate_fp8", "vp_reset_fp8", "vp_fp8_layers", "vp_set_fp8_exps", "vp_fp8_quantize_act", "vp_op_conv3x3_f8", "vp_op_fp8_quantize")
RULE_LAYERS = ("decode_layer_5",)     # 3x3, plain, >= 80 x 160 pixels, >= 512 input channels (decode_layer_7 / 9 fit the kernel but measured slower: DESIGN.md)


def test_abi_and_constant():
    from autoware_vision_pilot_amd import lib

    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in exported and s in lib._SIGS, s
    m = re.search(r"\bVP_MFMA_FP8 = (\d+)", open(abi.HEADER).read())
    assert m and int(m.group(1)) == lib.VP_MFMA_FP8 == 128


@pytest.mark.parametrize("qexp", fc.EXPS)
def test_host_quantiser_on_every_fp16_pattern(qexp):
    """ties, subnormals of both formats, +-448, the first value that saturates, the infinities and every NaN: bit for bit"""
    from autoware_vision_pilot_amd import lib

    every = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    got, want = lib.fp8_quantize_act(every, qexp), fc.quantize_act(every, qexp)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(i), int(got[i]), int(want[i])) for i in bad[:8]]
    sat = np.float16(448.0 * 2.0 ** qexp) if qexp < 8 else np.float16(np.inf)
    assert lib.fp8_quantize_act(np.array([sat, -sat, np.inf, -np.inf], np.float16), qexp).tolist() == [0x7e, 0xfe, 0x7e, 0xfe]
    assert lib.fp8_quantize_act(np.array([np.nan], np.float16), qexp)[0] & 0x7f == 0x7f


def test_host_quantiser_refuses_exponents_beyond_24():
    from autoware_vision_pilot_amd import lib

    for q in (-25, 25):
        with pytest.raises(ValueError):
            lib.fp8_quantize_act(np.zeros(4, np.float16), q)


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


def _blob(kind, seed):
    from autoware_vision_pilot_amd import weights as vw
    from oracle import weights

    return vw.pack_state_dict(weights.make_state_dict(kind, seed))


def _rows(eng):
    return [(n, k, l) for (n, _, _), k, l in zip(eng.layers(), eng.layer_kernels(), eng.layer_launches())]


@pytest.mark.parametrize("kind,seed", [("sceneseg", 0), ("scene3d", 1)])
def test_flagged_plan_moves_exactly_the_rules_layers(emu_lib, kind, seed):
    blob = _blob(kind, seed)
    plain = emu_lib.Engine(kind, blob, precision="fp16")
    f8 = emu_lib.Engine(kind, blob, precision="fp16", mfma_fp8=True)
    lat = emu_lib.Engine(kind, blob, precision="fp16", mfma_fp8=True, plan_latency=True)
    try:
        a, b = _rows(plain), _rows(f8)
        assert [r[0] for r in a] == [r[0] for r in b]
        moved = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
        assert sorted(a[i][0].split(".")[-1] for i in moved) == sorted(RULE_LAYERS), [a[i] for i in moved]
        assert all(b[i][1] == "conv3x3_f8" for i in moved) and not any(r[1] == "conv3x3_f8" for r in a)
        assert [i for i, r in enumerate(b) if r[1] == "conv3x3_f8"] == moved
        assert f8.plan_hash() != plain.plan_hash()
        # the entries: launch index, input tensor (the rule's shape conditions hold on it), exponent 0 from creation
        layers = f8.fp8_layers()
        assert [l[0] for l in layers] == moved and all(l[2] == 0 for l in layers)
        tensors = f8.tensors()
        for _, t, _ in layers:
            _, c, h, w = tensors[t]
            assert c % 64 == 0 and c >= 512 and h * w >= 12800, tensors[t]
        assert [r[1] for r in _rows(lat)].count("conv3x3_f8") == len(RULE_LAYERS)     # the flag combines with VP_PLAN_LATENCY
        # the exponent entries on the flagged engine; nothing is resident yet
        for table in ([3], [-24], [24]):
            f8.set_fp8_exps(table)
            assert [l[2] for l in f8.fp8_layers()] == table
        f8.reset_fp8()
        assert [l[2] for l in f8.fp8_layers()] == [0]
        for bad in ([], [0, 0], [25], [-25]):
            with pytest.raises(ValueError, match="vp_set_fp8_exps"):
                f8.set_fp8_exps(bad)
        with pytest.raises(ValueError, match="target_log2"):
            f8.calibrate_fp8(9)
        # refusal 5: all four entries on an engine without the flag
        for call in (lambda: plain.calibrate_fp8(0), plain.reset_fp8, plain.fp8_layers, lambda: plain.set_fp8_exps([0])):
            with pytest.raises(ValueError):
                call()
    finally:
        for e in (plain, f8, lat):
            e.close()


def test_flag_refusals_say_which_condition(emu_lib):
    """refusal 1: VP_FP16X3, VP_WEIGHTS_FP8, VP_ACT_SCALE, the three YOLO-family kinds, shared-prefix and batched creation"""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    blob = _blob("sceneseg", 0)
    for kw, msg in ((dict(precision="fp16x3"), "needs VP_FP16"), (dict(precision="fp16", weights_fp8=True), "VP_WEIGHTS_FP8"),
                    (dict(precision="fp16", act_scale=True), "VP_ACT_SCALE"), (dict(precision="fp16", frames=2), "batched")):
        with pytest.raises(ValueError, match=msg):
            emu_lib.Engine("sceneseg", blob, mfma_fp8=True, **kw)
    for kind in ("autodrive", "autospeed", "autosteer"):
        with pytest.raises(ValueError, match="VP_MFMA_FP8: VP_SCENESEG"):
            emu_lib.Engine(kind, blob, precision="fp16", mfma_fp8=True)      # refused ahead of the weights
    base = emu_lib.Engine("sceneseg", blob, precision="fp16")
    try:
        sd3 = synthetic.share_backbone(_sd("scene3d", 1), "scene3d", _sd("sceneseg", 0), "sceneseg")
        with pytest.raises(ValueError, match="shared-prefix"):
            emu_lib.Engine("scene3d", vw.pack_state_dict(sd3), precision="fp16", base=base, mfma_fp8=True)
    finally:
        base.close()


def _sd(kind, seed):
    from oracle import weights

    return weights.make_state_dict(kind, seed)
