"""VP_MFMA_FP8 on the GPU (include/vp_hip.h "FP8 MFMA ENGINES"): the kernel's quantiser against the host entry, the operator against the numpy restatement
of tests/f8_cases.py -- with exact asymmetric integers first, which is what checks the e4m3 MFMA's operand pairing on the hardware -- and flagged SceneSeg
/ Scene3D engines: untouched ahead of the first fp8 launch, the engine's layer equal to the operator bit for bit, calibration, reset, a shipped table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f8_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu

RULE_LAYERS = ("decode_layer_5",)     # the dispatch rule as measured: 3x3, plain, >= 80 x 160 pixels, >= 512 input channels


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_device_quantiser_equals_the_host_entry():
    from autoware_vision_pilot_amd import lib

    every = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    for qexp in fc.EXPS:
        got, want = lib.fp8_quantize(every, qexp), lib.fp8_quantize_act(every, qexp)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (qexp, [(hex(i), int(got[i]), int(want[i])) for i in bad[:8]])


@pytest.mark.parametrize("shape", fc.SHAPES_GPU)
def test_operator_exact_integers_bit_for_bit(shape):
    from autoware_vision_pilot_amd import lib

    fc.check_exact(lib.conv3x3_f8, shape)


@pytest.mark.parametrize("shape", fc.SHAPES_GPU[:4])
def test_operator_random_operands(shape):
    from autoware_vision_pilot_amd import lib

    for qexp in (-2, 0, 3):
        for act in (0, 1):
            fc.check_random(lib.conv3x3_f8, shape, qexp, act)


def test_operator_refusals():
    from autoware_vision_pilot_amd import lib

    fc.check_refusals(lib.conv3x3_f8)


@pytest.fixture(scope="module")
def sceneseg_pair(state_dicts, engines):
    from autoware_vision_pilot_amd import lib, weights as vw

    f8 = lib.Engine("sceneseg", vw.pack_state_dict(state_dicts("sceneseg")), precision="fp16", mfma_fp8=True)
    yield engines("sceneseg", "fp16"), f8
    f8.close()


def _layer_against_operator(lib, eng, sd, entry):
    """the 80 x 160 layer, 512 -> 256: its stored input through vp_op_conv3x3_f8 under its qexp == its stored output"""
    launch, t_in, qexp = entry
    name = eng.layers()[launch][0]
    tensors = eng.tensors()
    assert tensors[t_in][1:] == (512, 80, 160) and name.endswith("decode_layer_5")
    t_out = [i for i, t in enumerate(tensors) if t[0] == name]
    assert len(t_out) == 1 and tensors[t_out[0]][1:] == (256, 80, 160)
    x = eng.tensor_read(t_in)
    got = lib.conv3x3_f8(x, sd[name + ".weight"], sd[name + ".bias"], act=1, qexp=qexp)      # the scene decoders' convolutions carry no BatchNorm
    want = eng.tensor_read(t_out[0]).astype(np.float16)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), int((got != want).sum())


def test_sceneseg_engine(sceneseg_pair, state_dicts, frame720):
    from autoware_vision_pilot_amd import lib

    plain, f8 = sceneseg_pair
    sd = state_dicts("sceneseg")
    plain.infer(frame720)
    f8.infer(frame720)
    first = f8.logits().copy()
    layers = f8.fp8_layers()
    kernels = f8.layer_kernels()
    assert [i for i, k in enumerate(kernels) if k == "conv3x3_f8"] == [l[0] for l in layers] and len(layers) == len(RULE_LAYERS)
    assert sorted(f8.layers()[l[0]][0].split(".")[-1] for l in layers) == sorted(RULE_LAYERS)
    moved = {l[0] for l in layers}
    rows_plain = list(zip((a[0] for a in plain.layers()), plain.layer_kernels(), plain.layer_launches()))
    rows_f8 = list(zip((a[0] for a in f8.layers()), kernels, f8.layer_launches()))
    assert len(rows_plain) == len(rows_f8) and all(a == b for i, (a, b) in enumerate(zip(rows_plain, rows_f8)) if i not in moved)
    # every tensor stored before the first conv3x3_f8 launch: the unflagged engine's bits
    tensors = f8.tensors()
    assert tensors == plain.tensors()
    first_out = [i for i, t in enumerate(tensors) if t[0] == f8.layers()[layers[0][0]][0]][0]
    stored = {i for i, r in enumerate(f8.range_survey()) if r["count"] > 0}
    checked = 0
    for i in range(first_out):
        if i in stored:
            assert np.array_equal(_bits(f8.tensor_read(i)), _bits(plain.tensor_read(i))), tensors[i]
            checked += 1
    assert checked >= 10
    # engine against operator, before calibration
    assert all(l[2] == 0 for l in layers)
    _layer_against_operator(lib, f8, sd, layers[0])
    # calibration: absmax * 2^-qexp of every layer's input in [128, 256)
    f8.calibrate_fp8(0)
    cal = f8.fp8_layers()
    survey = f8.range_survey()
    for launch, t, q in cal:
        amax = float(survey[t]["absmax"])
        print(f"{f8.layers()[launch][0]}: input absmax {amax:.4g}, qexp {q}")
        assert (amax == 0.0 and q == 0) or 128.0 <= amax * 2.0 ** -q < 256.0, (launch, t, q, amax)
    f8.calibrate_fp8(0)
    assert f8.fp8_layers() == cal                                                  # a second call changes nothing
    f8.infer(frame720)
    calibrated = f8.logits().copy()
    f8.infer(frame720)
    assert np.array_equal(_bits(f8.logits()), _bits(calibrated))                   # infer; calibrate; infer; infer
    _layer_against_operator(lib, f8, sd, cal[0])                                   # engine against operator, after calibration
    f8.reset_fp8()
    assert [l[2] for l in f8.fp8_layers()] == [0] * len(RULE_LAYERS)
    f8.infer(frame720)
    assert np.array_equal(_bits(f8.logits()), _bits(first))
    f8.set_fp8_exps([l[2] for l in cal])                                           # the shipped table
    f8.infer(frame720)
    assert np.array_equal(_bits(f8.logits()), _bits(calibrated))
    assert np.isfinite(calibrated).all()


def test_scene3d_engine(state_dicts, frame720):
    from autoware_vision_pilot_amd import lib, weights as vw

    eng = lib.Engine("scene3d", vw.pack_state_dict(state_dicts("scene3d")), precision="fp16", mfma_fp8=True)
    try:
        eng.infer(frame720)
        assert np.isfinite(eng.logits()).all()
        tagged = [n.split(".")[-1] for (n, _, _), k in zip(eng.layers(), eng.layer_kernels()) if k == "conv3x3_f8"]
        assert sorted(tagged) == sorted(RULE_LAYERS)
        eng.calibrate_fp8(0)
        eng.infer(frame720)
        assert np.isfinite(eng.logits()).all()
    finally:
        eng.close()
