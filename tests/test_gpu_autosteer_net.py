"""The AutoSteer 2.0 lane-perception network as an engine of this library (VP_AUTOSTEER) on the MI355X.  References: tests/autosteer_net_ref.py (torch CPU
fp32 restatement) and tests/golden/autosteer_net.npz, the outputs of the reference's own nn.Module on the same weights and frames."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import autosteer_cases  # noqa: E402
import autosteer_net_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(HERE, "golden", "autosteer_net.npz"))
SEEDS = [int(s) for s in G["frame_seeds"]] + [31, 32]     # the first two are the fixture's (condition) frames


def _rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def _frame(seed):
    from autoware_vision_pilot_amd import synthetic

    return synthetic.synthetic_frame(ref.NET_H, ref.NET_W, seed)


@pytest.fixture(scope="module")
def net():
    from autoware_vision_pilot_amd import synthetic, weights as vw

    sd = synthetic.make_autosteer_state_dict(int(G["weight_seed"]))
    return sd, vw.pack_state_dict(sd)


@pytest.fixture(scope="module")
def wants(net):
    """The restatement's outputs on the four frames: computed once, read-only."""
    out = [ref.forward(net[0], ref.preprocess(_frame(s)))[0] for s in SEEDS]
    for xp, h in out:
        xp.setflags(write=False)
        h.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def x3(net):
    from autoware_vision_pilot_amd import lib

    eng = lib.Engine("autosteer", net[1], precision="fp16x3")
    yield eng
    eng.close()


def test_outputs_against_restatement_and_reference_module(x3, wants):
    assert x3.input_hw() == (512, 1024)
    for fi, seed in enumerate(SEEDS):
        x3.infer(_frame(seed))
        assert x3.output_shape() == (1, 2, 64, 1)
        got = x3.logits().reshape(2, 64)
        xp, h = wants[fi]
        ex, eh = _rel(got[0], xp), _rel(got[1], h)
        print(f"frame seed {seed}: xp {ex:.2e}  h_vector {eh:.2e}")
        assert ex <= 1e-3 and eh <= 1e-3
        if fi < 2:                                             # the reference module's own vectors, and its validity decision on every row
            assert _rel(got[0], G[f"xp_{fi}"]) <= 1e-3 and _rel(got[1], G[f"h_{fi}"]) <= 1e-3
            assert np.array_equal(got[1] >= 0.5, G[f"h_{fi}"] >= 0.5)


def test_replays_and_tensor_entry_give_the_same_bits(x3):
    f = _frame(SEEDS[0])
    x3.infer(f)
    first = x3.logits().view(np.uint32).copy()
    for _ in range(3):
        x3.infer(f)
        assert np.array_equal(x3.logits().view(np.uint32), first)
    planes = x3.input_tensor().copy()
    assert np.array_equal(planes.reshape(3, 512, 1024), ref.preprocess(f))
    x3.infer(_frame(SEEDS[1]))
    x3.infer_tensor(planes)
    assert np.array_equal(x3.logits().view(np.uint32), first)


def test_fp16_engine(net, wants):
    from autoware_vision_pilot_amd import lib

    eng = lib.Engine("autosteer", net[1], precision="fp16")
    try:
        for fi in range(2):
            eng.infer(_frame(SEEDS[fi]))
            got = eng.logits().reshape(2, 64)
            xp, h = wants[fi]
            ex = float(np.abs(got[0] - xp).max())
            eh = float(np.abs(got[1] - h).max() / max(1.0, np.abs(h).max()))
            print(f"fp16, frame seed {SEEDS[fi]}: xp max abs err {ex:.2e}; h_vector max abs err / max(1, max|ref|) {eh:.2e}")
            assert np.isfinite(got).all()
            assert ex <= 3e-2 and eh <= 3e-2
    finally:
        eng.close()


def test_lane_rows_head_kernel_against_fp64():
    from autoware_vision_pilot_amd import lib

    autosteer_cases.check_lane_rows(lib)


@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
@pytest.mark.parametrize("h,w", [(4, 5), (6, 16)])
@pytest.mark.parametrize("replicate", [False, True])
def test_rowpair_conv_kernel_against_fp64(precision, h, w, replicate):
    from autoware_vision_pilot_amd import lib

    autosteer_cases.check_rowpair(lib, precision, h, w, replicate)


def test_range_guard_then_a_sound_frame(x3, wants):
    from autoware_vision_pilot_amd import lib

    bad = ref.preprocess(_frame(SEEDS[0]))
    bad[1, 200, 300] = np.inf
    with pytest.raises(lib.VpRangeError):
        x3.infer_tensor(bad)
    x3.infer(_frame(SEEDS[0]))
    got = x3.logits().reshape(2, 64)
    assert _rel(got[0], wants[0][0]) <= 1e-3 and _rel(got[1], wants[0][1]) <= 1e-3


def test_infer_twin(net, tmp_path, x3):
    from autoware_vision_pilot_amd import infer

    path = tmp_path / "autosteer.vpw"
    path.write_bytes(bytes(net[1]))
    twin = infer.AutoSteerNetworkInfer(autosteer_checkpoint_path=str(path), precision="fp16x3")
    try:
        f = _frame(SEEDS[1])
        xp, h = twin.inference(f)
        assert xp.shape == (64,) and h.shape == (64,)
        x3.infer(f)
        got = x3.logits().reshape(2, 64)
        assert np.array_equal(xp, got[0]) and np.array_equal(h, got[1])
        with pytest.raises(ValueError):
            twin.inference(np.zeros((320, 640, 3), np.uint8))
    finally:
        twin.model.close()
