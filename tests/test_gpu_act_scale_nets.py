"""VP_ACT_SCALE for the AutoSpeed and AutoSteer engines on the device: the four hand-written kernels with exponents at the smallest shapes at which they
can go wrong, and the whole engines at 512 x 1024 -- bit-identity while every exponent is 0 (both plans), the ordinary case against the networks' golden
references, the band, the ill-scaled checkpoints of tests/golden/act_scale_nets.npz (tools/pin_act_scale_nets.py) that the unflagged engines refuse, the
shipped table and the reset.  The cases are tests/act_scale_nets_cases.py (shared with the emulated suite); the timings go to
profiles/act_scale_nets.txt by tools/bench_act_scale_nets.py."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import act_scale_nets_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib

    return lib


@pytest.mark.parametrize("exp", cases.EXPS)
@pytest.mark.parametrize("nch", [8, 16])
def test_upsample2_cat(lib, nch, exp):
    cases.check_upsample2_cat(lib, nch, exp)


@pytest.mark.parametrize("in_exp,out_exp", [(0, 0), (6, -3), (-3, 6), (6, 0), (0, -3)])
@pytest.mark.parametrize("replicate", [False, True])
@pytest.mark.parametrize("cin", [8, 64])
def test_rowpair_conv(lib, cin, replicate, in_exp, out_exp):
    cases.check_rowpair(lib, cin, replicate, in_exp, out_exp)


@pytest.mark.parametrize("in_exp", cases.EXPS)
@pytest.mark.parametrize("cin", [8, 64])
def test_lane_rows_head(lib, cin, in_exp):
    cases.check_lane_rows(lib, cin, in_exp)


@pytest.mark.parametrize("exps", [(0,) * 6, (6, -3, -3, 6, 6, 6), (-3, 0, 6, -3, 0, 6)])
@pytest.mark.parametrize("nc", [1, 4])
def test_detect_head_decode(lib, nc, exps):
    cases.check_detect(lib, nc, exps)


@pytest.mark.parametrize("latency", [False, True])
@pytest.mark.parametrize("net", ["autospeed", "autosteer"])
def test_zero_exponents_are_the_unflagged_engine(lib, net, latency):
    cases.check_zero_exponents(cases.Net(lib, net), latency)


@pytest.mark.parametrize("latency", [False, True])
@pytest.mark.parametrize("net", ["autospeed", "autosteer"])
def test_ordinary_case_band_table_and_reset(lib, net, latency):
    cases.check_ordinary_band_and_table(cases.Net(lib, net), latency)


@pytest.mark.parametrize("net", ["autospeed", "autosteer"])
def test_range_case(lib, net):
    cases.check_range_case(cases.Net(lib, net))


@pytest.mark.parametrize("net", ["autospeed", "autosteer"])
def test_tie_groups_and_refusals(lib, net):
    N = cases.Net(lib, net)
    blob = N.blob("ordinary")
    eng, _ = N.engine(blob, act_scale=True)
    cases.check_tie_groups(eng, net)
    with pytest.raises(ValueError, match="VP_ACT_SCALE needs VP_FP16X3"):
        lib.Engine(net, blob, precision="fp16", act_scale=True)
    N.close()


def test_autosteer_infer_class_calibrates_on_its_first_frame(lib, tmp_path):
    import numpy as np

    from autoware_vision_pilot_amd import infer

    N = cases.Net(lib, "autosteer")
    path = tmp_path / "autosteer.vpw"
    path.write_bytes(bytes(N.blob("range")))
    m = infer.AutoSteerNetworkInfer(str(path), precision="fp16x3", act_scale=True)
    xp, h = m.inference(N.frame)
    assert m.model.act_scales().any()
    assert cases.rel(xp, N.fix["autosteer_range_xp"]) <= cases.NET_BAR and cases.rel(h, N.fix["autosteer_range_h_vector"]) <= cases.NET_BAR
    assert np.isfinite(xp).all() and np.isfinite(h).all()
    m.model.close()
