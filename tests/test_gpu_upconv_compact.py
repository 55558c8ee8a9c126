"""The compacted form of the composed up-sampling stage (csrc/kernels_upconv.hip, CPT) on the device: the product library's vp_op_upconv with
the developer option VP_UPCONV_COMPACT forced to 0 (patch form), forced to 1 (compacted form) and unset (the engine's rule) -- bit-identical
results, each within the parity bar of torch fp64 evaluating the three-op form.  The CASES of the emulated test (ragged maps the rule never puts
on the form: 7x13, 1x5; skip tensors of one and two chunks; K slices) and the neck's two stages the rule does put on it, at their real channel
counts (neck0 10x20, neck1 20x40)."""
import numpy as np
import pytest

from test_upconv_compact_emulated import CASES, _stage
from test_upconv_emulated import make_stage, three_op_fp64

pytestmark = pytest.mark.gpu


def _three_forms(lib, vp_opts, t, act, shape, nsplit):
    outs = []
    for compact in ("0", "1", None):
        if compact is None:
            vp_opts.delenv("VP_UPCONV_COMPACT")
        else:
            vp_opts.setenv("VP_UPCONV_COMPACT", compact)
        outs.append(lib.op_upconv(t["x"], t["wt"], t["bt"], t["w3"], t["b3"], skip=t["skip"], ws=t["ws"], bs=t["bs"], act=act, shape=shape, nsplit=nsplit))
    vp_opts.delenv("VP_UPCONV_COMPACT")
    rect, comp, auto = outs
    assert np.isfinite(rect).all()
    assert np.array_equal(comp.view(np.uint32), rect.view(np.uint32)), f"max |diff| {np.abs(comp - rect).max():.3e}"
    assert np.array_equal(auto.view(np.uint32), rect.view(np.uint32))
    ref = three_op_fp64(t, act)
    for got in outs:
        err = float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
        assert err <= 2e-5, err


@pytest.mark.parametrize("h,w,shape,nsplit,cs,act", CASES)
def test_compacted_equals_patch_form_on_the_device(vp_opts, h, w, shape, nsplit, cs, act):
    from autoware_vision_pilot_amd import lib

    _three_forms(lib, vp_opts, _stage(h * 1000 + w * 10 + shape + cs, 64, 48, 128, cs, h, w), act, shape, nsplit)


@pytest.mark.parametrize("shape", [6, 7])
@pytest.mark.parametrize("name,cin,cm,cout,cs,h,w,nsplit", [("neck0", 1280, 1280, 768, 80, 10, 20, 1), ("neck0", 1280, 1280, 768, 80, 10, 20, 4),
                                                            ("neck1", 768, 768, 512, 40, 20, 40, 1), ("neck1", 768, 768, 512, 40, 20, 40, 3)])
def test_neck_stages_compacted_equals_patch_form(vp_opts, name, cin, cm, cout, cs, h, w, nsplit, shape):
    from autoware_vision_pilot_amd import lib

    _three_forms(lib, vp_opts, make_stage(np.random.default_rng(cin + h + nsplit), cin, cm, cout, cs, h, w), 1, shape, nsplit)
