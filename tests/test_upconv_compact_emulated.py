"""The compacted form of the composed up-sampling stage (csrc/kernels_upconv.hip, CPT): a workgroup owns a run of row-major low-resolution pixels
instead of a patch, its halo image is the window of the map those pixels' taps read, fragments past the run's end issue no work.  The form changes
which pixels share a workgroup, never what is summed for a pixel or in which order, so its output must equal the patch form's BIT FOR BIT.  Executed
on the CPU through the HIP-on-CPU shim of tests/emul; the patch form is forced with the developer option VP_UPCONV_COMPACT=0, the compacted form
with VP_UPCONV_COMPACT=1 (where the rule alone would not take it: maps one patch covers)."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))


@pytest.fixture(scope="module")
def emu_lib():
    import build as emul_build

    from autoware_vision_pilot_amd import lib

    if not os.path.exists(emul_build.CLANG):
        pytest.skip("host clang++ of the ROCm toolchain not found")
    so = ct.CDLL(emul_build.build(), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    for name, (res, args) in lib._SIGS.items():
        fn = getattr(so, name)
        fn.restype, fn.argtypes = res, args
    saved = lib._lib
    lib._lib = so
    yield lib
    lib.clear_options()
    lib._lib = saved


def _stage(seed, cin, cm, cout, cs, h, w):
    rng = np.random.default_rng(seed)
    f = np.float32
    t = dict(x=rng.standard_normal((cin, h, w), dtype=f), wt=rng.standard_normal((cin, cm, 2, 2), dtype=f) * f(np.sqrt(1.0 / cin)),
             bt=rng.standard_normal(cm, dtype=f) * f(0.1), w3=rng.standard_normal((cout, cm, 3, 3), dtype=f) * f(np.sqrt(2.0 / (9 * cm))),
             b3=rng.standard_normal(cout, dtype=f) * f(0.1), skip=None, ws=None, bs=None)
    if cs:
        t.update(skip=rng.standard_normal((cs, 2 * h, 2 * w), dtype=f), ws=rng.standard_normal((cm, cs), dtype=f) * f(np.sqrt(2.0 / cs)),
                 bs=rng.standard_normal(cm, dtype=f) * f(0.1))
    return t


def _run(lib, t, compact, shape, nsplit, act):
    lib.set_option("VP_UPCONV_COMPACT", compact)
    try:
        return lib.op_upconv(t["x"], t["wt"], t["bt"], t["w3"], t["b3"], skip=t["skip"], ws=t["ws"], bs=t["bs"], act=act, shape=shape, nsplit=nsplit)
    finally:
        lib.set_option("VP_UPCONV_COMPACT", None)


def _fits(lib, h, w, shape):
    fn = getattr(lib._lib, "_ZN2vp19upconv_compact_fitsEiii")
    fn.restype, fn.argtypes = ct.c_bool, (ct.c_int, ct.c_int, ct.c_int)
    return bool(fn(h, w, shape))


def test_the_neck_maps_fit_and_wide_maps_do_not(emu_lib):
    """the two stages the form is for (10x20 on the 8-wave shape, 20x40 on the 4-wave shape) fit their LDS plans; maps too wide for a window do not"""
    assert _fits(emu_lib, 10, 20, 6) and _fits(emu_lib, 20, 40, 7)
    assert _fits(emu_lib, 7, 13, 6) and _fits(emu_lib, 7, 13, 7) and _fits(emu_lib, 1, 5, 6) and _fits(emu_lib, 1, 5, 7)
    assert not _fits(emu_lib, 40, 80, 7) and not _fits(emu_lib, 80, 160, 6)


# (h, w, shape, nsplit, cs, act): the neck's two maps on their shapes (the rule's own choice), ragged maps forced onto the form, skip tensors of one and
# two 32-channel chunks and none, K slices cutting x chunks and skip chunks
CASES = [
    (10, 20, 6, 1, 40, 1), (10, 20, 6, 3, 0, 0), (10, 20, 7, 2, 24, 1),
    (20, 40, 7, 1, 0, 1), (20, 40, 7, 3, 40, 0),
    (7, 13, 6, 1, 24, 1), (7, 13, 7, 4, 40, 1), (7, 13, 7, 1, 0, 0),
    (1, 5, 6, 2, 24, 1), (1, 5, 7, 1, 0, 1),
]


@pytest.mark.parametrize("h,w,shape,nsplit,cs,act", CASES)
def test_compacted_equals_patch_form_bit_for_bit(emu_lib, h, w, shape, nsplit, cs, act):
    t = _stage(h * 1000 + w * 10 + shape + cs, 64, 48, 128, cs, h, w)
    rect = _run(emu_lib, t, "0", shape, nsplit, act)
    comp = _run(emu_lib, t, "1", shape, nsplit, act)
    auto = _run(emu_lib, t, None, shape, nsplit, act)
    assert np.isfinite(rect).all()
    assert np.array_equal(comp.view(np.uint32), rect.view(np.uint32)), f"max |diff| {np.abs(comp - rect).max():.3e}"
    assert np.array_equal(auto.view(np.uint32), rect.view(np.uint32))
