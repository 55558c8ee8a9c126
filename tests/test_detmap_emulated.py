"""The detector-validation kernels and accumulator code on the HIP-on-CPU emulation (tests/emul), as it stands: the nb 64 and nb 1344 cases of
tests/detmap_cases.py through vp_op_detect_validate and add_det_raw / fetch_det, bit for bit against the fixture."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
import detmap_cases as dc  # noqa: E402


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


@pytest.mark.parametrize("name", dc.EMULATED)
def test_detect_validate_bit_for_bit_emulated(emu_lib, name):
    dc.check_validate(emu_lib, name)


def test_frames_rows_and_tp_words_emulated(emu_lib):
    s = dc.check_frames(emu_lib, dc.EMULATED)
    assert s["rows"] > 300 and s["labels"] == 10 and s["map"] > 0.0


def test_refusals_emulated(emu_lib):
    m = emu_lib.Metric(max_frames=1)
    try:
        raw, labels = dc.frame("small")
        for bad in (lambda: m.add_det_raw(np.zeros((4 + 81, 8), np.float32), labels), lambda: m.add_det_raw(np.zeros((5, 16385), np.float32), labels),
                    lambda: m.add_det_raw(np.zeros((4 + 80, 2048), np.float32), labels), lambda: m.add_det_raw(raw, labels, iou_v=np.zeros(17, np.float32)),
                    lambda: m.add_det_raw(raw, labels, iou_v=np.zeros(0, np.float32)), lambda: m.add_det_raw(raw, np.zeros((4097, 5), np.float32)),
                    lambda: m.add_det_raw(raw, labels, conf=float("nan"))):
            with pytest.raises(ValueError):
                bad()
        assert m.det_frames() == 0
        m.add_det_raw(raw, labels)
        with pytest.raises(emu_lib.VpError, match="full"):
            m.add_det_raw(raw, labels)
        m.reset()
        m.add_det_raw(raw, labels)
        with pytest.raises(ValueError):
            emu_lib.detect_validate(np.zeros((4, 8), np.float32))
    finally:
        m.close()
