"""vp_lanes on the HIP-on-CPU emulation of the real kernel and host class (tests/emul): the hand-made cases and 20 generated frames through
vp_lanes_add_logits / vp_lanes_fetch / vp_lanes_fetch_points -- start points, windows, point lists in order and moments bit for bit against the numpy
twin, the coefficients within one ulp of the exact solution, the smoothing sequence and the refusals that need no engine."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
import lane_filter_cases as lc  # noqa: E402
import lane_filter_ref as ref  # noqa: E402


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


def test_hand_made_cases_emulated(emu_lib):
    frames = [lc.HAND[k][0] for k in lc.HAND_NAMES]
    thr = [lc.HAND[k][1] for k in lc.HAND_NAMES]
    wants = [ref.LaneFilterRef().update(f, t) for f, t in zip(frames, thr)]
    for k, w in zip(lc.HAND_NAMES, wants):                       # the twin itself stands on the literal expectations
        assert tuple(lc.lane_tuple(r) for r in w) == lc.EXPECT[k], k
    lc.run_and_check(emu_lib, frames, thr, wants, capacity=5)   # 16 records through a ring of 5: the ring wraps


def test_generated_frames_emulated(emu_lib):
    frames, results, _, _ = lc.generated()
    idx = list(lc.EMULATED_FRAMES)
    lc.run_and_check(emu_lib, frames[idx], [0.0] * len(idx), [results[i] for i in idx], capacity=8)


def test_sequence_and_reset_emulated(emu_lib):
    lc.check_sequence(emu_lib)


def test_refusals_without_an_engine_emulated(emu_lib):
    lc.check_refusals_no_engine(emu_lib)
