"""vp_op_conv3x3_f8 on the CPU-emulated library (tests/emul: the real kernel, packer and launch on the HIP-on-CPU shim; the e4m3 MFMA there is the
four-fp16-MFMA form of the same fragments) against the numpy restatement of tests/f8_cases.py.  The device twin is tests/test_gpu_f8.py."""
import ctypes as ct
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emul"))
sys.path.insert(0, HERE)
import f8_cases as fc  # noqa: E402


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


@pytest.mark.parametrize("shape", fc.SHAPES)
def test_exact_integers_bit_for_bit(emu_lib, shape):
    fc.check_exact(emu_lib.conv3x3_f8, shape)


@pytest.mark.parametrize("shape", fc.SHAPES)
def test_random_operands_within_the_fp16_operator_bound(emu_lib, shape):
    for qexp in (-2, 0, 3):
        for act in (0, 1):
            fc.check_random(emu_lib.conv3x3_f8, shape, qexp, act)


def test_refuses_channel_counts_off_the_64_grid(emu_lib):
    fc.check_refusals(emu_lib.conv3x3_f8)


def test_device_quantiser_equals_the_host_entry(emu_lib):
    import numpy as np

    every = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    for qexp in fc.EXPS:
        assert np.array_equal(emu_lib.fp8_quantize(every, qexp), emu_lib.fp8_quantize_act(every, qexp)), qexp
