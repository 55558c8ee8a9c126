"""The attention, SPPF and max-pool kernels of kernels_autodrive.hip at the plans' token counts, at their limits and at the softmax's value edges, on the CPU:
the bodies of tests/attention_cases.py on the HIP-on-CPU emulation (tests/emul: the real kernel sources).  The device twin is tests/test_gpu_attention.py."""
import ctypes as ct
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))

import attention_cases as cases   # noqa: E402

MAP_ID = lambda m: "%dx%d" % m   # noqa: E731


@pytest.fixture(scope="module")
def be():
    import backends
    import build as emul_build

    if not os.path.exists(emul_build.CLANG):
        pytest.skip("host clang++ of the ROCm toolchain not found")
    return backends.load("emu")


@pytest.fixture(scope="module")
def emu_lib(be):
    from autoware_vision_pilot_amd import lib

    so = ct.CDLL(be.path, mode=os.RTLD_LOCAL | os.RTLD_NOW)     # never RTLD_GLOBAL: same symbol names as libvp_hip.so
    for name, (res, args) in lib._SIGS.items():
        fn = getattr(so, name)
        fn.restype, fn.argtypes = res, args
    saved = lib._lib
    lib._lib = so
    yield lib
    lib._lib = saved


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    cases.table()


def test_plan_shapes(be, emu_lib):
    cases.check_plan_shapes(be, emu_lib)


@pytest.mark.parametrize("hw", cases.EDGE_MAPS, ids=MAP_ID)
def test_token_count_edges(be, hw):
    cases.check_token_edge(be, *hw)


@pytest.mark.parametrize("hw", cases.REFUSED_MAPS, ids=MAP_ID)
def test_block_kernel_limit(be, hw):
    cases.check_block_limit(be, *hw)


@pytest.mark.parametrize("name", cases.VALUE_EDGES, ids=lambda n: n.replace(" ", "_"))
def test_softmax_value_edges(be, name):
    cases.check_value_edge(be, name)


@pytest.mark.parametrize("s", cases.ACT_EXPS)
def test_activation_scale_form(be, s):
    cases.check_act_scale(be, s)


@pytest.mark.parametrize("dk,dv", cases.HEAD_SIZES)
def test_other_head_sizes(be, dk, dv):
    cases.check_head_size(be, dk, dv)


def test_out_and_vout_of_different_pitches_are_refused(be):
    cases.check_pitch_refusal(be)


def test_three_launches_are_bit_identical(be):
    cases.check_determinism(be)


@pytest.mark.parametrize("hw", cases.SPPF_MAPS, ids=MAP_ID)
def test_sppf_pool_is_three_chained_maxpools(be, hw):
    cases.check_sppf(be, *hw)


def test_sppf_pool_refusals(be):
    cases.check_sppf_refusals(be)


def test_maxpool_chain_equals_sppf_pool(be):
    cases.check_chain_equals_sppf(be)


def test_maxpool_chain_on_a_map_above_512_pixels(be):
    cases.check_chain_large_map(be)


def test_block_as_the_plan_runs_it(be):
    cases.check_block_as_planned(be)
