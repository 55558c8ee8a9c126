"""Status codes and messages of the single-operator entries that validate their arguments up front (vp_op_conv2d, vp_compose_upconv, vp_op_upconv:
include/vp_hip.h), on the CPU through the HIP-on-CPU shim of tests/emul.  Called through the raw ctypes functions: the Python wrappers turn every
failure into one exception type and hide the code.  Every expected value is what the entries returned while each carried its own try / catch ladder."""
import ctypes as ct
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))

VP_ERR_ARG, VP_ERR_HIP, VP_ERR_RANGE = -1, -3, -5
VP_FP16, VP_FP16X3 = 0, 1


@pytest.fixture(scope="module")
def so():
    import build as emul_build

    from autoware_vision_pilot_amd import lib

    if not os.path.exists(emul_build.CLANG):
        pytest.skip("host clang++ of the ROCm toolchain not found")
    so = ct.CDLL(emul_build.build(), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    for name in ("vp_op_conv2d", "vp_compose_upconv", "vp_op_upconv"):
        fn = getattr(so, name)
        fn.restype, fn.argtypes = lib._SIGS[name]
    return so


def _p(a):
    return None if a is None else a.ctypes.data_as(ct.c_void_p)


def _call(fn, *args):
    err = ct.create_string_buffer(b"untouched", 512)
    rc = fn(*args, err, len(err))
    return rc, err.value.decode()


def _conv2d(so, x, weight, bias, out, mode=0, ks=3, act=0, res_mode=0, res=None, precision=VP_FP16X3):
    cin, h, w = (8, 1, 1) if x is None else x.shape
    return _call(so.vp_op_conv2d, 0, precision, mode, _p(x), cin, h, w, _p(weight), _p(bias), 8, ks, act, res_mode, _p(res), -1, -1, -1, _p(out))


def _stage(value=0.01):
    """a 1 x 1 map, 8-channel stage: x, wt, bt, w3, b3, out"""
    f = np.float32
    return dict(x=np.ones((8, 1, 1), f), wt=np.full((8, 8, 2, 2), value, f), bt=np.zeros(8, f), w3=np.full((8, 8, 3, 3), value, f), b3=np.zeros(8, f),
                out=np.zeros((8, 2, 2), f))


def _upconv(so, t, precision=VP_FP16X3, **null):
    a = {k: (None if k in null else v) for k, v in t.items()}
    return _call(so.vp_op_upconv, 0, _p(a["x"]), 8, 1, 1, None, 0, _p(a["wt"]), _p(a["bt"]), None, None, _p(a["w3"]), _p(a["b3"]), 8, 8, 0, -1, 0, precision,
                 _p(a["out"]))


def _compose(so, t, **null):
    a = {k: (None if k in null else v) for k, v in t.items()}
    wx, bias = np.zeros((4, 4, 8, 8)), np.zeros((9, 8))
    return _call(so.vp_compose_upconv, 0, _p(a["wt"]), _p(a["bt"]), None, None, _p(a["w3"]), _p(a["b3"]), 8, 8, 8, 0, _p(None if "wx" in null else wx), None, _p(bias))


@pytest.mark.parametrize("null", ["x", "weight", "bias", "out"])
def test_conv2d_null_required_pointer(so, null):
    f = np.float32
    a = dict(x=np.ones((8, 1, 1), f), weight=np.zeros((8, 8, 3, 3), f), bias=np.zeros(8, f), out=np.zeros((8, 1, 1), f))
    a[null] = None
    assert _conv2d(so, **a) == (VP_ERR_ARG, "bad argument")


@pytest.mark.parametrize("null", ["x", "wt", "bt", "w3", "b3", "out"])
def test_upconv_null_required_pointer(so, null):
    assert _upconv(so, _stage(), **{null: True}) == (VP_ERR_ARG, "bad argument")


@pytest.mark.parametrize("null", ["wt", "bt", "w3", "b3", "wx"])
def test_compose_upconv_null_required_pointer(so, null):
    assert _compose(so, _stage(), **{null: True}) == (VP_ERR_ARG, "bad argument")


@pytest.mark.parametrize("precision", [2, VP_FP16X3 | 16, VP_FP16X3 | 64, -1])
def test_upconv_refuses_other_precisions(so, precision):
    """ahead of the pointer checks: a null pointer beside a bad precision reports the precision"""
    assert _upconv(so, _stage(), precision=precision) == (VP_ERR_ARG, "precision must be VP_FP16 or VP_FP16X3")
    assert _upconv(so, _stage(), precision=precision, x=True) == (VP_ERR_ARG, "precision must be VP_FP16 or VP_FP16X3")


def test_conv2d_mode_3_wants_a_3x3(so):
    f = np.float32
    rc, msg = _conv2d(so, np.ones((8, 4, 4), f), np.zeros((8, 8, 1, 1), f), np.zeros(8, f), np.zeros((8, 4, 4), f), mode=3, ks=1)
    assert (rc, msg) == (VP_ERR_ARG, "mode 3: 3x3, no activation, no residual")


def test_weights_beyond_fp16_after_composition(so):
    """vp_op_upconv alone among the operator entries answers VP_ERR_RANGE; vp_op_conv2d reports the same refusal of the same weights as VP_ERR_HIP"""
    refusal = r"weight 1\d{30}\.0+ is outside the fp16 range the matrix pipe carries \(\|w\| <= 65504\): re-scale the checkpoint"
    t = _stage(1e30)
    rc, msg = _upconv(so, t)
    assert rc == VP_ERR_RANGE and re.fullmatch(refusal, msg), (rc, msg)
    rc, msg = _conv2d(so, t["x"], t["w3"], t["b3"], np.zeros((8, 1, 1), np.float32))
    assert rc == VP_ERR_HIP and re.fullmatch(refusal, msg), (rc, msg)


def test_a_good_call_still_succeeds(so):
    t = _stage()
    assert _upconv(so, t)[0] == 0 and np.isfinite(t["out"]).all() and np.abs(t["out"]).max() > 0
    assert _compose(so, t)[0] == 0
