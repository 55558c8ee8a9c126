"""vp_frame without a GPU: the ABI (header, shared library, binding), the numpy restatement of the YUV definition that every conversion test uses as its
oracle, and -- on the HIP-on-CPU emulation of the real kernel and engine code (tests/emul) -- the conversions, the upload refusals and one consumer
(AutoDrive: frame region in, the host path's bits out)."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
import abi  # noqa: E402
import frame_cases as fc  # noqa: E402

NEW_SYMBOLS = ("vp_frame_create", "vp_frame_destroy", "vp_frame_last_error", "vp_frame_upload", "vp_frame_upload_device", "vp_frame_sync", "vp_frame_dims",
               "vp_frame_fetch_bgr8", "vp_upload_from_frame", "vp_infer_frame", "vp_detect_infer_frame")


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


def test_new_symbols_are_declared_exported_and_bound():
    from autoware_vision_pilot_amd import lib

    src = abi.header_source()
    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in exported, s
        assert s in lib.EXPORTED_SYMBOLS, s
    assert all(f"VP_FRAME_{n.upper()} = {v}" in src for n, v in lib.FRAME_FORMATS.items())


def test_restatement_anchors_and_monotone_in_y():
    assert fc.yuv_to_bgr(16, 128, 128).tolist() == [0, 0, 0]
    assert fc.yuv_to_bgr(235, 128, 128).tolist() == [255, 255, 255]
    Y = np.arange(256)
    for u in fc.UV_GRID:
        for v in fc.UV_GRID:
            px = fc.yuv_to_bgr(Y, np.full(256, u), np.full(256, v)).astype(np.int64)
            assert (np.diff(px, axis=0) >= 0).all(), (u, v)
            assert (px[:17] == px[0]).all()          # the Y < 16 floor


def test_restatement_reaches_both_clamps_on_the_byte_grid():
    Y, U, V = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij", sparse=True)
    for name, c in zip("RGB", fc.yuv_raw(Y, U, V)):
        c = np.broadcast_to(c, (256, 256, 256))
        assert c.min() < 0 and c.max() > 255, name       # the clamp is live at both ends of every channel
        assert abs(int(c.min())) < (1 << 10) and int(c.max()) < (1 << 10)   # and 32-bit arithmetic has room: |y + chroma| < 2^30


@pytest.mark.parametrize("fmt,h,w,strides", fc.CONVERSION_CASES, ids=[c[0] for c in fc.CONVERSION_CASES])
def test_conversion_bit_for_bit_emulated(emu_lib, fmt, h, w, strides):
    fc.check_conversion(emu_lib, fmt, h, w, strides)


@pytest.mark.parametrize("fmt", fc.YUV)
def test_table_frame_emulated(emu_lib, fmt):
    fc.check_table(emu_lib, fmt)


def test_upload_refusals_emulated(emu_lib):
    fc.check_upload_refusals(emu_lib)


def test_reupload_changes_geometry_and_format_emulated(emu_lib):
    """one frame object, three uploads: the buffers grow, the geometry follows the last upload"""
    f = emu_lib.Frame()
    try:
        for fmt, h, w, strides in (("yuy2", 4, 6, (13,)), ("nv12", 6, 10, (12, 11)), ("gray8", 2, 3, (3,))):
            planes = fc.random_planes(fmt, h, w, strides, 7)
            f.upload(planes, fmt, hw=(h, w))
            assert f.hw() == (h, w)
            assert np.array_equal(f.fetch_bgr8(), fc.to_bgr(fmt, planes, h, w))
    finally:
        f.close()


def test_consumer_equals_host_path_emulated(emu_lib):
    """AutoDrive (fp16), odd offset and odd size out of an NV12 frame.  One engine, two passes over the same pixels: the first frame of a stream pairs with
    itself, the second pairs with an identical previous frame, so input tensor AND outputs must agree bit for bit.  Then the consumer refusals that need
    no second engine."""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    eng = emu_lib.Engine("autodrive", vw.pack_state_dict(synthetic.make_autodrive_state_dict(0)), precision="fp16")
    try:
        fc.check_consumer_equals_host(emu_lib, eng, "nv12", 48, 64, (5, 7, 41, 29))
        f = emu_lib.Frame()
        try:
            with pytest.raises(emu_lib.VpError, match="never uploaded"):
                eng.upload_from_frame(f)
            f.upload(np.zeros((8, 12, 3), np.uint8), "bgr8")
            for region in ((0, 0, 13, 8), (11, 0, 2, 2), (0, 7, 2, 2), (-1, 0, 4, 4), (0, 0, 1, 8), (0, 0, 12, 0)):
                with pytest.raises(ValueError, match="frame region"):
                    eng.upload_from_frame(f, region)
            eng.set_input_format(emu_lib.VP_RGB8, emu_lib.VP_PLANES_RGB)
            with pytest.raises(ValueError, match="VP_BGR8"):
                eng.upload_from_frame(f)
        finally:
            f.close()
    finally:
        eng.close()
