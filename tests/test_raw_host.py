"""Raw Bayer, P010 and GRAY16 uploads of vp_frame without a GPU: the ABI, the properties of the numpy restatement that every raw test uses as its oracle
(tests/raw_cases.py), and -- on the HIP-on-CPU emulation of the real kernel and frame code (tests/emul) -- the conversions bit for bit, the setting, the
refusals, the canvas and one consumer."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
import abi  # noqa: E402
import color_cases as kc  # noqa: E402
import raw_cases as rc  # noqa: E402


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


# ---- the ABI
def test_new_symbols_and_codes_are_declared_exported_and_bound():
    from autoware_vision_pilot_amd import lib

    src = abi.header_source()
    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in rc.NEW_SYMBOLS:
        assert s in declared and s in exported and s in lib.EXPORTED_SYMBOLS, s
    for name, code in rc.CODES.items():
        assert lib.FRAME_FORMATS[name] == code and f"VP_FRAME_{name.upper()} = {code}" in src
    assert not set(lib.FRAME_FORMATS.values()) & (set(range(8, 16)) | {19})          # 8 .. 15 and 19 stay unknown
    assert "typedef struct vp_raw { int bits, shift, black; int gains[3]; int ccm_on; int ccm[9]; const uint8_t* lut; int lut_len; } vp_raw;" in src
    assert ct.sizeof(lib.Raw) == 16 * 4 + 8 + 8                                      # the C layout: 16 ints, the pointer, lut_len and the tail's padding
    assert lib.Raw.lut.offset == 64 and lib.Raw.lut_len.offset == 72


# ---- the restatement's own properties (pure numpy)
@pytest.mark.parametrize("B", (8, 10, 12, 16))
def test_constant_colour_comes_back_exact(B):
    """a picture constant per channel, mosaicked in any order, comes back exact at every pixel, borders included"""
    M = (1 << B) - 1
    container = 8 if B == 8 else 16
    for h, w in rc.SHAPES:
        for order in rc.ORDERS:
            for colour in ((M, 0, M // 3), (1, M - 1, M // 2), (M, M, M)):
                rgb = np.broadcast_to(np.array(colour, np.int64), (h, w, 3))
                raw = rc.mosaic(order, rgb)
                (R, G, Bl), bits = rc.raw_to_rgb(order, raw, container, bits=0 if B == container else B)
                assert bits == B
                assert (R == colour[0]).all() and (G == colour[1]).all() and (Bl == colour[2]).all(), (B, h, w, order, colour)


def test_grbg_is_rggb_shifted_by_one_column():
    raw = rc.random_raw(34, 67, 16, 1, bits=12, extra=0)
    a = rc.raw_to_bgr("grbg", raw[:, 1:], 16, bits=12, gains=rc.GAINS)
    b = rc.raw_to_bgr("rggb", raw[:, :-1], 16, bits=12, gains=rc.GAINS)
    assert np.array_equal(a[:, 1:-2], b[:, 2:-1])           # raw columns 2 .. 64: away from the border columns of either picture
    c = rc.raw_to_bgr("gbrg", raw[1:], 16, bits=12, gains=rc.GAINS)
    d = rc.raw_to_bgr("rggb", raw[:-1], 16, bits=12, gains=rc.GAINS)
    assert np.array_equal(c[1:-2], d[2:-1])                  # and GBRG is RGGB shifted by one row
    assert not np.array_equal(a[:, 1:-1], b[:, 1:-1])


@pytest.mark.parametrize("container,B", ((8, 8), (16, 10), (16, 12), (16, 14), (16, 16)))
def test_identity_matrix_and_linear_lut_are_the_defaults(container, B):
    raw = rc.random_raw(34, 66, container, 2, bits=0 if B == container else B)
    bits = 0 if B == container else B
    plain = rc.raw_to_bgr("bggr", raw, container, bits=bits)
    assert np.array_equal(rc.raw_to_bgr("bggr", raw, container, bits=bits, ccm=(1024, 0, 0, 0, 1024, 0, 0, 0, 1024), lut=rc.linear_lut(B)), plain)
    assert plain.min() == 0 and plain.max() == 255


def test_arithmetic_fits_32_bits():
    assert 65535 * 16383 + 128 < 2 ** 31 and 3 * 8191 * 65535 + 512 < 2 ** 31


def test_narrowing_rounds_and_clamps():
    assert rc.narrow16([0, 127, 128, 0x807F, 0x8080, 0xFF7F, 0xFF80, 0xFFFF]).tolist() == [0, 0, 1, 128, 129, 255, 255, 255]
    ten = np.arange(1024) << 6                                # 10-bit samples, MSB-aligned: every code lands on round(code / 4)
    assert np.array_equal(rc.narrow16(ten), np.minimum(255, (np.arange(1024) + 2) >> 2))


# ---- the emulated library
@pytest.mark.parametrize("name,order,container,kw,hw", rc.CONVERSION_CASES, ids=[c[0] for c in rc.CONVERSION_CASES])
def test_conversion_bit_for_bit_emulated(emu_lib, name, order, container, kw, hw):
    rc.check_conversion(emu_lib, order, container, kw, hw)


@pytest.mark.parametrize("order,container,B,shift", rc.TABLE_CASES, ids=[f"{c[0]}{c[1]}-b{c[2]}" for c in rc.TABLE_CASES])
def test_value_table_emulated(emu_lib, order, container, B, shift):
    rc.check_table(emu_lib, order, container, B, shift)


@pytest.mark.parametrize("fmt,h,w,extras", rc.DEEP_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in rc.DEEP_CASES])
def test_p010_and_gray16_equal_the_narrowed_uploads_emulated(emu_lib, fmt, h, w, extras):
    rc.check_deep(emu_lib, fmt, h, w, extras)


def test_row_ends_inside_a_store_block_emulated(emu_lib):
    rc.check_row_ends_inside_a_store_block(emu_lib)


def test_zeros_behind_a_row_end_emulated(emu_lib):
    """under the emulation vp_canvas_device hands out host memory"""
    rc.check_zeros_behind_a_row_end(emu_lib, ct.string_at)


def test_setting_applies_to_later_uploads_emulated(emu_lib):
    rc.check_setting_applies_to_later_uploads(emu_lib)


def test_refusals_emulated(emu_lib):
    rc.check_refusals(emu_lib)


def test_canvas_refuses_the_new_codes_emulated(emu_lib):
    rc.check_canvas_refuses(emu_lib)


def test_rectification_composes_emulated(emu_lib):
    rc.check_rectification_composes(emu_lib)


def test_consumer_equals_host_path_emulated(emu_lib):
    """AutoDrive (fp16), odd offset and odd size out of a bayer_grbg16 frame.  The region copy under test is the same for every engine kind; the two
    passes the comparison needs take over a minute on an emulated scene network and under a second here.  SceneSeg is the consumer of the GPU test."""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    eng = emu_lib.Engine("autodrive", vw.pack_state_dict(synthetic.make_autodrive_state_dict(0)), precision="fp16")
    try:
        rc.check_consumer_equals_host(emu_lib, eng)
    finally:
        eng.close()
