"""The JPEG stream of vp_canvas_fetch_jpeg without a GPU: the numpy twin (tests/jpeg_ref.py) against an independent implementation -- Pillow with
libjpeg-turbo writes the tables the twin must carry and decodes every stream the twin makes -- the integer DCT against scipy, and the library's host-only
entries against the twin.  The device never is the reference here."""
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_cases as jc  # noqa: E402
import jpeg_ref as ref  # noqa: E402


def segments(stream):
    """[(marker, payload)] of a JPEG file up to SOS"""
    out, p = [], 2
    assert stream[:2] == b"\xff\xd8"
    while True:
        assert stream[p] == 0xFF
        marker, n = stream[p + 1], int.from_bytes(stream[p + 2:p + 4], "big")
        out.append((marker, stream[p + 4:p + 2 + n]))
        p += 2 + n
        if marker == 0xDA:
            return out


def pillow_stream(bgr, quality):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, "JPEG", quality=quality, subsampling=2, optimize=False)
    return buf.getvalue()


def tables_of(stream):
    """({table index: 64 zigzag bytes}, {(class, index): BITS + HUFFVAL}) of a file, whether it packs several tables into one segment or not"""
    dqt, dht = {}, {}
    for marker, payload in segments(stream):
        p = 0
        while marker == 0xDB and p < len(payload):
            assert payload[p] >> 4 == 0     # 8-bit precision
            dqt[payload[p] & 15] = payload[p + 1:p + 65]
            p += 65
        while marker == 0xC4 and p < len(payload):
            n = sum(payload[p + 1:p + 17])
            dht[(payload[p] >> 4, payload[p] & 15)] = payload[p + 1:p + 17 + n]
            p += 17 + n
    return dqt, dht


@pytest.mark.parametrize("quality", (1, 25, 50, 75, 90, 100))
def test_tables_equal_the_ones_pillow_writes(quality):
    """(a) the independent pin of the quantisation scaling and of the four Huffman tables"""
    dqt, dht = tables_of(pillow_stream(jc.picture("noise", 16, 16), quality))
    mine_q, mine_h = tables_of(ref.header(16, 16, quality, 1))
    assert set(dqt) == set(mine_q) == {0, 1} and set(dht) == set(mine_h) == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert dqt == mine_q
    assert dht == mine_h


def test_header_layout():
    markers = [m for m, _ in segments(ref.header(18, 34, 75, 3))]
    assert markers == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    seg = dict((m, p) for m, p in segments(ref.header(18, 34, 75, 3)) if m in (0xE0, 0xC0, 0xDD, 0xDA))
    assert seg[0xE0] == b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    assert seg[0xC0] == bytes([8, 0, 18, 0, 34, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert seg[0xDD] == b"\x00\x03" and seg[0xDA] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert segments(ref.header(18, 34, 75, 0))[8][1] == ref.DEFAULT_RESTART_MCUS.to_bytes(2, "big")


def test_the_default_restart_interval_is_four():
    """the literal default include/vp_hip.h documents and profiles/canvas_jpeg.txt selects, in the twin and in the shipped library's DRI segment"""
    from autoware_vision_pilot_amd import lib

    assert ref.DEFAULT_RESTART_MCUS == 4
    for header in (ref.header(48, 64, 75, 0), lib.jpeg_header(48, 64, 75, 0)):
        assert segments(header)[8] == (0xDD, b"\x00\x04")
        assert header == ref.header(48, 64, 75, 4)
    assert lib.jpeg_bound(48, 64, 0) == lib.jpeg_bound(48, 64, 4) != lib.jpeg_bound(48, 64, 2)
    with pytest.raises(ValueError, match="default 4"):
        lib.jpeg_bound(48, 64, -1)


def test_the_cases_reach_every_path_of_the_coder():
    jc.coverage()


@pytest.mark.parametrize("case", jc.CASES, ids=jc.case_id)
def test_pillow_decodes_every_case(case):
    """(b) an independent decoder accepts the stream and finds the picture in it.  libjpeg only warns about a damaged scan, so loading is not enough: the
    decoded picture must be, to the pixel, the one Pillow decodes from the same picture's stream with ONE interval (restart markers and predictor resets
    change no sample), and as close to the original as Pillow's own encode of it (PSNR_GAP below) -- at every case's own Ri, the default included"""
    p, h, w, q, ri = case
    stream = jc.stream_of(case)[0]
    assert stream[-2:] == b"\xff\xd9"
    im = Image.open(io.BytesIO(stream))
    assert im.format == "JPEG" and im.size == (w, h) and im.mode == "RGB"
    im.load()
    got = np.asarray(im)
    assert got.shape == (h, w, 3)
    bgr = jc.picture(p, h, w)
    one = np.asarray(Image.open(io.BytesIO(jc.stream_of((p, h, w, q, 65535))[0])).convert("RGB"))
    assert np.array_equal(got, one), (case, np.argwhere(got != one)[:4])
    rgb = bgr[..., ::-1]
    mine, theirs = psnr(got, rgb), psnr(np.asarray(Image.open(io.BytesIO(pillow_stream(bgr, q))).convert("RGB")), rgb)
    print(jc.case_id(case), "PSNR", round(mine, 3), "Pillow's", round(theirs, 3))
    assert mine >= theirs - PSNR_GAP[q], (case, mine, theirs)


def test_restart_markers_sit_between_the_intervals():
    stream, _ = jc.stream_of(("frame", 16, 272, 75, 1))
    scan = stream[ref.HEADER_BYTES:-2]
    found = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert found == [0xD0 + i % 8 for i in range(16)]          # 17 intervals: the index wraps past 7, none behind the last
    assert all(scan[i + 1] == 0 or 0xD0 <= scan[i + 1] <= 0xD7 for i in range(len(scan) - 1) if scan[i] == 0xFF) and scan[-1] != 0xFF


def test_dct_rule():
    """(c) the integer DCT is within 1 of the orthonormal DCT on random and extreme blocks, its intermediate bounds hold and the AC clamp is unreachable"""
    from scipy.fft import dctn

    M = ref.dct_matrix()
    assert M[0, 0] == 2896 and M[1, 0] == 4017 and np.abs(M).max() == 4017
    rng = np.random.default_rng(0)
    blocks = [rng.integers(-128, 128, size=(2000, 8, 8))]
    for k in range(8):
        for l in range(8):   # the blocks that drive one coefficient to its extreme, both signs
            s = np.sign(np.outer(M[l], M[k]))
            s[s == 0] = 1
            ext = np.where(s > 0, 127, -128)
            blocks.append(np.stack([ext, -1 - ext]))
    blocks.append(np.stack([np.full((8, 8), 127), np.full((8, 8), -128)]))
    x = np.concatenate(blocks)
    F = ref.fdct(x)
    exact = dctn(x.astype(np.float64), axes=(1, 2), norm="ortho")
    err = np.abs(F - exact).max()
    print("largest |F - exact|", err)       # 0.648 on these blocks
    assert err <= 1.0, err
    assert np.abs(np.rint(exact) - F).max() <= 1
    T = (np.einsum("kn,byn->byk", M, x) + 512) >> 10
    assert np.abs(T).max() <= 2896
    assert np.abs(np.einsum("lm,bmk->blk", M, T)).max() < 1 << 26
    # from M's row sums alone (positive and negative entries apart, samples in -128 .. 127): the interval of T[.][k], then of F[l][k]; every AC position
    # stays inside +-1023, so the clamp is never reached
    pos, neg = np.clip(M, 0, None).sum(axis=1), np.clip(-M, 0, None).sum(axis=1)
    thi, tlo = (pos * 127 + neg * 128 + 512) >> 10, (-(pos * 128 + neg * 127) + 512) >> 10
    fhi = (pos[:, None] * thi[None, :] - neg[:, None] * tlo[None, :] + (1 << 15)) >> 16
    flo = (pos[:, None] * tlo[None, :] - neg[:, None] * thi[None, :] + (1 << 15)) >> 16
    fhi[0, 0] = flo[0, 0] = 0
    print("AC interval from the row sums", flo.min(), fhi.max())
    assert fhi.max() < 1023 and flo.min() > -1023, (flo.min(), fhi.max())
    assert max(thi.max(), -tlo.min()) == 2896 and (pos + neg).max() * 2896 < 1 << 26      # int32 sums with room


# (d) closeness, measured on the case pictures at 16 x 16, 18 x 34, 48 x 64 and 176 x 320 with Pillow 12.2.0 / libjpeg-turbo on the development box
# (profiles/canvas_jpeg.txt).  At quality 100 im.draft("YCbCr") of the twin's stream against the I420 planes the stream was made of: the largest
# difference of the Y plane was 1 on every picture; of the 2x2 means of the decoded (smoothly up-sampled) chroma planes it was frame 28, grey 0,
# noise 43, checker 0, ramp 4.  Bound = that maximum + 1 code value, for another libjpeg's IDCT.
Y_BOUND = 2
CHROMA_BOUND = {"frame": 29, "grey": 1, "noise": 44, "checker": 1, "ramp": 5}
# At every quality PSNR(decode(twin), picture) >= PSNR(decode(Pillow's own encode, same quality and subsampling), picture) - gap; the largest gaps
# measured were 0.289, 0.135, 0.160, 0.464, 0.024 dB at quality 1, 50, 75, 90, 100, rounded up to 0.1 dB (on the cases of tests/jpeg_cases.py, the 2 x 2
# and 16 x 272 ones included, the largest were 0.011, 0.100, 0.018, 0.464, 0.000 dB).  One addition to the comparison as the issue words it: a PSNR counts as
# at most 60 dB (an RMS error of a quarter of a code value).  Without it the comparison has no value where Pillow's encode comes back exact (flat grey, the
# checkerboards at quality 100: PSNR infinite) while the integer DCT leaves a few pixels one code value off (checker 18 x 34 at quality 100: 76.0 dB).
PSNR_GAP = {1: 0.3, 50: 0.2, 75: 0.2, 90: 0.5, 100: 0.1}
CLOSENESS_SIZES = ((16, 16), (18, 34), (48, 64), (176, 320))


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 60.0 if mse == 0 else min(60.0, 10.0 * np.log10(255.0 ** 2 / mse))


@pytest.mark.parametrize("kind", ("frame", "grey", "noise", "checker", "ramp"))
def test_closeness_to_the_samples_and_to_pillows_encoder(kind):
    for h, w in CLOSENESS_SIZES:
        bgr = jc.picture(kind, h, w)
        Y, U, V = (p.astype(int) for p in ref.planes_of(bgr))
        im = Image.open(io.BytesIO(ref.encode(bgr, 100, 1)))
        im.draft("YCbCr", (w, h))
        a = np.asarray(im).astype(int)
        assert im.mode == "YCbCr" and a.shape == (h, w, 3)
        mean4 = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2   # noqa: E731
        dy, dc = np.abs(a[..., 0] - Y).max(), max(np.abs(mean4(a[..., 1]) - U).max(), np.abs(mean4(a[..., 2]) - V).max())
        print(kind, h, w, "Y", dy, "chroma", dc)
        assert dy <= Y_BOUND and dc <= CHROMA_BOUND[kind], (kind, h, w, dy, dc)
        rgb = bgr[..., ::-1]
        for q in jc.QUALITIES:
            mine = psnr(np.asarray(Image.open(io.BytesIO(ref.encode(bgr, q, 1))).convert("RGB")), rgb)
            theirs = psnr(np.asarray(Image.open(io.BytesIO(pillow_stream(bgr, q))).convert("RGB")), rgb)
            print(kind, h, w, "quality", q, "PSNR", round(mine, 3), "Pillow's", round(theirs, 3))
            assert mine >= theirs - PSNR_GAP[q], (kind, h, w, q, mine, theirs)


def test_quality_scaling():
    assert (ref.quant_tables(50)[0] == ref.BASE_LUMA).all() and (ref.quant_tables(100)[1] == 1).all()
    assert ref.quant_tables(1)[0].max() == 255 and ref.quant_tables(1)[0].min() == 255      # 5000 / 1: every entry clamps
    assert ref.quant_tables(25)[0][0] == (16 * 200 + 50) // 100


def test_library_header_and_bound_equal_the_twin():
    """(e) the host-only entries of the shipped library, no device"""
    from autoware_vision_pilot_amd import lib

    jc.check_host_entries(lib)


def test_symbols_declared_exported_bound():
    import abi
    from autoware_vision_pilot_amd import lib

    new = {"vp_canvas_fetch_jpeg", "vp_canvas_fetch_jpeg_resized", "vp_op_jpeg_encode_bgr8", "vp_jpeg_bound", "vp_jpeg_header"}
    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in new:
        assert s in declared and s in exported and s in lib.EXPORTED_SYMBOLS and s in lib._SIGS, s
    assert {s for s in declared if "jpeg" in s} == new
    for name in ("fetch_jpeg",):
        assert callable(getattr(lib.Canvas, name))
    for name in ("jpeg_encode", "jpeg_bound", "jpeg_header"):
        assert callable(getattr(lib, name))
