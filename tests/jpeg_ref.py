"""The baseline JPEG stream of vp_canvas_fetch_jpeg / vp_op_jpeg_encode_bgr8 restated in numpy / Python, from the rules include/vp_hip.h states as the
DEFINITION ("vp_canvas: the picture as a baseline JPEG"): JFIF 4:2:0 samples by the canvas's BT.601 full-range forward formula with the mean chroma
rule, the integer 8x8 DCT, libjpeg's quality scaling of the Annex K tables, the typical Huffman tables of Annex K.3.3, restart intervals.  Written from
those rules and from ITU-T T.81; tests/test_jpeg_host.py pins the tables against a file Pillow writes and decodes every stream with Pillow."""
import struct

import numpy as np

import color_cases as col

STD = ("bt601", "full")
DEFAULT_RESTART_MCUS = 4   # what restart_mcus = 0 selects (include/vp_hip.h; profiles/canvas_jpeg.txt)

# natural (row-major) index of the i-th coefficient in zigzag order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
                   57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# T.81 Annex K.1 / K.2, row-major
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
# T.81 Annex K.3.3: (BITS[1..16], HUFFVAL) of tables K.3 (DC luminance), K.5 (AC luminance), K.4 (DC chrominance), K.6 (AC chrominance)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))


def _regular(first_run, first_size):
    """the tail both AC tables share: (run, size) symbols in ascending order, sizes 1 .. 10, from (first_run, first_size) on"""
    out = []
    for run in range(first_run, 16):
        for size in range(first_size if run == first_run else 1, 11):
            out.append(run << 4 | size)
    return out


AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42,
            0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35,
            0x36, 0x37, 0x38, 0x39, 0x3A] + [s for s in _regular(4, 3) if s not in (0x51, 0x52, 0x61, 0x62, 0x71, 0x72, 0x81, 0x82, 0x91, 0xA1, 0xB1, 0xC1, 0xD1, 0xF0)])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1,
              0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A,
              0x35, 0x36, 0x37, 0x38, 0x39, 0x3A] + [s for s in _regular(4, 3) if s not in (0x51, 0x52, 0x61, 0x62, 0x71, 0x72, 0x81, 0x91, 0xA1, 0xB1, 0xC1, 0xD1, 0xE1,
                                                                                                     0xF0, 0xF1)])
HUFF_SPECS = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)   # the order of the DHT segments: DC0, AC0, DC1, AC1


def huff_codes(spec):
    """{symbol: (code, length)} by T.81 Annex C: codes of one length count up, a longer length shifts left"""
    bits, vals = spec
    assert sum(bits) == len(vals) == len(set(vals))
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def dct_matrix():
    """M[k][n] = rne(2^13 s_k cos((2n + 1) k pi / 16)), formed in double; int64 [8][8]"""
    k, n = np.arange(8.0)[:, None], np.arange(8.0)[None, :]
    s = np.where(k == 0, 1.0 / (2.0 * np.sqrt(2.0)), 0.5)
    return np.rint(8192.0 * s * np.cos((2.0 * n + 1.0) * k * np.pi / 16.0)).astype(np.int64)


def fdct(x):
    """the integer forward DCT of level-shifted blocks x [..., 8][8] (rows y, columns n): F [..., l][k], int64"""
    M = dct_matrix()
    T = (np.einsum("kn,...yn->...yk", M, np.asarray(x, np.int64)) + (1 << 9)) >> 10
    return (np.einsum("lm,...mk->...lk", M, T) + (1 << 15)) >> 16


def quant_tables(quality):
    """(luminance, chrominance) tables of a quality 1 .. 100, row-major int64 [64]: libjpeg's scaling"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base.astype(np.int64) * s + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA))


def planes_of(bgr):
    """Y [h][w], Cb, Cr [h/2][w/2]: vp_canvas_fetch(I420) under (BT.601, full range, mean chroma)"""
    return col.from_bgr(STD, "mean", "i420", np.asarray(bgr))


def mcu_grid(h, w):
    return (h + 15) // 16, (w + 15) // 16


def coefficients(planes, quality):
    """quantised coefficients in zigzag order, int64 [MCU rows * MCU columns][6][64]; blocks Y00 Y01 Y10 Y11 Cb Cr"""
    Y, Cb, Cr = (np.asarray(p).astype(np.int64) for p in planes)
    h, w = Y.shape
    my, mx = mcu_grid(h, w)
    Y = np.pad(Y, ((0, 16 * my - h), (0, 16 * mx - w)), mode="edge") - 128
    C = [np.pad(c, ((0, 8 * my - h // 2), (0, 8 * mx - w // 2)), mode="edge") - 128 for c in (Cb, Cr)]
    yb = Y.reshape(my, 2, 8, mx, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(my * mx, 4, 8, 8)
    cb = [c.reshape(my, 8, mx, 8).transpose(0, 2, 1, 3).reshape(my * mx, 1, 8, 8) for c in C]
    F = fdct(np.concatenate([yb] + cb, axis=1)).reshape(my * mx, 6, 64)
    ql, qc = quant_tables(quality)
    Q = np.stack([ql] * 4 + [qc] * 2)[None]
    c = np.sign(F) * ((np.abs(F) + (Q >> 1)) // Q)
    c[:, :, 1:] = np.clip(c[:, :, 1:], -1023, 1023)
    return c[:, :, ZIGZAG]


_CODES = [huff_codes(s) for s in HUFF_SPECS]


def code_interval(coef, stats=None):
    """the entropy-coded bytes of one restart interval, coef int [n MCUs][6][64]: predictors 0, padded with 1-bits, 0xFF stuffed"""
    acc, nbits = 0, 0
    pred = [0, 0, 0]
    for mcu in coef:
        for b in range(6):
            comp = max(0, b - 3)
            dc, ac = (_CODES[0], _CODES[1]) if comp == 0 else (_CODES[2], _CODES[3])
            blk = mcu[b]
            v = int(blk[0]) - pred[comp]
            pred[comp] = int(blk[0])
            size = abs(v).bit_length()
            code, length = dc[size]
            acc, nbits = acc << length | code, nbits + length
            if size:
                acc, nbits = acc << size | ((v if v >= 0 else v - 1) & ((1 << size) - 1)), nbits + size
            if stats is not None:
                stats["dc_max"] = max(stats.get("dc_max", 0), size)
            nz = np.flatnonzero(blk[1:]) + 1
            last = 0
            for k in nz:
                run = int(k) - last - 1
                last = int(k)
                while run > 15:
                    code, length = ac[0xF0]
                    acc, nbits = acc << length | code, nbits + length
                    run -= 16
                    if stats is not None:
                        stats["zrl"] = stats.get("zrl", 0) + 1
                v = int(blk[k])
                size = abs(v).bit_length()
                code, length = ac[run << 4 | size]
                acc, nbits = acc << length | code, nbits + length
                acc, nbits = acc << size | ((v if v >= 0 else v - 1) & ((1 << size) - 1)), nbits + size
            if last != 63:
                code, length = ac[0x00]
                acc, nbits = acc << length | code, nbits + length
            elif stats is not None:
                stats["no_eob"] = stats.get("no_eob", 0) + 1
    pad = -nbits % 8
    acc, nbits = acc << pad | ((1 << pad) - 1), nbits + pad
    raw = acc.to_bytes(nbits // 8, "big")
    if stats is not None:
        stats["stuffed"] = stats.get("stuffed", 0) + raw.count(b"\xff")
    return raw.replace(b"\xff", b"\xff\x00")


def restart_of(restart_mcus):
    return DEFAULT_RESTART_MCUS if restart_mcus == 0 else restart_mcus


def scan(coef, restart_mcus, stats=None):
    """the scan data: the intervals with RST(i mod 8) between them"""
    ri = restart_of(restart_mcus)
    parts = [code_interval(coef[i:i + ri], stats) for i in range(0, len(coef), ri)]
    out = bytearray()
    for i, p in enumerate(parts):
        if i:
            out += bytes([0xFF, 0xD0 + (i - 1) % 8])
        out += p
    return bytes(out)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def dqt_segment(index, table):
    return _segment(0xDB, bytes([index]) + bytes(int(v) for v in np.asarray(table)[ZIGZAG]))


def dht_segment(cls, index, spec):
    return _segment(0xC4, bytes([cls << 4 | index]) + bytes(spec[0]) + bytes(spec[1]))


def header(h, w, quality, restart_mcus):
    """SOI through SOS"""
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += dqt_segment(0, ql) + dqt_segment(1, qc)
    out += _segment(0xC0, bytes([8]) + struct.pack(">HH", h, w) + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    out += dht_segment(0, 0, DC_LUMA) + dht_segment(1, 0, AC_LUMA) + dht_segment(0, 1, DC_CHROMA) + dht_segment(1, 1, AC_CHROMA)
    out += _segment(0xDD, struct.pack(">H", restart_of(restart_mcus)))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode_planes(planes, quality, restart_mcus=0, stats=None):
    h, w = np.asarray(planes[0]).shape
    return header(h, w, quality, restart_mcus) + scan(coefficients(planes, quality), restart_mcus, stats) + b"\xff\xd9"


def encode(bgr, quality, restart_mcus=0, stats=None):
    """the whole stream of an [h][w][3] BGR8 picture"""
    return encode_planes(planes_of(bgr), quality, restart_mcus, stats)


HEADER_BYTES = 623 + 6   # every segment has a fixed length: SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 33 + 183 + 33 + 183, DRI 6, SOS 14


def bound(h, w, restart_mcus=0):
    """vp_jpeg_bound: header + EOI + per MCU 6 blocks of at most 22 + 63 * 26 bits (the longest DC code 11 bits + 11, the longest AC code 16 bits + 10; a ZRL or
    an EOB is shorter than the coefficients it stands for), every byte stuffed, + 2 per interval (the marker; the padding stays inside the MCU's whole bytes)"""
    my, mx = mcu_grid(h, w)
    n = my * mx
    ri = restart_of(restart_mcus)
    return HEADER_BYTES + 2 + n * 2 * (6 * (22 + 63 * 26) // 8) + 2 * ((n + ri - 1) // ri)
