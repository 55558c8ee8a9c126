"""Shared cases of the raw Bayer / P010 / GRAY16 upload tests (tests/test_raw_host.py on the emulated library, tests/test_gpu_raw.py on the MI355X).

The oracle is the numpy restatement below of what include/vp_hip.h states as the DEFINITION of a Bayer upload: linearise, white balance, bilinear
demosaic with mirrored borders, optional Q10 matrix, tone (LUT or rounding shift), all in integers.  P010 and GRAY16 narrow every 16-bit sample to
x8 = min(255, (s + 128) >> 8) and are NV12 / GRAY8 from there (tests/color_cases.py holds that arithmetic).  Plane builders follow
tests/frame_cases.py: every plane is a view into a larger, randomly filled parent, so a stride slip shows in the result."""
import ctypes as C

import numpy as np

import color_cases as kc

ORDERS = ("rggb", "grbg", "gbrg", "bggr")
CODES = {"gray16": 20, "p010": 21}
CODES.update({f"bayer_{o}8": 32 + i for i, o in enumerate(ORDERS)})
CODES.update({f"bayer_{o}16": 36 + i for i, o in enumerate(ORDERS)})
NEW_SYMBOLS = ("vp_frame_set_raw", "vp_frame_get_raw")
DEFAULTS = {"bits": 0, "shift": 0, "black": 0, "gains": (256, 256, 256), "ccm": None, "lut_len": 0}

# 2x2: all border, a single cell.  4x6: more than one cell each way, w % 4 != 0, a row ending inside a store block.  34x66: 17 x 17 blocks = 289
# work-items, more than one 256-wide workgroup.
SHAPES = ((2, 2), (4, 6), (34, 66))


def fmt_of(order, container):
    return f"bayer_{order}{container}"


# ---- the definition
def cfa_colours(order, h, w):
    """[h][w] of 0 (R), 1 (G), 2 (B): the four letters name the cell at (row 0, column 0) in reading order"""
    cell = np.array(["rgb".index(ch) for ch in order]).reshape(2, 2)
    return cell[(np.arange(h) & 1)[:, None], (np.arange(w) & 1)[None, :]]


def mosaic(order, rgb):
    """the raw frame a sensor of that order records of an [h][w][3] R, G, B picture"""
    h, w = rgb.shape[:2]
    return np.take_along_axis(rgb, cfa_colours(order, h, w)[:, :, None], axis=2)[:, :, 0]


def linear_lut(B):
    """the table that gives the bits of the LUT-less tone step: 2^min(B, 12) entries"""
    b = min(B, 12)
    i = np.arange(1 << b)
    return (i if b == 8 else np.minimum(255, (i + (1 << (b - 9))) >> (b - 8))).astype(np.uint8)


def gamma_lut(B):
    n = 1 << min(B, 12)
    return np.round(255.0 * (np.arange(n) / (n - 1.0)) ** (1 / 2.2)).astype(np.uint8)


def raw_to_rgb(order, raw, container, bits=0, shift=0, black=0, gains=(256, 256, 256), ccm=None, hits=None):
    """steps 1 .. 4: (R, G, B) int64 [h][w] at B bits, and B.  hits: a dict that learns which clamps decided something"""
    B = bits or container
    M = (1 << B) - 1
    s = np.asarray(raw).astype(np.int64)
    h, w = s.shape
    col = cfa_colours(order, h, w)
    a = s >> shift
    lin = np.minimum(a, M) - black
    v = np.maximum(0, lin)
    wb = (v * np.asarray(gains, dtype=np.int64)[col] + 128) >> 8
    if hits is not None:
        hits.update(above_M=bool((a > M).any()), below_black=bool((lin < 0).any()), gain_clamp=bool((wb > M).any()))
    v = np.minimum(M, wb)
    p = np.pad(v, 1, mode="reflect")                      # -1 -> 1, n -> n - 2: the edge is not repeated
    c, N, S, W, E = p[1:-1, 1:-1], p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]
    cross = (N + S + W + E + 2) >> 2
    diag = (p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:] + 2) >> 2
    hor, ver = (W + E + 1) >> 1, (N + S + 1) >> 1
    green = col == 1
    red_row = (col == 0).any(axis=1)[:, None]              # the rows that hold the red sites
    R = np.where(col == 0, c, np.where(green, np.where(red_row, hor, ver), diag))
    G = np.where(green, c, cross)
    Bl = np.where(col == 2, c, np.where(green, np.where(red_row, ver, hor), diag))
    if ccm is not None:
        k = np.asarray(ccm, dtype=np.int64).reshape(3, 3)
        pre = [(k[i, 0] * R + k[i, 1] * G + k[i, 2] * Bl + 512) >> 10 for i in range(3)]
        if hits is not None:
            hits.update(ccm_low=bool(min(int(q.min()) for q in pre) < 0), ccm_high=bool(max(int(q.max()) for q in pre) > M))
        R, G, Bl = (np.clip(q, 0, M) for q in pre)
    return (R, G, Bl), B


def raw_to_bgr(order, raw, container, bits=0, shift=0, black=0, gains=(256, 256, 256), ccm=None, lut=None, hits=None):
    """the BGR8 picture [h][w][3] a vp_frame holds after uploading `raw` as bayer_<order><container> under the setting"""
    rgb, B = raw_to_rgb(order, raw, container, bits, shift, black, gains, ccm, hits)
    if lut is not None:
        table = np.asarray(lut, dtype=np.uint8)
        assert table.size == 1 << min(B, 12)
        out = [table[x >> (B - min(B, 12))] for x in rgb]
    elif B == 8:
        out = rgb
    else:
        pre = [(x + (1 << (B - 9))) >> (B - 8) for x in rgb]
        if hits is not None:
            hits.update(tone_clamp=bool(max(int(q.max()) for q in pre) > 255))
        out = [np.minimum(255, q) for q in pre]
    return np.stack([out[2], out[1], out[0]], axis=-1).astype(np.uint8)


def narrow16(a):
    return np.minimum(255, (np.asarray(a).astype(np.int64) + 128) >> 8).astype(np.uint8)


# ---- frames: views into larger random parents
def random_raw(h, w, container, seed, bits=0, shift=0, extra=3):
    """[h][w] view (uint8 or uint16) into an [h][w + extra] parent; samples use bits + shift bits of the container, plus now and then bits above them"""
    rng = np.random.default_rng(seed)
    top = 1 << min(container, (bits or container) + shift)
    dt = np.uint8 if container == 8 else np.uint16
    parent = rng.integers(0, 1 << container, size=(h, w + extra)).astype(dt)
    view = parent[:, :w]
    view[:] = rng.integers(0, top, size=(h, w)).astype(dt)
    if top < (1 << container):                             # a few samples with container bits above B set: min(s >> shift, M) decides
        view[rng.random((h, w)) < 0.1] |= dt(top)
    return view


def random_words(rows, cols, extra, seed):
    return np.random.default_rng(seed).integers(0, 65536, size=(rows, cols + extra)).astype(np.uint16)[:, :cols]


def table_raw(container, B, shift, black):
    """16 x 16: {0, black - 1, black, black + 1, M - 1, M, M + 1 (container bits above B set), the container's maximum}, one value per 2x2 cell in the top
    half so that every value meets every CFA site with other values around it, drawn at random in the bottom half"""
    M = (1 << B) - 1
    top = (1 << container) - 1
    vals = sorted({min(v << shift, top) for v in (0, black - 1, black, black + 1, M - 1, M, M + 1) if v >= 0} | {top})
    vals = np.array(vals, dtype=np.int64)
    y, x = np.mgrid[0:16, 0:16]
    raw = vals[((x >> 1) + 3 * (y >> 1)) % len(vals)]
    raw[8:] = np.random.default_rng(77).choice(vals, size=(8, 16))
    parent = np.full((16, 21), top, dtype=np.uint8 if container == 8 else np.uint16)
    parent[:, :16] = raw
    return parent[:, :16]


CCM = (1434, -307, -103, -205, 1331, -102, 51, -410, 1383)          # rows sum to 1024: grey stays grey
HARSH_CCM = (2253, -819, -410, -717, 2048, -307, -205, -1126, 2355)  # rows sum to 1024; saturated colours leave 0 .. M on both sides
GAINS = (520, 256, 410)


def settings(B):
    """name -> keyword arguments of Frame.set_raw / raw_to_bgr: black, gains, ccm and LUT each alone and all together"""
    black = 1 << (B - 4)
    return {
        "black": {"black": black},
        "gains": {"gains": GAINS},
        "ccm": {"ccm": CCM},
        "lut": {"lut": gamma_lut(B)},
        "all": {"black": black, "gains": GAINS, "ccm": HARSH_CCM, "lut": gamma_lut(B)},
    }


# (id, order, container, setting keywords, (h, w)): four orders x {8-bit container, 16-bit container with bits 10, 12, 16} x the three shapes,
# shift = 4 with bits = 12, and the settings on both containers
def _conversion_cases():
    out = []
    for order in ORDERS:
        for container, bits in ((8, 0), (16, 10), (16, 12), (16, 0)):
            for h, w in SHAPES:
                out.append((f"{order}{container}-b{bits or container}-{h}x{w}", order, container, {"bits": bits}, (h, w)))
    out.append(("grbg16-b12-shift4-4x6", "grbg", 16, {"bits": 12, "shift": 4}, (4, 6)))
    out.append(("bggr16-b12-shift4-34x66", "bggr", 16, {"bits": 12, "shift": 4}, (34, 66)))
    for i, (container, bits) in enumerate(((8, 0), (16, 12))):
        for k, (name, kw) in enumerate(settings(bits or container).items()):
            order = ORDERS[(i + k) % 4]
            out.append((f"{order}{container}-{name}-4x6", order, container, dict(kw, bits=bits), (4, 6)))
    out.append(("gbrg16-b12-all-34x66", "gbrg", 16, dict(settings(12)["all"], bits=12), (34, 66)))
    out.append(("rggb16-b16-lut-4x6", "rggb", 16, {"lut": gamma_lut(16)}, (4, 6)))
    return out


CONVERSION_CASES = _conversion_cases()
TABLE_CASES = (("rggb", 8, 8, 0), ("gbrg", 16, 10, 0), ("grbg", 16, 12, 4), ("bggr", 16, 16, 0))      # (order, container, B, shift)
DEEP_CASES = (("p010", 2, 2, (2, 3)), ("p010", 4, 6, (1, 5)), ("p010", 34, 66, (7, 2)), ("gray16", 3, 5, (2,)), ("gray16", 33, 67, (5,)))   # extras in words


# ---- checks shared by the two test files: `lib` is autoware_vision_pilot_amd.lib bound to the library under test
def upload_fetch(lib, fmt, planes, setting=None, hw=None):
    f = lib.Frame()
    try:
        if setting is not None:
            f.set_raw(**setting)
        f.upload(planes, fmt, hw=hw)
        return f.fetch_bgr8()
    finally:
        f.close()


def check_conversion(lib, order, container, kw, hw, seed=0):
    h, w = hw
    raw = random_raw(h, w, container, seed, kw.get("bits", 0), kw.get("shift", 0))
    want = raw_to_bgr(order, raw, container, **kw)
    got = upload_fetch(lib, fmt_of(order, container), raw, kw)
    assert got.shape == want.shape
    assert np.array_equal(got, want), (order, container, kw, np.argwhere(got != want)[:4])


def check_table(lib, order, container, B, shift):
    black = 1 << (B - 4)
    raw = table_raw(container, B, shift, black)
    kw = {"bits": 0 if B == container else B, "shift": shift, "black": black, "gains": GAINS, "ccm": HARSH_CCM}
    hits = {}
    want = raw_to_bgr(order, raw, container, hits=hits, **kw)
    need = {"below_black", "gain_clamp", "ccm_low", "ccm_high"} | ({"above_M"} if B + shift < container else set())     # a full container has no bits above B
    assert all(hits[k] for k in need), hits                # the table does what it is for
    if B > 8:
        plain = {}
        raw_to_bgr(order, raw, container, hits=plain, bits=kw["bits"], shift=shift)
        assert plain["tone_clamp"], plain                  # M rounds to 256 without a LUT: min(255, .) decides
    for setting in (kw, {"bits": kw["bits"], "shift": shift}, dict(kw, lut=gamma_lut(B))):
        want = raw_to_bgr(order, raw, container, **setting)
        got = upload_fetch(lib, fmt_of(order, container), raw, setting)
        assert np.array_equal(got, want), (order, container, B, sorted(setting), np.argwhere(got != want)[:4])


def deep_planes(fmt, h, w, extras, seed):
    if fmt == "p010":
        return [random_words(h, w, extras[0], seed), random_words(h // 2, w, extras[1], seed + 1)]
    return [random_words(h, w, extras[0], seed)]


def deep_to_bgr(std, fmt, planes, h, w):
    if fmt == "p010":
        return kc.to_bgr(std, "nv12", [narrow16(p) for p in planes], h, w)
    return np.repeat(narrow16(planes[0])[:, :, None], 3, axis=2)


def check_deep(lib, fmt, h, w, extras, seed=0):
    """P010 under every colour standard == the restatement == an NV12 upload of the narrowed planes; GRAY16 == GRAY8 of the narrowed plane"""
    planes = deep_planes(fmt, h, w, extras, seed)
    if fmt == "p010":                                      # the rounding of the narrowing decides somewhere, and so does its clamp
        planes[0][0, 0], planes[0][0, 1], planes[1][0, 0] = 0xFF80, 0x807F, 0xFFFF
    narrowed = [narrow16(p) for p in planes]
    f, g = lib.Frame(), lib.Frame()
    try:
        f.set_raw(bits=12, black=100, gains=(300, 300, 300))           # the raw setting touches no other format
        for std in kc.STANDARDS if fmt == "p010" else (kc.DEFAULT,):
            want = deep_to_bgr(std, fmt, planes, h, w)
            for fr in (f, g):
                fr.set_color(*std)
            f.upload(planes, fmt)
            assert f.hw() == (h, w)
            got = f.fetch_bgr8()
            assert np.array_equal(got, want), (fmt, std, np.argwhere(got != want)[:4])
            g.upload(narrowed, "nv12" if fmt == "p010" else "gray8", hw=(h, w))
            assert np.array_equal(g.fetch_bgr8(), got), (fmt, std)
    finally:
        f.close()
        g.close()


def fetch_padded(lib, f, h, w):
    """vp_frame_fetch_bgr8 into rows of 12 * ceil(w / 4) + 8 bytes pre-filled with 0xA5: the call writes 3 w bytes a row and nothing else"""
    pitch = 12 * ((w + 3) // 4) + 8
    buf = np.full((h, pitch), 0xA5, np.uint8)
    f._ck(f._lib.vp_frame_fetch_bgr8(f._h, buf.ctypes.data_as(C.c_void_p), pitch))
    return buf


def check_row_ends_inside_a_store_block(lib):
    """8 -> 6 -> 6 -> 5 pixels a row into ONE frame, so the picture buffer is reused: a row that ends inside its last store block holds its own pixels
    and no stale one, and the fetch writes the row's bytes only.  (check_zeros_behind_a_row_end looks at the bytes of the pitch behind the row.)"""
    f = lib.Frame()
    try:
        for fmt, planes, kw, h, w in (("bayer_rggb16", random_raw(4, 8, 16, 3), {"bits": 0}, 4, 8), ("bayer_rggb16", random_raw(4, 6, 16, 4), {"bits": 0}, 4, 6),
                                      ("p010", deep_planes("p010", 4, 6, (1, 1), 5), None, 4, 6), ("gray16", deep_planes("gray16", 4, 5, (1,), 6), None, 4, 5)):
            if kw is not None:
                f.set_raw(**kw)
            f.upload(planes, fmt)
            buf = fetch_padded(lib, f, h, w)
            want = raw_to_bgr("rggb", planes, 16) if kw is not None else deep_to_bgr(kc.DEFAULT, fmt, planes, h, w)
            assert np.array_equal(buf[:, :3 * w].reshape(h, w, 3), want), fmt
            assert (buf[:, 3 * w:] == 0xA5).all(), fmt
    finally:
        f.close()


def picture_with_pitch(lib, f, c, read):
    """the frame's whole BGR8 picture, [h][pitch] bytes: vp_canvas_begin copies h * pitch bytes of it and vp_canvas_device hands out pointer and pitch.
    read(pointer, n) -> n bytes at that address (host memory under the emulation, device memory on the GPU)"""
    c.begin(f)
    c.sync()
    ptr, pitch = c.device()
    h, w = c.hw()
    assert (h, w) == f.hw() and pitch == 12 * ((w + 3) // 4)
    return np.frombuffer(read(ptr, h * pitch), np.uint8).reshape(h, pitch)


def check_zeros_behind_a_row_end(lib, read):
    """Pixels beyond the row's end inside the last store block are zero bytes: the canvas kernels keep the bytes 3 w .. pitch of a row as they read them,
    so both new kernels have to store zeros there.  Into ONE frame, so the same bytes are written again: before each narrow upload an 8-pixel row of 255s
    (pitch 24, no byte to spare), then 6 pixels a row of Bayer (8- and 16-bit containers) and of P010 and 5 of GRAY16: bytes 3 w .. 24 of every row are 0."""
    full = np.full((4, 8, 3), 255, np.uint8)
    cases = [(fmt_of(o, cont), [random_raw(4, 6, cont, 20 + i, extra=2)], 4, 6) for i, (o, cont) in enumerate((("rggb", 8), ("gbrg", 16), ("bggr", 16)))]
    cases += [("p010", deep_planes("p010", 4, 6, (1, 1), 25), 4, 6), ("gray16", deep_planes("gray16", 4, 5, (1,), 26), 4, 5),
              ("gray16", deep_planes("gray16", 3, 7, (1,), 27), 3, 7)]
    f, c = lib.Frame(), lib.Canvas()
    try:
        for fmt, planes, h, w in cases:
            f.upload(full, "bgr8")
            assert (picture_with_pitch(lib, f, c, read) == 255).all()                  # every byte of the pitch holds something to clear
            f.upload(planes, fmt)
            got = picture_with_pitch(lib, f, c, read)
            assert got.shape == (h, 24)
            want = raw_to_bgr(fmt[6:10], planes[0], int(fmt[10:])) if fmt.startswith("bayer") else deep_to_bgr(kc.DEFAULT, fmt, planes, h, w)
            assert np.array_equal(got[:, :3 * w].reshape(h, w, 3), want), fmt
            assert (got[:, 3 * w:] == 0).all(), (fmt, got[:, 3 * w:])
    finally:
        c.close()
        f.close()


def set_raw_null(lib, f):
    return f._lib.vp_frame_set_raw(f._h, None)


def check_setting_applies_to_later_uploads(lib):
    raw = random_raw(4, 6, 16, 9, bits=12)
    f = lib.Frame()
    try:
        assert f.get_raw() == DEFAULTS
        kw = {"bits": 12, "shift": 0, "black": 200, "gains": GAINS, "ccm": CCM, "lut": gamma_lut(12)}
        f.set_raw(**kw)
        assert f.get_raw() == {"bits": 12, "shift": 0, "black": 200, "gains": GAINS, "ccm": CCM, "lut_len": 4096}
        r = lib.Raw()
        assert f._lib.vp_frame_get_raw(f._h, C.byref(r)) == 0 and r.lut is None and r.lut_len == 4096      # the table itself stays inside
        f.upload(raw, "bayer_grbg16")
        first = f.fetch_bgr8()
        assert np.array_equal(first, raw_to_bgr("grbg", raw, 16, **kw))
        f.set_raw(bits=12)                                              # a later setting: the resident picture keeps its bits
        assert np.array_equal(f.fetch_bgr8(), first)
        f.upload(raw, "bayer_grbg16")
        second = f.fetch_bgr8()
        assert np.array_equal(second, raw_to_bgr("grbg", raw, 16, bits=12)) and not np.array_equal(second, first)
        f.set_raw(**kw)
        assert set_raw_null(lib, f) == 0 and f.get_raw() == DEFAULTS    # NULL: the defaults
        f.upload(raw, "bayer_grbg16")
        assert np.array_equal(f.fetch_bgr8(), raw_to_bgr("grbg", raw, 16))
        # the identity matrix and the linear table are the defaults, bit for bit
        f.set_raw(bits=12, ccm=(1024, 0, 0, 0, 1024, 0, 0, 0, 1024), lut=linear_lut(12))
        f.upload(raw, "bayer_grbg16")
        assert np.array_equal(f.fetch_bgr8(), second)
    finally:
        f.close()


def check_refusals(lib):
    """every refusal of the upload and of the setting, with its text; a refused call leaves the previous picture and setting"""
    import pytest

    z8, z16 = np.zeros((8, 64), np.uint8), np.zeros((8, 64), np.uint16)
    raw = random_raw(4, 6, 16, 12, bits=12)
    f = lib.Frame()
    try:
        kept = {"bits": 12, "black": 64, "gains": GAINS}
        f.set_raw(**kept)
        setting = f.get_raw()
        f.upload(raw, "bayer_bggr16")
        picture = f.fetch_bgr8()
        assert np.array_equal(picture, raw_to_bgr("bggr", raw, 16, **kept))

        def unchanged():
            assert f.get_raw() == setting and f.hw() == (4, 6) and np.array_equal(f.fetch_bgr8(), picture)

        # -- the upload
        for fmt in [k for k in CODES if k != "gray16"]:
            z = z8 if fmt.endswith("8") else z16
            planes = [z, z] if fmt == "p010" else [z]
            with pytest.raises(ValueError, match="even width"):
                f.upload(planes, fmt, hw=(4, 5))
            with pytest.raises(ValueError, match="even height"):
                f.upload(planes, fmt, hw=(5, 6))
        for fmt in CODES:
            z = z8 if fmt.endswith("8") else z16
            n = 2 if fmt == "p010" else 1
            for hw in ((1, 6), (4, 1), (0, 0)):
                with pytest.raises(ValueError, match="frame size"):
                    f.upload([z] * n, fmt, hw=hw)
            for m in (n - 1, n + 1):
                with pytest.raises(ValueError, match=r"plane\(s\), got n_planes"):
                    f.upload_device([z.ctypes.data] * m, [z.strides[0]] * m, fmt, 4, 6)
            with pytest.raises(ValueError, match="below the row's"):
                f.upload([z] * n, fmt, hw=(4, 66))                       # 66 samples a row, 64 in the array
        with pytest.raises(ValueError, match="below the row's"):
            f.upload([z16, np.zeros((8, 8), np.uint16)], "p010", hw=(4, 10))   # the U V plane: 20 bytes a row, stride 16
        words = np.zeros((8, 129), np.uint8)
        for fmt in ("gray16", "p010", "bayer_rggb16"):
            n = 2 if fmt == "p010" else 1
            with pytest.raises(ValueError, match="is odd"):              # 129 bytes a row
                f.upload([words[:, :128]] * n, fmt, hw=(4, 6))
            with pytest.raises(ValueError, match="odd address"):
                f.upload_device([words.ctypes.data + 1] * n, [128] * n, fmt, 4, 6)
        unchanged()                                                      # (8-bit containers take any stride and address: the conversion cases)
        # -- a setting that does not fit the format: B is only known at the upload
        f.set_raw(bits=8)
        with pytest.raises(ValueError, match="bits = 8 does not fit BAYER_RGGB16"):
            f.upload(z16, "bayer_rggb16", hw=(4, 6))
        f.set_raw(bits=10)
        with pytest.raises(ValueError, match="bits = 10 does not fit BAYER_GBRG8"):
            f.upload(z8, "bayer_gbrg8", hw=(4, 6))
        f.set_raw(bits=10, black=1024)
        with pytest.raises(ValueError, match="black = 1024 is above"):
            f.upload(z16, "bayer_rggb16", hw=(4, 6))
        f.set_raw(black=256)
        with pytest.raises(ValueError, match="black = 256 is above"):
            f.upload(z8, "bayer_rggb8", hw=(4, 6))
        f.set_raw(bits=10, lut=gamma_lut(12))
        with pytest.raises(ValueError, match="LUT has 4096 entries"):
            f.upload(z16, "bayer_rggb16", hw=(4, 6))
        f.set_raw(lut=gamma_lut(10))
        with pytest.raises(ValueError, match="LUT has 1024 entries"):
            f.upload(z8, "bayer_rggb8", hw=(4, 6))
        f.upload(z16, "gray16", hw=(4, 6))                               # ... and touches no other format
        f.upload([z16, z16], "p010", hw=(4, 6))
        f.set_raw(**kept)
        f.upload(raw, "bayer_bggr16")
        unchanged()
        # -- the setting
        for bad, text in (({"bits": 9}, "bits = 9"), ({"bits": -1}, "bits = -1"), ({"bits": 18}, "bits = 18"), ({"shift": -1}, "shift = -1"), ({"shift": 9}, "shift = 9"),
                          ({"black": -1}, "black = -1"), ({"gains": (256, -1, 256)}, "gain -1"), ({"gains": (16384, 256, 256)}, "gain 16384"),
                          ({"ccm": (1024, 0, 0, 0, 8192, 0, 0, 0, 1024)}, "ccm entry 8192"), ({"ccm": (1024, 0, -8192, 0, 1024, 0, 0, 0, 1024)}, "ccm entry -8192"),
                          ({"lut": np.zeros(0, np.uint8)}, "go together"), ({"lut": np.zeros(512, np.uint8)}, "lut_len = 512"), ({"lut": np.zeros(8192, np.uint8)}, "lut_len = 8192")):
            with pytest.raises(ValueError, match=text):
                f.set_raw(**bad)
        r = lib.Raw()
        r.gains[:] = [256, 256, 256]
        r.lut_len = 256                                                   # a length without a table
        assert f._lib.vp_frame_set_raw(f._h, C.byref(r)) == -1 and b"go together" in f._lib.vp_frame_last_error(f._h)
        r.lut_len = 0
        r.ccm[4] = 99999                                                  # read only with ccm_on
        assert f._lib.vp_frame_set_raw(f._h, C.byref(r)) == 0 and f.get_raw() == DEFAULTS
        assert f._lib.vp_frame_get_raw(f._h, None) == -1 and f._lib.vp_frame_set_raw(None, None) == -1
        f.set_raw(gains=(0, 16383, 256), ccm=(8191, -8191, 0, 0, 1024, 0, 0, 0, 1024), shift=8, bits=16)    # the limits themselves are accepted
        f.set_raw(**kept)
        unchanged()
        # -- the old codes stay what they were
        for code in (8, 15, 19, 22, 31, 40, 99):
            with pytest.raises(ValueError, match="unknown format"):
                f.upload(z8, code, hw=(4, 6))
        unchanged()
    finally:
        f.close()


def check_canvas_refuses(lib):
    """the new codes are upload-only: vp_canvas_fetch*, vp_canvas_layout and vp_canvas_layout3 answer VP_ERR_ARG"""
    import pytest

    f, c = lib.Frame(), lib.Canvas()
    try:
        f.upload(random_raw(4, 6, 8, 2), "bayer_rggb8")
        c.begin(f)                                                        # a raw-uploaded frame is a picture like any other
        assert np.array_equal(c.fetch("bgr8"), f.fetch_bgr8())
        for fmt in CODES:
            with pytest.raises(ValueError, match="unknown format"):
                c.fetch(fmt)
            with pytest.raises(ValueError, match="unknown format"):
                c.fetch(fmt, size=(4, 6))
            with pytest.raises(ValueError):
                lib.canvas_layout(fmt, 4, 6)
            with pytest.raises(ValueError):
                lib.canvas_layout3(fmt, 4, 6)
    finally:
        c.close()
        f.close()


def check_rectification_composes(lib):
    """the conversion writes where the rectification passes read: a 34x66 RGGB12 upload under rectify_cases' barrel setting == the BGR8 upload of the
    oracle's picture under the same setting"""
    import rectify_cases as rq

    kw = {"bits": 12, "gains": GAINS}
    raw = random_raw(34, 66, 16, 21, bits=12)
    K = rq.k_matrix(52.0, 51.0, 33.2, 16.7)
    f, g = lib.Frame(), lib.Frame()
    try:
        for fr in (f, g):
            fr.set_rectify(K, rq.BARREL, np.eye(3), (34, 66))
        f.set_raw(**kw)
        f.upload(raw, "bayer_rggb16")
        g.upload(raw_to_bgr("rggb", raw, 16, **kw), "bgr8")
        got = f.fetch_bgr8()
        assert np.array_equal(got, g.fetch_bgr8())
        assert not np.array_equal(got, raw_to_bgr("rggb", raw, 16, **kw))      # the setting did something
    finally:
        f.close()
        g.close()


def check_consumer_equals_host(lib, eng, order="grbg", hw=(48, 64), region=(5, 7, 41, 29), seed=3):
    """input tensor and logits of infer_frame on `region` of a bayer_<order>16 frame == vp_infer on the same region of fetch_bgr8(), bit for bit"""
    import frame_cases as fc

    kw = {"bits": 12, "black": 64, "gains": GAINS}
    raw = random_raw(hw[0], hw[1], 16, seed, bits=12)
    f = lib.Frame()
    try:
        f.set_raw(**kw)
        f.upload(raw, fmt_of(order, 16))
        bgr = np.ascontiguousarray(f.fetch_bgr8())
        assert np.array_equal(bgr, raw_to_bgr(order, raw, 16, **kw))
        x0, y0, rw, rh = region
        fc.infer_view(lib, eng, bgr, x0, y0, rw, rh)
        want_in, want = eng.input_tensor().copy(), eng.logits().copy()
        eng.infer_frame(f, region)
        assert eng.frame_hw() == (rh, rw)
        assert np.array_equal(eng.input_tensor(), want_in)
        assert np.array_equal(eng.logits(), want)
    finally:
        f.close()
