"""Shared cases of the colour-standard tests (tests/test_color_host.py on the emulated library, tests/test_gpu_color.py on the MI355X): BT.601 / BT.709,
limited / full range, the I420 / YV12 / NV21 layouts and the mean chroma rule of vp_canvas_fetch.

The oracle is the numpy restatement below of what include/vp_hip.h states as the DEFINITION, parameterised by the standard: 20 fractional bits,
+ 2^19, arithmetic shift, clamp to 0 .. 255.  The constants are written out here as the header writes them; tests/test_color_host.py rederives every one
of them from (Kr, Kb) as rationals (derive() below).  Plane builders follow tests/frame_cases.py: every plane is a view into a larger, randomly filled
parent, so a stride slip shows in the result."""
from fractions import Fraction

import numpy as np

import canvas_cases as cc
import frame_cases as fc

MATRICES = {"bt601": 0, "bt709": 1}
RANGES = {"limited": 0, "full": 1}
STANDARDS = (("bt601", "limited"), ("bt601", "full"), ("bt709", "limited"), ("bt709", "full"))
DEFAULT = STANDARDS[0]
NEW_STANDARDS = STANDARDS[1:]
KR_KB = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}

# (off, CY, CVR, CVG, CUG, CUB):  y = CY * max(0, Y - off);  R = y + CVR v;  G = y - CVG v - CUG u;  B = y + CUB u
INVERSE = {
    ("bt601", "limited"): (16, 1220542, 1673527, 852492, 409993, 2116026),    # OpenCV's constants, not the nearest integers: kept as they are
    ("bt601", "full"): (0, 1048576, 1470104, 748826, 360853, 1858077),
    ("bt709", "limited"): (16, 1220945, 1879825, 558796, 223607, 2215014),
    ("bt709", "full"): (0, 1048576, 1651297, 490864, 196424, 1945738),
}
# (off, (YR, YG, YB), (UR, UG, UB), (VR, VG, VB))
FORWARD = {
    ("bt601", "limited"): (16, (269484, 528482, 102760), (-155188, -305135, 460324), (460324, -385875, -74448)),
    ("bt601", "full"): (0, (313524, 615514, 119538), (-176932, -347356, 524288), (524288, -439026, -85262)),
    ("bt709", "limited"): (16, (191455, 644067, 65019), (-105533, -355018, 460551), (460551, -418321, -42230)),
    ("bt709", "full"): (0, (222927, 749942, 75707), (-120138, -404150, 524288), (524288, -476214, -48074)),
}

PLANAR = ("i420", "yv12")
NEW_FORMATS = ("i420", "yv12", "nv21")
OLD_YUV = fc.YUV
ALL_YUV = OLD_YUV + NEW_FORMATS
SUBSAMPLED_2X2 = ("nv12",) + NEW_FORMATS
CODES = {"i420": 16, "yv12": 17, "nv21": 18}


def std_id(std):
    return f"{std[0]}-{std[1]}"


def nearest(x):
    """the nearest integer to the rational x * 2^20 (no constant of the tables is a tie)"""
    x = Fraction(x) * (1 << 20)
    n = (abs(x) + Fraction(1, 2)).__floor__()
    assert abs(x) + Fraction(1, 2) != n, "a tie"
    return n if x >= 0 else -n


def derive(matrix, rng):
    """(INVERSE entry, FORWARD entry) of a standard from (Kr, Kb): the scales are 255/219 (luma) and 255/224 (chroma) for limited range, 1 for full range;
    UB and VR are minus the sum of the row's other two constants, so grey gives exactly (128, 128)"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    full = rng == "full"
    sy, sc = (Fraction(1), Fraction(1)) if full else (Fraction(255, 219), Fraction(255, 224))
    inv = (0 if full else 16, nearest(sy), nearest(2 * (1 - kr) * sc), nearest(2 * (1 - kr) * kr / kg * sc), nearest(2 * (1 - kb) * kb / kg * sc), nearest(2 * (1 - kb) * sc))
    yrow = tuple(nearest(k / sy) for k in (kr, kg, kb))
    ur, ug = nearest(-kr / (2 * (1 - kb)) / sc), nearest(-kg / (2 * (1 - kb)) / sc)
    vg, vb = nearest(-kg / (2 * (1 - kr)) / sc), nearest(-kb / (2 * (1 - kr)) / sc)
    return inv, (0 if full else 16, yrow, (ur, ug, -(ur + ug)), (-(vg + vb), vg, vb))


# ---- the arithmetic
def yuv_raw(std, Y, U, V):
    """(R, G, B) before the clamp, int64"""
    off, cy, cvr, cvg, cug, cub = INVERSE[std]
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    y = cy * np.maximum(0, Y - off)
    u, v = U - 128, V - 128
    return (y + cvr * v + (1 << 19)) >> 20, (y - cvg * v - cug * u + (1 << 19)) >> 20, (y + cub * u + (1 << 19)) >> 20


def yuv_to_bgr(std, Y, U, V):
    """uint8 [..., 3] in B, G, R order"""
    r, g, b = yuv_raw(std, Y, U, V)
    return np.stack([np.clip(c, 0, 255) for c in (b, g, r)], axis=-1).astype(np.uint8)


def bgr_raw(std, R, G, B):
    """(Y, U, V) before the clamp, int64"""
    off, yk, uk, vk = FORWARD[std]
    R, G, B = (np.asarray(a).astype(np.int64) for a in (R, G, B))
    return tuple((k[0] * R + k[1] * G + k[2] * B + (o << 20) + (1 << 19)) >> 20 for k, o in ((yk, off), (uk, 128), (vk, 128)))


def bgr_to_yuv(std, bgr):
    """uint8 planes Y, U, V (per pixel) of a [..., 3] BGR array"""
    bgr = np.asarray(bgr)
    return tuple(np.clip(c, 0, 255).astype(np.uint8) for c in bgr_raw(std, bgr[..., 2], bgr[..., 1], bgr[..., 0]))


# ---- upload: planes -> BGR8
def plane_rows(fmt, h, w):
    """[(rows, bytes per row)] of the planes of a YUV format"""
    if fmt in PLANAR:
        return [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    if fmt in ("nv12", "nv21"):
        return [(h, w), (h // 2, w)]
    return [(h, 2 * w)]


def random_planes(fmt, h, w, strides, seed):
    """planes of a random frame as views [rows][row bytes] into parents [rows][stride] filled with other random bytes"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(n, st), dtype=np.uint8)[:, :rb] for (n, rb), st in zip(plane_rows(fmt, h, w), strides)]


def chroma_planes(fmt, planes, h, w):
    """(U, V) [h/2][w/2] of a 2x2-subsampled format"""
    if fmt in PLANAR:
        u, v = (np.asarray(p)[:h // 2, :w // 2] for p in planes[1:3])
        return (u, v) if fmt == "i420" else (v, u)
    q = np.asarray(planes[1])[:h // 2, :w].reshape(h // 2, w // 2, 2)
    return (q[:, :, 0], q[:, :, 1]) if fmt == "nv12" else (q[:, :, 1], q[:, :, 0])


def to_bgr(std, fmt, planes, h, w):
    """the BGR8 image [h][w][3] a vp_frame holds after uploading `planes` as `fmt` under `std`: no chroma interpolation"""
    if fmt in SUBSAMPLED_2X2:
        U, V = (c.repeat(2, axis=0).repeat(2, axis=1) for c in chroma_planes(fmt, planes, h, w))
        return yuv_to_bgr(std, np.asarray(planes[0])[:h, :w], U, V)
    q = np.asarray(planes[0])[:h, :2 * w].reshape(h, w // 2, 4)
    yo, co = (0, 1) if fmt == "yuy2" else (1, 0)
    Y = np.stack([q[:, :, yo], q[:, :, yo + 2]], axis=2).reshape(h, w)
    return yuv_to_bgr(std, Y, q[:, :, co].repeat(2, axis=1), q[:, :, co + 2].repeat(2, axis=1))


def table_planes(fmt):
    """frame_cases.table_planes for every YUV format: all 256 Y values across, one row group per (U, V) pair of UV_GRID squared.  (planes, h, w)"""
    if fmt in OLD_YUV:
        return fc.table_planes(fmt)
    (yp, uv), h, w = fc.table_planes("nv12")
    uv = uv.reshape(h // 2, w // 2, 2)
    if fmt == "nv21":
        return [yp, np.ascontiguousarray(uv[:, :, ::-1]).reshape(h // 2, w)], h, w
    u, v = np.ascontiguousarray(uv[:, :, 0]), np.ascontiguousarray(uv[:, :, 1])
    return [yp, u, v] if fmt == "i420" else [yp, v, u], h, w


# (format, h, w, strides): two chroma rows and columns, w % 4 != 0, strides above the row's bytes that differ per plane
NEW_CONVERSION_CASES = (("i420", 4, 6, (8, 5, 4)), ("yv12", 4, 6, (7, 4, 6)), ("nv21", 4, 6, (8, 8)))
OLD_CONVERSION_CASES = tuple(c for c in fc.CONVERSION_CASES if c[0] in OLD_YUV)


# ---- fetch: BGR8 -> planes
def subsample(c, fmt, mode):
    """one chroma plane (per pixel, uint8) -> the stored samples: the even pixel (2x2: the top-left one), or the rounded mean of the group"""
    c = c.astype(np.int64)
    if fmt in SUBSAMPLED_2X2:
        out = c[0::2, 0::2] if mode == "even" else (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    else:
        out = c[:, 0::2] if mode == "even" else (c[:, 0::2] + c[:, 1::2] + 1) >> 1
    return out.astype(np.uint8)


def from_bgr(std, mode, fmt, bgr):
    """the planes vp_canvas_fetch returns for an [h][w][3] BGR picture, rows packed"""
    h, w = bgr.shape[:2]
    Y, U, V = bgr_to_yuv(std, bgr)
    if fmt == "gray8":
        return [Y]
    Us, Vs = subsample(U, fmt, mode), subsample(V, fmt, mode)
    if fmt in PLANAR:
        return [Y, Us, Vs] if fmt == "i420" else [Y, Vs, Us]
    if fmt in ("nv12", "nv21"):
        return [Y, np.stack([Us, Vs] if fmt == "nv12" else [Vs, Us], axis=2).reshape(h // 2, w)]
    q = np.stack([Y[:, 0::2], Us, Y[:, 1::2], Vs] if fmt == "yuy2" else [Us, Y[:, 0::2], Vs, Y[:, 1::2]], axis=2)
    return [q.reshape(h, 2 * w)]


def fetch_picture(fmt, seed=0):
    """random 4 x 6 (YUY2 / UYVY, GRAY8: 3 x 6) with pure blue and pure red in it: in full range their U / V reach 256 before the clamp"""
    h, w = (4, 6) if fmt in SUBSAMPLED_2X2 else (3, 6)
    bgr = cc.random_bgr(h, w, seed)
    bgr[0, 0], bgr[1, 3] = (255, 0, 0), (0, 0, 255)
    return bgr


def layout3(fmt, h, w):
    """[(bytes per row, rows)] of each plane, or None where vp_canvas_layout3 refuses"""
    if fmt in cc.FORMATS:
        return cc.layout(fmt, h, w)
    if fmt not in NEW_FORMATS or not (2 <= h <= 16384 and 2 <= w <= 16384) or h % 2 or w % 2:
        return None
    return [(rb, n) for n, rb in plane_rows(fmt, h, w)]


# ---- checks shared by the two test files: `lib` is autoware_vision_pilot_amd.lib bound to the library under test
def upload_fetch(lib, std, fmt, planes, h, w):
    f = lib.Frame()
    try:
        f.set_color(*std)
        assert f.get_color() == (MATRICES[std[0]], RANGES[std[1]])
        f.upload(planes, fmt, hw=(h, w))
        assert f.hw() == (h, w)
        return f.fetch_bgr8()
    finally:
        f.close()


def check_conversion(lib, std, fmt, h, w, strides, seed=0):
    planes = random_planes(fmt, h, w, strides, seed)
    want = to_bgr(std, fmt, planes, h, w)
    got = upload_fetch(lib, std, fmt, planes, h, w)
    assert got.shape == want.shape
    assert np.array_equal(got, want), (std, fmt, np.argwhere(got != want)[:4])


def check_table(lib, std, fmt):
    planes, h, w = table_planes(fmt)
    want = to_bgr(std, fmt, planes, h, w)
    for c in range(3):   # both clamps of every channel are reached under every standard
        assert want[:, :, c].min() == 0 and want[:, :, c].max() == 255, (std, c)
    got = upload_fetch(lib, std, fmt, planes, h, w)
    assert np.array_equal(got, want), (std, fmt, np.argwhere(got != want)[:4])


def check_flat_upload(lib, fmt):
    """one flat contiguous H*W*3/2 buffer == the planes it consists of"""
    h, w = 4, 6
    flat = np.random.default_rng(11).integers(0, 256, size=h * w * 3 // 2, dtype=np.uint8)
    if fmt in PLANAR:
        planes = [flat[:h * w].reshape(h, w), flat[h * w:h * w * 5 // 4].reshape(h // 2, w // 2), flat[h * w * 5 // 4:].reshape(h // 2, w // 2)]
    else:
        planes = [flat[:h * w].reshape(h, w), flat[h * w:].reshape(h // 2, w)]
    want = to_bgr(DEFAULT, fmt, planes, h, w)
    for buf in (flat, flat.reshape(h * 3 // 2, w)):
        f = lib.Frame()
        try:
            f.upload(buf, fmt, hw=(h, w))
            assert np.array_equal(f.fetch_bgr8(), want), fmt
        finally:
            f.close()


def fetch_planes(lib, std, mode, fmt, bgr, strides=None):
    with cc.OnCanvas(lib, bgr) as oc:
        c = oc.canvas
        assert c.get_color() == (0, 0, 0)
        c.set_color(std[0], std[1], mode)
        assert c.get_color() == (MATRICES[std[0]], RANGES[std[1]], 1 if mode == "mean" else 0)
        got = c.fetch(fmt, strides=strides)
        return list(got) if isinstance(got, tuple) else [got]


def check_fetch(lib, std, fmt, seed=0):
    """both chroma modes, packed and with strides above the row's bytes that differ per plane; the full-range clamp decides; the mean differs from the
    even pixel"""
    bgr = fetch_picture(fmt, seed)
    if std[1] == "full":
        _, u, v = bgr_raw(std, bgr[..., 2], bgr[..., 1], bgr[..., 0])
        assert u.max() == 256 and v.max() == 256      # pure blue / pure red: only the clamp keeps them bytes
    res = {}
    for mode in ("even", "mean"):
        want = from_bgr(std, mode, fmt, bgr)
        for strides in (None, [p.shape[1] + 5 + 2 * i for i, p in enumerate(want)]):
            got = fetch_planes(lib, std, mode, fmt, bgr, strides)
            assert len(got) == len(want)
            for g, x in zip(got, want):
                assert np.array_equal(g.reshape(x.shape), x), (std, mode, fmt, strides, np.argwhere(g.reshape(x.shape) != x)[:4])
        res[mode] = want
    if fmt != "gray8":
        assert any(not np.array_equal(a, b) for a, b in zip(res["even"], res["mean"])), (std, fmt)


LAYOUT_SIZES = ((2, 2), (4, 6), (6, 10), (720, 1280), (16384, 16384), (5, 6), (4, 7), (1, 4), (16386, 4))


def check_layout3(lib):
    for fmt in cc.FORMATS + NEW_FORMATS:
        for h, w in LAYOUT_SIZES:
            want = layout3(fmt, h, w)
            if want is None:
                try:
                    lib.canvas_layout3(fmt, h, w)
                except ValueError:
                    continue
                raise AssertionError((fmt, h, w))
            assert lib.canvas_layout3(fmt, h, w) == want, (fmt, h, w)
            if fmt in PLANAR:     # the two-plane call has no room for them
                try:
                    lib.canvas_layout(fmt, h, w)
                except ValueError:
                    continue
                raise AssertionError((fmt, h, w))
            assert lib.canvas_layout(fmt, h, w) == want, (fmt, h, w)


def exact_colours(std, n):
    """the first n non-grey (Y, U, V) of a coarse grid that the restatement itself takes to BGR and back unchanged, no clamp involved"""
    off = INVERSE[std][0]
    Y, U, V = (a.ravel() for a in np.meshgrid(np.arange(off + 24, 220, 7), np.arange(96, 161, 5), np.arange(96, 161, 5), indexing="ij"))
    r, g, b = yuv_raw(std, Y, U, V)
    y2, u2, v2 = bgr_raw(std, r, g, b)
    ok = (np.minimum(np.minimum(r, g), b) >= 0) & (np.maximum(np.maximum(r, g), b) <= 255) & (y2 == Y) & (u2 == U) & (v2 == V) & ((U != 128) | (V != 128))
    idx = np.flatnonzero(ok)[:: max(1, int(ok.sum()) // n)][:n]
    assert len(idx) == n
    return [(int(Y[i]), int(U[i]), int(V[i])) for i in idx]


def roundtrip_frame(std):
    """I420 6 x 8 in poisoned parents: moderate random chroma (most pixels convert without a clamp); the first two 2x2 groups of each group row hold ONE
    colour each, one that the restatement returns unchanged (exact_colours) -- the last of them grey.  (planes, h, w, mask of the constant groups)"""
    h, w = 6, 8
    planes = random_planes("i420", h, w, (w + 3, w // 2 + 2, w // 2 + 1), 17)
    rng = np.random.default_rng(18)
    planes[0][:] = rng.integers(40, 216, size=(h, w))
    for p in planes[1:]:
        p[:] = rng.integers(100, 157, size=p.shape)
    cols = exact_colours(std, 5) + [(120, 128, 128)]
    const = np.zeros((h // 2, w // 2), bool)
    for i, (y, u, v) in enumerate(cols):
        gy, gx = divmod(i, 2)
        planes[0][2 * gy:2 * gy + 2, 2 * gx:2 * gx + 2] = y
        planes[1][gy, gx], planes[2][gy, gx] = u, v
        const[gy, gx] = True
    return planes, h, w, const


def roundtrip_bound(std):
    """max |Y' - Y| the restatement gives over the byte grid of (Y, U, V) whose RGB stays unclamped: the rounding of two integer conversions"""
    off = INVERSE[std][0]
    Y, U, V = np.meshgrid(np.arange(off, 236 if off else 256), np.arange(0, 256, 3), np.arange(0, 256, 3), indexing="ij")
    r, g, b = yuv_raw(std, Y, U, V)
    ok = (np.minimum(np.minimum(r, g), b) >= 0) & (np.maximum(np.maximum(r, g), b) <= 255)
    return int(np.abs(np.clip(bgr_raw(std, r, g, b)[0], 0, 255) - Y)[ok].max())


def check_roundtrip(lib, std):
    """upload I420, canvas.begin, the same standard on the canvas, fetch as I420.  Y: within the bound the restatement gives on this very frame (computed
    here over the pixels no clamp touches; at most 2 in limited and 1 in full range, as on the byte grid).  Chroma of the constant-colour groups: what went
    in, in both modes (the mean of four equal bytes is that byte)."""
    planes, h, w, const = roundtrip_frame(std)
    bgr = to_bgr(std, "i420", planes, h, w)
    yin, uin, vin = (np.asarray(p).astype(np.int64) for p in planes)
    r, g, b = yuv_raw(std, yin, *(c.repeat(2, axis=0).repeat(2, axis=1) for c in (uin, vin)))
    unclamped = (np.minimum(np.minimum(r, g), b) >= 0) & (np.maximum(np.maximum(r, g), b) <= 255)
    assert unclamped.sum() > h * w // 2
    want = from_bgr(std, "even", "i420", bgr)
    bound = int(np.abs(want[0].astype(np.int64) - yin)[unclamped].max())
    limit = 2 if std[1] == "limited" else 1
    print(f"round trip {std_id(std)}: Y bound on this frame {bound}, on the byte grid {roundtrip_bound(std)}")
    assert bound <= roundtrip_bound(std) <= limit
    for mode in ("even", "mean"):      # the restatement first: the constant groups come back as they went in
        _, uu, vv = from_bgr(std, mode, "i420", bgr)
        assert np.array_equal(uu[const], uin[const]) and np.array_equal(vv[const], vin[const])
    f, c = lib.Frame(), lib.Canvas()
    try:
        f.set_color(*std)
        f.upload(planes, "i420", hw=(h, w))
        c.begin(f)
        for mode in ("even", "mean"):
            c.set_color(std[0], std[1], mode)
            Y, U, V = c.fetch("i420")
            assert int(np.abs(Y.astype(np.int64) - yin)[unclamped].max()) <= bound
            assert np.array_equal(U[const], uin[const]) and np.array_equal(V[const], vin[const])
    finally:
        c.close()
        f.close()


def check_consumer_equals_host(lib, eng, std, fmt, h, w, region, strides, seed=3):
    """frame_cases.check_consumer_equals_host's method under a colour standard: input tensor and logits of infer_frame on `region` of a random `fmt` frame
    == vp_infer on the numpy-converted BGR8 slice passed as a strided view, bit for bit"""
    planes = random_planes(fmt, h, w, strides, seed)
    bgr = np.ascontiguousarray(to_bgr(std, fmt, planes, h, w))
    assert not np.array_equal(bgr, to_bgr(DEFAULT, fmt, planes, h, w))      # the standard matters on this frame
    x0, y0, rw, rh = region
    fc.infer_view(lib, eng, bgr, x0, y0, rw, rh)
    want_in, want = eng.input_tensor().copy(), eng.logits().copy()
    f = lib.Frame()
    try:
        f.set_color(*std)
        f.upload(planes, fmt, hw=(h, w))
        eng.infer_frame(f, region)
        assert eng.frame_hw() == (rh, rw)
        assert np.array_equal(eng.input_tensor(), want_in)
        assert np.array_equal(eng.logits(), want)
    finally:
        f.close()


def check_refusals_and_state(lib):
    import pytest

    z = np.zeros((8, 64), np.uint8)
    f, c = lib.Frame(), lib.Canvas()
    try:
        assert f.get_color() == (0, 0) and c.get_color() == (0, 0, 0)         # the defaults on fresh handles
        for bad in ((2, 0), (-1, 0), (0, 2), (0, -1)):
            with pytest.raises(ValueError, match="unknown"):
                f.set_color(*bad)
        for bad in ((2, 0, 0), (0, 2, 0), (0, 0, 2), (0, 0, -1)):
            with pytest.raises(ValueError, match="unknown"):
                c.set_color(*bad)
        assert f.get_color() == (0, 0) and c.get_color() == (0, 0, 0)         # a refused call changes nothing
        for fmt in NEW_FORMATS:
            n = 3 if fmt in PLANAR else 2
            with pytest.raises(ValueError, match="even width"):
                f.upload([z] * n, fmt, hw=(4, 5))
            with pytest.raises(ValueError, match="even height"):
                f.upload([z] * n, fmt, hw=(5, 6))
            with pytest.raises(ValueError, match="plane"):
                f.upload([z] * (n - 1), fmt, hw=(4, 6))
            with pytest.raises(ValueError, match="plane"):
                f.upload([z] * (n + 1), fmt, hw=(4, 6))
        with pytest.raises(ValueError, match="below the row's"):
            f.upload([z, z, np.zeros((8, 4), np.uint8)], "i420", hw=(4, 10))    # the third plane: 5 bytes a row, stride 4
        with pytest.raises(ValueError, match="below the row's"):
            f.upload([z, np.zeros((8, 8), np.uint8)], "nv21", hw=(4, 10))
        for code in (8, 15, 19, 99):
            with pytest.raises(ValueError, match="unknown format"):
                f.upload(z, code, hw=(4, 6))
        # a setting survives re-upload, and a later setting applies to the next upload only
        f.set_color("bt709", "full")
        for seed in (1, 2):
            planes = random_planes("nv21", 4, 6, (9, 7), seed)
            f.upload(planes, "nv21", hw=(4, 6))
            assert f.get_color() == (1, 1)
            assert np.array_equal(f.fetch_bgr8(), to_bgr(("bt709", "full"), "nv21", planes, 4, 6))
        f.set_color("bt601", "limited")
        assert np.array_equal(f.fetch_bgr8(), to_bgr(("bt709", "full"), "nv21", planes, 4, 6))      # the picture is what the upload made it
        # a canvas does not inherit from the frame; GRAY8 upload and the RGB family are untouched by the settings
        f.set_color("bt709", "limited")
        g = np.random.default_rng(5).integers(0, 256, size=(4, 6), dtype=np.uint8)
        f.upload(g, "gray8")
        assert np.array_equal(f.fetch_bgr8(), np.repeat(g[:, :, None], 3, axis=2))
        bgr = cc.random_bgr(5, 6, 3)
        f.upload(bgr, "bgr8")
        c.begin(f)
        assert c.get_color() == (0, 0, 0)
        assert np.array_equal(c.fetch("yuy2"), cc.from_bgr("yuy2", bgr)[0])
        c.set_color("bt709", "full", "mean")
        assert np.array_equal(c.fetch("rgba8"), cc.from_bgr("rgba8", bgr)[0].reshape(5, 6, 4))
        for fmt in NEW_FORMATS:                                                 # 5 x 6: odd height
            with pytest.raises(ValueError, match="even height"):
                c.fetch(fmt)
        with pytest.raises(ValueError, match="unknown format"):
            c.fetch(8)
        f.upload(cc.random_bgr(4, 6, 4), "bgr8")
        c.begin(f)
        assert c.get_color() == (1, 1, 1)                                        # the setting survives a new picture
        with pytest.raises(ValueError, match="plane"):
            c.fetch("i420", strides=[6, 3])
        with pytest.raises(ValueError, match="below the row's"):
            c.fetch("yv12", strides=[6, 3, 2])
    finally:
        c.close()
        f.close()
