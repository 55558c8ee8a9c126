"""Shared cases of the production-display tests (tests/test_display_host.py on the emulated library, tests/test_gpu_display.py on the MI355X): the additive
lane overlay, the points and lane rows, and the resized fetch of vp_canvas.

Numpy restatements of the rules include/vp_hip.h states, written from those rules: the nearest tables are oracle.pre_post.nearest_index, the resize is
oracle.pre_post.resize_bilinear_u8, the formats are canvas_cases.from_bgr (color_cases.from_bgr where a chroma rule or a planar format is asked for).
Every comparison is equality of bytes.  The case tables hold the smallest shapes at which the kernels' indexing can still go wrong: four-pixel blocks (widths
that are no multiple of four, odd region origins and sizes, the last row and column), both chunks of a 65-point list, discs across every edge, and one
64 x 300 canvas that takes each kernel over more than one workgroup."""
import numpy as np

import canvas_cases as cc
import color_cases as col
from oracle import pre_post

# drawRawMasksInPlace's colours (BGR) in the plane order of the EgoLanes logits -- ego left, ego right, other lanes -- and what addWeighted(.., 1.0, .., 0.4)
# adds to a byte under each
LANE_COLOURS = ((255, 0, 0), (255, 0, 200), (0, 153, 0))
LANE_ADD = ((102, 0, 0), (102, 0, 80), (0, 61, 0))
ROW_COLOUR, ROW_RADIUS = (0, 255, 0), 3


# ---- additive planes
def addweighted_1_04(d, colour, fused):
    """cv::addWeighted(image, 1.0, overlay, 0.4, 0) on u8 before rounding, float32: image * alpha + overlay * beta with every product and the sum rounded
    to float32 (unfused), or fma(overlay, beta, fl(image * alpha)) (fused; evaluated in float64, where product and sum are exact)"""
    a, b = np.float32(1.0), np.float32(0.4)
    d, c = np.asarray(d, np.float32), np.asarray(colour, np.float32)
    fa = (d * a).astype(np.float32)
    return (c.astype(np.float64) * np.float64(b) + fa.astype(np.float64)).astype(np.float32) if fused else (fa + (c * b).astype(np.float32)).astype(np.float32)


def planes_on(planes, threshold, region):
    """[n][h][w] bool: plane k is on at the region's pixel (NaN is never on)"""
    _, _, w, h = region
    n, mh, mw = planes.shape
    yi, xi = pre_post.nearest_index(mh, h), pre_post.nearest_index(mw, w)
    with np.errstate(invalid="ignore"):
        return planes.astype(np.float32)[:, yi][:, :, xi] > np.float32(threshold)


def add_planes(canvas, planes, threshold, add_bgr, region):
    """vp_canvas_add_planes_f32: one clamped sum per pixel"""
    x0, y0, w, h = region
    on = planes_on(planes, threshold, region)
    s = (on[..., None].astype(np.int64) * np.asarray(add_bgr, np.int64).reshape(-1, 1, 1, 3)).sum(axis=0)
    out = canvas.copy()
    out[y0:y0 + h, x0:x0 + w] = np.minimum(255, canvas[y0:y0 + h, x0:x0 + w].astype(np.int64) + s).astype(np.uint8)
    return out


def add_planes_sequential(canvas, planes, threshold, add_bgr, region, order):
    """the reference's way: one saturating overlay after the other, in `order`"""
    x0, y0, w, h = region
    on = planes_on(planes, threshold, region)
    out = canvas.copy()
    for k in order:
        r = out[y0:y0 + h, x0:x0 + w].astype(np.int64)
        out[y0:y0 + h, x0:x0 + w] = np.where(on[k][..., None], np.minimum(255, r + np.asarray(add_bgr[k], np.int64)), r).astype(np.uint8)
    return out


def overlay_lanes(canvas, logits, threshold, region):
    """vp_canvas_overlay_lanes on the logits vp_logits returns ([1][3][80][160] or [3][80][160])"""
    return add_planes(canvas, np.asarray(logits, np.float32).reshape(3, 80, 160), threshold, LANE_ADD, region)


SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.25, np.nextafter(np.float32(0.25), np.float32(1)), np.nextafter(np.float32(0.25), np.float32(0)), -3.0, 7.5], np.float32)
THRESHOLD = 0.25   # sits in the planes itself: `>` is strict


def random_planes(n, mh, mw, seed):
    """normal values with the threshold itself, its two neighbours, NaN and both infinities strewn in (all of them present when there is room)"""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((n, mh, mw)).astype(np.float32)
    flat = p.reshape(-1)
    k = min(len(flat), 3 * len(SPECIALS))
    flat[rng.choice(len(flat), size=k, replace=False)] = np.resize(SPECIALS, k)
    return p


def random_add(n, seed):
    """increments 0 .. 255, the first plane's large enough to clamp"""
    a = np.random.default_rng(seed).integers(0, 256, size=(n, 3), dtype=np.uint8)
    a[0] = (255, 200, 1)
    return a


# ((h, w) of the canvas, (n, mh, mw) of the planes, region (x0, y0, w, h))
ADD_CASES = (
    ((2, 2), (1, 1, 1), (0, 0, 2, 2)),          # the smallest canvas, whole, one 1 x 1 plane
    ((7, 5), (3, 3, 5), (1, 1, 3, 5)),          # odd origin, odd size, across a block boundary
    ((7, 5), (4, 1, 1), (3, 4, 2, 3)),          # the last rows and columns, a row that ends inside a block
    ((7, 5), (1, 80, 160), (0, 0, 5, 7)),       # whole, a plane far larger than the region
    ((11, 14), (3, 80, 160), (3, 1, 9, 7)),     # the lane planes down to a 7 x 9 (h x w) region
    ((11, 14), (4, 3, 5), (1, 3, 13, 7)),       # four planes up to a region that ends in the last column
    ((11, 14), (3, 3, 5), (0, 0, 14, 11)),      # whole, width no multiple of 4
    ((9, 13), (3, 3, 5), (5, 3, 7, 5)),         # odd everything
    ((9, 13), (4, 80, 160), (1, 1, 11, 7)),
    ((9, 13), (1, 1, 1), (11, 7, 2, 2)),        # 2 x 2 in the corner
    ((9, 13), (3, 1, 1), (0, 0, 13, 9)),        # whole, odd width
)
ADD_IDS = ["%dx%d-%dx%dx%d-%d.%d.%d.%d" % (c[0] + c[1] + c[2]) for c in ADD_CASES]
BIG = (64, 300)   # one canvas on which every kernel runs on more than one workgroup


def check_add(lib, hw, shape, region, seed=0, device_pointer=None):
    """host planes; twice, so that the second overlay reads what the first wrote.  device_pointer(array) -> (pointer, keep-alive): also from device memory"""
    bgr, planes, add = cc.random_bgr(*hw, seed), random_planes(*shape, seed + 1), random_add(shape[0], seed + 2)
    want = add_planes(bgr, planes, THRESHOLD, add, region)
    with cc.OnCanvas(lib, bgr) as oc:
        c = oc.canvas
        c.add_planes(planes, THRESHOLD, add, region)
        got = c.fetch("bgr8")
        assert np.array_equal(got, want), np.argwhere(got != want)[:4]
        c.add_planes(planes[::-1].copy(), -THRESHOLD, add, region)
        assert np.array_equal(c.fetch("bgr8"), add_planes(want, planes[::-1], -THRESHOLD, add, region))
        if device_pointer is not None:
            ptr, keep = device_pointer(planes)
            c.begin(oc.frame)
            c.add_planes(ptr, THRESHOLD, add, region, device_shape=planes.shape)
            assert np.array_equal(c.fetch("bgr8"), want)
            del keep


# ---- points
def disc(radius):
    """the (dx, dy) of a disc: dx * dx + dy * dy <= radius * radius"""
    return {(dx, dy) for dx in range(-radius, radius + 1) for dy in range(-radius, radius + 1) if dx * dx + dy * dy <= radius * radius}


def draw_points(canvas, xy, radius, bgr):
    """vp_canvas_draw_points: every disc set to the colour, clipped to the canvas"""
    out = canvas.copy()
    H, W = out.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    for x, y in np.asarray(xy, np.int64).reshape(-1, 2):
        dx, dy = np.clip(xx - x, -radius - 1, radius + 1), np.clip(yy - y, -radius - 1, radius + 1)   # far points: the squares stay small
        out[dx * dx + dy * dy <= radius * radius] = np.asarray(bgr, np.uint8)
    return out


def lane_row_points(logits, origin):
    """the (x, y) vp_canvas_draw_lane_rows draws for the logits vp_logits returns ([1][2][64][1]): fp32 product, truncation, integer division"""
    xp, hv = np.asarray(logits, np.float32).reshape(2, 64)
    pts = []
    for i in range(64):
        v = np.float32(xp[i]) * np.float32(1024.0)
        if hv[i] >= np.float32(0.5) and -1e8 < v < 1e8:
            pts.append((origin[0] + int(v), origin[1] + i * 511 // 63))
    return pts


def draw_lane_rows(canvas, logits, origin):
    return draw_points(canvas, lane_row_points(logits, origin), ROW_RADIUS, ROW_COLOUR)


def point_cases(h, w):
    """{name: xy} on an h x w canvas: every corner, across every edge, overlapping, outside, none, one, two chunks"""
    far = 2 ** 31 - 1
    many = [((i * 7) % (w + 8) - 4, (i * 5) % (h + 8) - 4) for i in range(65)]
    return {
        "none": [],
        "one": [(w // 2, h // 2)],
        "corners": [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)],
        "edges": [(-1, h // 2), (w, h // 2), (w // 2, -2), (w // 2, h + 1), (-3, -3), (w + 2, h + 2)],
        "overlap": [(w // 2, h // 2), (w // 2 + 1, h // 2), (w // 2, h // 2 + 2), (w // 2, h // 2)],
        "outside": [(-17, 0), (w + 16, h // 2), (0, -17), (0, h + 16), (far, far), (-far - 1, -far - 1), (far, 0), (0, -far - 1)],
        "two-chunks": many,
    }


RADII = (0, 3, 16)
POINT_COLOUR = (7, 201, 90)


def check_points(lib, hw, seed=0):
    bgr = cc.random_bgr(*hw, seed)
    with cc.OnCanvas(lib, bgr) as oc:
        c = oc.canvas
        for radius in RADII:
            for name, xy in point_cases(*hw).items():
                c.begin(oc.frame)      # a fresh picture for every case
                c.draw_points(np.array(xy, np.int64).reshape(-1, 2).astype(np.int32), radius, POINT_COLOUR)
                got, want = c.fetch("bgr8"), draw_points(bgr, xy, radius, POINT_COLOUR)
                assert np.array_equal(got, want), (radius, name, np.argwhere(got != want)[:4])
                if name in ("outside", "none"):
                    assert np.array_equal(got, bgr)


# ---- resized fetch
def resized(bgr, size):
    return pre_post.resize_bilinear_u8(bgr, size[0], size[1])


# ((h, w) of the canvas, (out_h, out_w))
RESIZE_CASES = (((7, 5), (3, 2)), ((7, 5), (14, 10)), ((9, 13), (20, 9)), ((11, 14), (11, 14)), ((9, 13), (1, 1)))
RESIZE_FORMATS = ("bgr8", "rgba8")
EVEN_TARGETS = (((7, 5), (14, 10)), ((9, 13), (6, 4)), ((11, 14), (2, 2)))
YUV_FORMATS = ("nv12", "i420", "yuy2")
CHROMA_MODES = ("even", "mean")


def as_list(planes):
    return list(planes) if isinstance(planes, tuple) else [planes]


def check_planes(got, want, what):
    got = as_list(got)
    assert len(got) == len(want), what
    for g, x in zip(got, want):
        assert g.size == x.size and np.array_equal(g.reshape(x.shape), x), (what, np.argwhere(g.reshape(x.shape) != x)[:4])


def check_resize(lib, hw, size, seed=0):
    """BGR8 and RGBA8, packed and with strides above the row's bytes; the canvas keeps its picture; the canvas's own size gives vp_canvas_fetch's bytes"""
    for bgr in (cc.random_bgr(*hw, seed), cc.corner_bgr(*hw)):
        small = resized(bgr, size)
        with cc.OnCanvas(lib, bgr) as oc:
            c = oc.canvas
            for fmt in RESIZE_FORMATS:
                want = cc.from_bgr(fmt, small)
                check_planes(c.fetch(fmt, size=size), want, (fmt, hw, size))
                check_planes(c.fetch(fmt, size=size, strides=[want[0].shape[1] + 7]), want, (fmt, hw, size, "strided"))
                if size == hw:
                    check_planes(c.fetch(fmt, size=size), as_list(c.fetch(fmt)), (fmt, hw, "identity"))
            assert np.array_equal(c.fetch("bgr8"), bgr)       # the canvas itself is unchanged ...
            c.draw_points([(1, 1)], 0, POINT_COLOUR)           # ... and a later draw and resize see the full-size picture
            check_planes(c.fetch("bgr8", size=size), cc.from_bgr("bgr8", resized(draw_points(bgr, [(1, 1)], 0, POINT_COLOUR), size)), (hw, size, "after a draw"))


def check_resize_yuv(lib, hw, size, fmt, mode, seed=0):
    bgr = cc.random_bgr(*hw, seed)
    want = col.from_bgr(col.DEFAULT, mode, fmt, resized(bgr, size))
    with cc.OnCanvas(lib, bgr) as oc:
        oc.canvas.set_color("bt601", "limited", mode)
        check_planes(oc.canvas.fetch(fmt, size=size), want, (fmt, mode, hw, size))
        if mode == "even" and fmt in cc.FORMATS:
            check_planes(oc.canvas.fetch(fmt, size=size), cc.from_bgr(fmt, resized(bgr, size)), (fmt, hw, size))


def check_big(lib, seed=9, device_pointer=None):
    """one 64 x 300 canvas: each kernel on more than one workgroup, the draws stacked"""
    bgr = cc.random_bgr(*BIG, seed)
    planes, add = random_planes(3, 80, 160, seed + 1), random_add(3, seed + 2)
    region = (3, 1, 295, 61)
    xy = [((i * 37) % 310 - 5, (i * 11) % 70 - 3) for i in range(65)]
    want = draw_points(add_planes(bgr, planes, THRESHOLD, add, region), xy, 3, POINT_COLOUR)
    with cc.OnCanvas(lib, bgr) as oc:
        c = oc.canvas
        if device_pointer is not None:
            ptr, keep = device_pointer(planes)
            c.add_planes(ptr, THRESHOLD, add, region, device_shape=planes.shape)
        else:
            c.add_planes(planes, THRESHOLD, add, region)
        c.draw_points(xy, 3, POINT_COLOUR)
        assert np.array_equal(c.fetch("bgr8"), want)
        for size in ((37, 111), (128, 600)):
            check_planes(c.fetch("bgr8", size=size), cc.from_bgr("bgr8", resized(want, size)), size)
        check_planes(c.fetch("nv12", size=(36, 110)), cc.from_bgr("nv12", resized(want, (36, 110))), "nv12")


# ---- refusals that need no engine
def check_display_refusals(lib):
    import ctypes as C

    import pytest

    f, c = lib.Frame(), lib.Canvas()
    try:
        planes, add = np.zeros((3, 3, 5), np.float32), np.zeros((3, 3), np.uint8)
        for call in (lambda: c.add_planes(planes, 0.0, add, (0, 0, 2, 2)), lambda: c.draw_points([(0, 0)]), lambda: c.fetch("bgr8", size=(2, 2))):
            with pytest.raises(lib.VpError, match="no picture"):
                call()
        bgr = cc.random_bgr(7, 5, 0)
        f.upload(bgr, "bgr8")
        c.begin(f)
        P, A = planes.ctypes.data_as(C.c_void_p), add.ctypes.data_as(C.c_void_p)
        raw = lambda *a: c._ck(c._lib.vp_canvas_add_planes_f32(c._h, *a))   # noqa: E731
        for n in (0, 5, -1):
            with pytest.raises(ValueError, match="n_planes"):
                raw(P, 0, n, 3, 5, 0.0, A, 0, 0, 2, 2)
        for p, a in ((None, A), (P, None)):
            with pytest.raises(ValueError, match="null"):
                raw(p, 0, 3, 3, 5, 0.0, a, 0, 0, 2, 2)
        for mh, mw in ((0, 5), (3, 0), (16385, 5), (3, 16385)):
            with pytest.raises(ValueError, match="plane size"):
                raw(P, 0, 3, mh, mw, 0.0, A, 0, 0, 2, 2)
        for t in (float("nan"), float("inf"), float("-inf")):
            with pytest.raises(ValueError, match="threshold"):
                c.add_planes(planes, t, add, (0, 0, 2, 2))
        for region in ((0, 0, 6, 7), (4, 0, 2, 2), (0, 6, 2, 2), (-1, 0, 4, 4), (0, 0, 1, 7), (0, 0, 5, 1), (0, 0, 5, 0)):
            with pytest.raises(ValueError, match="region"):
                c.add_planes(planes, 0.0, add, region)
        xy, colour = np.zeros((2, 2), np.int32), np.zeros(3, np.uint8)
        X, K = xy.ctypes.data_as(C.c_void_p), colour.ctypes.data_as(C.c_void_p)
        pts = lambda *a: c._ck(c._lib.vp_canvas_draw_points(c._h, *a))   # noqa: E731
        for n in (-1, 4097):
            with pytest.raises(ValueError, match="n outside"):
                pts(X, n, 3, K)
        with pytest.raises(ValueError, match="null points"):
            pts(None, 1, 3, K)
        with pytest.raises(ValueError, match="null colour"):
            pts(X, 1, 3, None)
        for radius in (-1, 17):
            with pytest.raises(ValueError, match="radius"):
                c.draw_points([(1, 1)], radius)
        c.draw_points([], 3)                                    # n = 0: nothing
        pts(None, 0, 3, K)
        assert np.array_equal(c.fetch("bgr8"), bgr)             # and nothing above drew
        for size in ((0, 4), (4, 0), (16385, 4), (4, 16385), (-1, -1)):
            with pytest.raises(ValueError, match="frame size"):
                c.fetch("bgr8", size=size)
        for fmt in ("nv12", "yuy2", "i420"):
            with pytest.raises(ValueError, match="even width"):
                c.fetch(fmt, size=(4, 5))
        for fmt in ("nv12", "i420"):
            with pytest.raises(ValueError, match="even height"):
                c.fetch(fmt, size=(5, 4))
        with pytest.raises(ValueError, match="even width"):
            c.fetch("yuy2", size=(1, 1))
        with pytest.raises(ValueError, match="below the row's"):
            c.fetch("bgra8", size=(3, 2), strides=[7])
        with pytest.raises(ValueError, match="plane"):
            c.fetch("bgr8", size=(3, 2), strides=[6, 6])
        with pytest.raises(ValueError, match="unknown format"):
            c.fetch(8, size=(3, 2))
        assert c.hw() == (7, 5) and np.array_equal(c.fetch("bgr8"), bgr)
    finally:
        c.close()
        f.close()
