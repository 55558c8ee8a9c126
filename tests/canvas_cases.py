"""Shared cases of the vp_canvas tests (tests/test_canvas_host.py on the emulated library, tests/test_gpu_canvas.py on the MI355X).

Numpy restatements of what include/vp_hip.h defines: the region blend (oracle/pre_post.visualize_mask on the region's pixels: the existing call's
arithmetic), the box rule of vp_canvas_draw_detections, the forward BT.601 form of vp_canvas_fetch and the plane layout of every format; and the case
tables: the smallest shapes at which the kernels' indexing can still go wrong (four-pixel blocks: widths that are no multiple of four, odd widths, odd
region offsets, the last row and column, more than one chunk of boxes)."""
import numpy as np

from oracle import pre_post

FORMATS = ("bgr8", "rgb8", "bgra8", "rgba8", "gray8", "nv12", "yuy2", "uyvy")
PX_BYTES = {"bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4, "gray8": 1, "nv12": 1, "yuy2": 2, "uyvy": 2}


# ---- region blend
def blend_region(canvas, mask, viz_type, region):
    """vp_canvas_blend_mask_u8: `mask` nearest-resized to the region (x0, y0, w, h), coloured, blended 50 / 50 with the canvas pixels of the region"""
    x0, y0, w, h = region
    out = canvas.copy()
    out[y0:y0 + h, x0:x0 + w] = pre_post.visualize_mask(mask, canvas[y0:y0 + h, x0:x0 + w], viz_type)
    return out


def paste_region(canvas, picture, region):
    x0, y0, w, h = region
    out = canvas.copy()
    out[y0:y0 + h, x0:x0 + w] = picture
    return out


# ---- boxes
def box_colour(class_id):
    return {1: (0, 0, 255), 2: (0, 255, 255), 3: (255, 255, 0)}.get(int(class_id), (255, 255, 255))


def fill_fifth(colour, d):
    """nearest integer to (colour + 4 d) / 5; never a tie (the fraction is a multiple of 0.2)"""
    return (2 * np.asarray(colour, np.int64) + 8 * np.asarray(d, np.int64) + 5) // 10


def fill_addweighted(colour, d, fused):
    """cv::addWeighted(overlay, 0.2, frame, 0.8, 0) on u8 in float32, rounded half to even: overlay * alpha + frame * beta with every product and the sum
    rounded to float32 (unfused), or fma(overlay, alpha, fl(frame * beta)) (fused; evaluated in float64, where product and sum are exact)"""
    a, b = np.float32(0.2), np.float32(0.8)
    c, d = np.asarray(colour, np.float32), np.asarray(d, np.float32)
    fb = (d * b).astype(np.float32)
    t = (c.astype(np.float64) * np.float64(a) + fb.astype(np.float64)).astype(np.float32) if fused else ((c * a).astype(np.float32) + fb).astype(np.float32)
    return np.clip(np.rint(t), 0, 255).astype(np.int64)


def draw_boxes(canvas, rows):
    """vp_canvas_draw_detections, one detection after the other.  rows: [n][6] x1, y1, x2, y2, confidence, class_id"""
    out = canvas.copy()
    H, W = out.shape[:2]
    for x1, y1, x2, y2, _, cls in np.asarray(rows, np.float32).reshape(-1, 6):
        bx, by, bw, bh = int(x1), int(y1), int(np.float32(x2) - np.float32(x1)), int(np.float32(y2) - np.float32(y1))   # int(): toward zero
        if bw <= 0 or bh <= 0:
            continue
        colour = np.array(box_colour(cls), np.int64)
        cx0, cy0, cx1, cy1 = max(bx, 0), max(by, 0), min(bx + bw - 1, W - 1), min(by + bh - 1, H - 1)
        if cx1 < cx0 or cy1 < cy0:
            continue
        out[cy0:cy1 + 1, cx0:cx1 + 1] = fill_fifth(colour, out[cy0:cy1 + 1, cx0:cx1 + 1])
        for y in (by, by + bh - 1):          # the outline of the rectangle before clipping: a side outside the canvas is not drawn
            if 0 <= y < H:
                out[y, cx0:cx1 + 1] = colour
        for x in (bx, bx + bw - 1):
            if 0 <= x < W:
                out[cy0:cy1 + 1, x] = colour
    return out


def det(x1, y1, x2, y2, cls=1, conf=0.5):
    return (x1, y1, x2, y2, conf, cls)


def box_cases(h, w):
    """{name: rows} on an h x w canvas: inside, cut by each border, outside, empty, one pixel, overlaps in both orders, two chunks, every colour"""
    a, b = det(1.7, 1.2, w - 1.4, h - 1.1, 1), det(w / 2 - 1, -3.5, w + 6.5, h / 2 + 1.6, 2)
    many = [det((i * 3) % w - 1, (i * 5) % h - 1, (i * 3) % w + 2 + i % 4, (i * 5) % h + 1 + i % 3, i % 5 - 1) for i in range(65)]
    return {
        "inside": [det(1, 1, w - 1, h - 1, 1)],
        "fractional": [det(0.9, 0.2, w - 0.3, h - 0.6, 3)],
        "cut-left": [det(-3.5, 1, 2.6, h - 1, 2)],
        "cut-top": [det(1, -2.2, w - 1, 2.5, 3)],
        "cut-right": [det(w - 2, 0, w + 9, h - 1, 1)],
        "cut-bottom": [det(0, h - 2, w - 1, h + 30, 0)],
        "covers-all": [det(-5, -5, w + 5, h + 5, 2)],
        "outside": [det(w + 1, h + 1, w + 9, h + 9, 1), det(-10, -10, -2, -2, 2), det(-6, 0, 0.5, h, 3)],
        "zero-width": [det(1, 0, 1.5, h, 1)],
        "negative-width": [det(w - 1, 0, 0, h, 1), det(0, h - 1, w, 0, 1)],
        "one-pixel": [det(w - 1, h - 1, w, h, 3), det(0, 0, 1.9, 1.2, 7)],
        "overlap-ab": [a, b],
        "overlap-ba": [b, a],
        "two-chunks": many,
        "class-ids": [det(i % max(w - 1, 1), 0, i % max(w - 1, 1) + 2, h, c) for i, c in enumerate((-1, 0, 1, 2, 3, 7))],
        "none": [],
    }


# ---- forward YUV and the formats
def yuv_raw(R, G, B):
    """(Y, U, V) before the clamp, int64: 20 fractional bits, + 2^19, arithmetic shift"""
    R, G, B = (np.asarray(a).astype(np.int64) for a in (R, G, B))
    y = (269484 * R + 528482 * G + 102760 * B + (16 << 20) + (1 << 19)) >> 20
    u = (-155188 * R - 305135 * G + 460324 * B + (128 << 20) + (1 << 19)) >> 20
    v = (460324 * R - 385875 * G - 74448 * B + (128 << 20) + (1 << 19)) >> 20
    return y, u, v


def bgr_to_yuv(bgr):
    """uint8 planes Y, U, V of a [..., 3] BGR array"""
    y, u, v = yuv_raw(bgr[..., 2], bgr[..., 1], bgr[..., 0])
    return tuple(np.clip(c, 0, 255).astype(np.uint8) for c in (y, u, v))


def from_bgr(fmt, bgr):
    """the planes vp_canvas_fetch returns for an [h][w][3] BGR picture, rows packed"""
    h, w = bgr.shape[:2]
    if fmt == "bgr8":
        return [bgr.reshape(h, 3 * w).copy()]
    if fmt == "rgb8":
        return [bgr[:, :, ::-1].reshape(h, 3 * w).copy()]
    if fmt in ("bgra8", "rgba8"):
        px = np.concatenate([bgr if fmt == "bgra8" else bgr[:, :, ::-1], np.full((h, w, 1), 255, np.uint8)], axis=2)
        return [px.reshape(h, 4 * w)]
    Y, U, V = bgr_to_yuv(bgr)
    if fmt == "gray8":
        return [Y]
    if fmt == "nv12":       # chroma of the top-left pixel of each 2x2 block
        return [Y, np.stack([U[0::2, 0::2], V[0::2, 0::2]], axis=2).reshape(h // 2, w)]
    Ue, Ve = U[:, 0::2], V[:, 0::2]   # chroma of the even pixel of each pair
    q = np.stack([Y[:, 0::2], Ue, Y[:, 1::2], Ve] if fmt == "yuy2" else [Ue, Y[:, 0::2], Ve, Y[:, 1::2]], axis=2)
    return [q.reshape(h, 2 * w)]


def layout(fmt, h, w):
    """[(bytes per row, rows)] of each plane, or None where vp_canvas_layout refuses: h or w outside 2 .. 16384, odd w for the 4:2:x formats, odd h for NV12"""
    if fmt not in FORMATS or not (2 <= h <= 16384 and 2 <= w <= 16384):
        return None
    if fmt in ("nv12", "yuy2", "uyvy") and w % 2:
        return None
    if fmt == "nv12":
        return None if h % 2 else [(w, h), (w, h // 2)]
    return [(PX_BYTES[fmt] * w, h)]


LAYOUT_SIZES = ((2, 2), (7, 5), (11, 14), (9, 13), (6, 10), (3, 2), (3, 10), (720, 1280), (16384, 16384), (1, 4), (4, 1), (16385, 4), (4, 16385), (5, 6), (4, 7))

# (h, w) of the canvas
CANVAS_SIZES = ((2, 2), (7, 5), (11, 14), (9, 13))
FETCH_SIZES = {"nv12": ((2, 2), (6, 10)), "yuy2": ((3, 2), (3, 10)), "uyvy": ((3, 2), (3, 10))}

# ((h, w) of the canvas, (mh, mw) of the mask, region (x0, y0, w, h), viz_type)
BLEND_CASES = (
    ((2, 2), (1, 1), (0, 0, 2, 2), 0),        # the smallest canvas, whole, a 1 x 1 mask
    ((7, 5), (3, 5), (0, 0, 5, 7), 1),        # whole canvas, a row that ends inside a block
    ((7, 5), (1, 1), (3, 0, 2, 2), 2),        # 2 x 2 across a block boundary, odd x0, last column
    ((7, 5), (9, 12), (1, 3, 4, 4), 0),       # odd x0, last row and column
    ((11, 14), (3, 5), (3, 2, 9, 7), 0),      # 3 x 5 mask up to a 7 x 9 (h x w) region, odd x0
    ((11, 14), (9, 12), (9, 7, 5, 4), 2),     # 9 x 12 mask down to a 4 x 5 region in the last rows and columns, odd x0
    ((11, 14), (3, 5), (0, 0, 14, 11), 2),    # whole, width no multiple of 4
    ((9, 13), (3, 5), (4, 2, 9, 7), 1),       # block-aligned x0, last row and column of an odd width
    ((9, 13), (9, 12), (1, 1, 5, 4), 2),
    ((9, 13), (1, 1), (11, 7, 2, 2), 0),      # 2 x 2 in the corner
    ((9, 13), (9, 12), (0, 0, 13, 9), 1),     # whole, odd width
)
MASK_LABELS = np.array([0, 1, 2, 255, 7, 128], np.uint8)   # every row of the three colour tables that is not black, and two that are


def random_bgr(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def random_mask(mh, mw, seed):
    return MASK_LABELS[np.random.default_rng(seed).integers(0, len(MASK_LABELS), size=(mh, mw))]


def corner_bgr(h, w):
    """black, white and the six saturated colours across a picture: the extremes of Y, U and V"""
    cols = np.array([(0, 0, 0), (255, 255, 255), (0, 0, 255), (0, 255, 0), (255, 0, 0), (0, 255, 255), (255, 0, 255), (255, 255, 0)], np.uint8)
    return cols[(np.arange(h)[:, None] * 3 + np.arange(w)[None, :]) % len(cols)]


# ---- checks shared by the two test files: `lib` is autoware_vision_pilot_amd.lib bound to the library under test
class OnCanvas:
    """a Frame holding `bgr` and a Canvas begun on it"""

    def __init__(self, lib, bgr):
        self.frame, self.canvas = lib.Frame(), lib.Canvas()
        try:
            self.frame.upload(np.ascontiguousarray(bgr), "bgr8")
            self.canvas.begin(self.frame)
        except Exception:
            self.close()
            raise

    def close(self):
        self.canvas.close()
        self.frame.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def check_blend(lib, hw, mhw, region, viz, seed=0):
    bgr, mask = random_bgr(*hw, seed), random_mask(*mhw, seed + 1)
    with OnCanvas(lib, bgr) as oc:
        c = oc.canvas
        assert c.hw() == hw
        c.blend_mask_u8(mask, viz, region)
        got = c.fetch("bgr8")
        assert np.array_equal(got, blend_region(bgr, mask, viz, region)), np.argwhere(got != blend_region(bgr, mask, viz, region))[:4]
        # a second overlay on top of the first: the blend reads what the first one wrote
        c.blend_mask_u8(mask.T.copy(), (viz + 1) % 3, region)
        assert np.array_equal(c.fetch("bgr8"), blend_region(blend_region(bgr, mask, viz, region), mask.T, (viz + 1) % 3, region))


def check_boxes(lib, hw, seed=0):
    bgr = random_bgr(*hw, seed)
    with OnCanvas(lib, bgr) as oc:
        c = oc.canvas
        for name, rows in box_cases(*hw).items():
            c.begin(oc.frame)      # a fresh picture for every case
            c.draw_detections(np.array(rows, np.float32).reshape(-1, 6))
            got, want = c.fetch("bgr8"), draw_boxes(bgr, rows)
            assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4])


def check_fetch(lib, fmt, hw, seed=0):
    """packed, and with strides above the row's bytes"""
    h, w = hw
    for bgr in (random_bgr(h, w, seed), corner_bgr(h, w)):
        want = from_bgr(fmt, bgr)
        with OnCanvas(lib, bgr) as oc:
            c = oc.canvas
            for strides in (None, [p.shape[1] + 5 + 2 * i for i, p in enumerate(want)]):
                got = c.fetch(fmt, strides=strides)
                got = list(got) if isinstance(got, tuple) else [got]
                assert len(got) == len(want)
                for g, x in zip(got, want):
                    assert np.array_equal(g.reshape(x.shape), x), (fmt, hw, strides, np.argwhere(g.reshape(x.shape) != x)[:4])


def check_canvas_refusals(lib):
    """every refusal that needs no engine, with its text"""
    import ctypes as C

    import pytest

    f, c = lib.Frame(), lib.Canvas()
    try:
        m = np.zeros((3, 5), np.uint8)
        for call in (lambda: c.fetch("bgr8"), c.hw, c.device, lambda: c.blend_mask_u8(m, 0, (0, 0, 2, 2)), lambda: c.draw_detections([det(0, 0, 2, 2)])):
            with pytest.raises(lib.VpError, match="no picture"):
                call()
        with pytest.raises(lib.VpError, match="never uploaded"):
            c.begin(f)
        f.upload(random_bgr(7, 5, 0), "bgr8")
        c.begin(f)
        assert c.hw() == (7, 5) and c.device()[1] == 24 and c.device()[0]
        for region in ((0, 0, 6, 7), (4, 0, 2, 2), (0, 6, 2, 2), (-1, 0, 4, 4), (0, 0, 1, 7), (0, 0, 5, 1), (0, 0, 5, 0)):
            with pytest.raises(ValueError, match="region"):
                c.blend_mask_u8(m, 0, region)
        with pytest.raises(ValueError, match="mask size"):
            c.blend_mask_u8(np.zeros((0, 5), np.uint8), 0, (0, 0, 2, 2))
        with pytest.raises(ValueError, match="mask size"):
            c._ck(c._lib.vp_canvas_blend_mask_u8(c._h, m.ctypes.data_as(C.c_void_p), 0, 3, 0, 0, 0, 0, 2, 2))
        with pytest.raises(ValueError, match="null mask"):
            c._ck(c._lib.vp_canvas_blend_mask_u8(c._h, None, 0, 3, 5, 0, 0, 0, 2, 2))
        for viz in (-1, 3):
            with pytest.raises(ValueError, match="viz_type"):
                c.blend_mask_u8(m, viz, (0, 0, 2, 2))
        rec = np.zeros((1, 6), np.float32)
        with pytest.raises(ValueError, match="n < 0"):
            c._ck(c._lib.vp_canvas_draw_detections(c._h, rec.ctypes.data_as(C.c_void_p), -1))
        with pytest.raises(ValueError, match="null detections"):
            c._ck(c._lib.vp_canvas_draw_detections(c._h, None, 1))
        with pytest.raises(ValueError, match="coordinate"):
            c.draw_detections([det(0, 0, float("nan"), 2)])
        c.draw_detections([])                                   # n = 0: nothing
        assert np.array_equal(c.fetch("bgr8"), f.fetch_bgr8())  # and nothing above drew
        for fmt in ("nv12", "yuy2", "uyvy"):                    # 7 x 5: odd width
            with pytest.raises(ValueError, match="even width"):
                c.fetch(fmt)
        with pytest.raises(ValueError, match="below the row's"):
            c.fetch("bgra8", strides=[19])
        with pytest.raises(ValueError, match="plane"):
            c.fetch("bgr8", strides=[15, 15])
        with pytest.raises(ValueError, match="unknown format"):
            c.fetch(8)
        f.upload(random_bgr(5, 6, 1), "bgr8")                   # a second begin changes the geometry
        c.begin(f)
        assert c.hw() == (5, 6)
        with pytest.raises(ValueError, match="even height"):
            c.fetch("nv12")
        with pytest.raises(ValueError, match="plane"):
            c.fetch("nv12", strides=[6])
        with pytest.raises(ValueError, match="below the row's"):
            c.fetch("yuy2", strides=[11])
        assert np.array_equal(c.fetch("yuy2"), from_bgr("yuy2", f.fetch_bgr8())[0])
    finally:
        c.close()
        f.close()


def check_engine_region(lib, eng, viz, frame_hw, region, before_first_pass=False, seed=4):
    """infer_frame on `region` (None: the whole frame) of a random frame, then on a fresh canvas: the region == vp_visualize_mask_bgr8 of that engine, the
    rest == the frame; a canvas of another geometry is refused, with both sizes in the text.  Returns (frame bgr, canvas picture)."""
    import pytest

    H, W = frame_hw
    bgr = random_bgr(H, W, seed)
    x0, y0, w, h = region if region is not None else (0, 0, W, H)
    with OnCanvas(lib, bgr) as oc:
        c, f = oc.canvas, oc.frame
        if before_first_pass:
            with pytest.raises(lib.VpError, match="Inference has not been run yet"):
                c.blend_mask(eng, viz)
        eng.infer_frame(f, region)
        want = eng.visualize_mask(viz, (h, w))
        c.blend_mask(eng, viz)
        got = c.fetch("bgr8")
        assert np.array_equal(got[y0:y0 + h, x0:x0 + w], want)
        assert np.array_equal(got, paste_region(f.fetch_bgr8(), want, (x0, y0, w, h)))
        f.upload(random_bgr(H + 2, W, seed), "bgr8")
        c.begin(f)
        with pytest.raises(ValueError, match=f"{W} x {H} frame.*{W} x {H + 2} picture"):
            c.blend_mask(eng, viz)
    return bgr, got
