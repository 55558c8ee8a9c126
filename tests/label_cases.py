"""vp_metric's label part: the shared cases and a plain numpy reference of the contract in include/vp_hip.h ("ground truth from the datasets' label files"),
written from that text.  tests/test_label_host.py checks the reference against the fixture tools/pin_label.py made from the reference project's loaders;
tests/test_label_emulated.py and tests/test_gpu_label.py check the kernels and the accumulator against this reference, bit for bit.

Bit for bit for floats means: the same NaN positions and the same bits everywhere else.  IEEE 754 leaves a NaN's sign and payload open (0 / 0 is a negative
quiet NaN on x86 and a positive one on the device), so those bits are not compared."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "label_cases.npz")
SYMBOLS = ("vp_metric_add_seg_label", "vp_metric_add_depth_label", "vp_metric_add_seg_logits_label", "vp_metric_add_depth_plane_label", "vp_metric_label_frames",
           "vp_metric_fetch_labels", "vp_op_label_gt", "vp_op_label_depth_gt")
VP_SCENESEG, VP_SCENE3D, VP_DOMAINSEG = 0, 1, 2
# the nine colours of createGroundTruth, in the contract's order
COLOURS = np.array([(61, 184, 255, 0), (61, 93, 255, 0), (216, 255, 61, 0), (0, 0, 0, 0), (255, 61, 61, 1), (255, 190, 61, 1), (255, 116, 61, 1), (255, 28, 145, 1),
                    (0, 255, 220, 2)], dtype=np.uint8)
TWO_ROWS = np.array([(0, 255, 220, 1), (0, 0, 0, 0)], dtype=np.uint8)
ROI_DATASETS = ("ACDC", "BDD100K", "IDDAW", "MUSES", "MAPILLARY", "COMMA10K")


# ---- the reference
def nearest_index(src, dst):
    """t[d] = min(floor(d * (1 / (dst / src))), src - 1) in double"""
    ifx = np.float64(1.0) / (np.float64(dst) / np.float64(src))
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * ifx).astype(np.int64), src - 1)


def crop_pad(label, box):
    """the PIL crop: pixels of the box outside the image are zero"""
    h, w = label.shape[:2]
    l, t, r, b = (0, 0, w, h) if box is None else (int(v) for v in box)
    out = np.zeros((b - t, r - l) + label.shape[2:], dtype=label.dtype)
    y0, y1, x0, x1 = max(t, 0), min(b, h), max(l, 0), min(r, w)
    if y1 > y0 and x1 > x0:
        out[y0 - t:y1 - t, x0 - l:x1 - l] = label[y0:y1, x0:x1]
    inside = max(y1 - y0, 0) * max(x1 - x0, 0)
    return out, out.shape[0] * out.shape[1] - inside


def classify(rgb, colours):
    """class per pixel of an [..][3] array: that of the first equal row, 255 for none"""
    cls = np.full(rgb.shape[:-1], 255, dtype=np.uint8)
    for r, g, b, c in np.asarray(colours, dtype=np.uint8)[::-1]:
        cls[(rgb[..., 0] == r) & (rgb[..., 1] == g) & (rgb[..., 2] == b)] = c
    return cls


def record(kind, n, freq=(0, 0, 0), unmatched=0, outside=0, nonfinite=0, mn=0.0, mx=0.0):
    return {"kind": kind, "n": n, "freq": tuple(int(f) for f in freq), "unmatched": int(unmatched), "outside": int(outside), "nonfinite": int(nonfinite), "min": float(mn),
            "max": float(mx)}


def seg_ref(label, out_hw, crop=None, colours=None):
    """(ground truth uint8 [oh][ow], record) of a colour [h][w][3] or mask [h][w] label"""
    label = np.asarray(label)
    crop_px, outside = crop_pad(label, crop)
    ch, cw = crop_px.shape[:2]
    if label.ndim == 3:
        full = classify(crop_px, COLOURS if colours is None else colours)
        freq = [int((full == c).sum()) for c in range(3)]
        black = classify(np.zeros((1, 3), np.uint8), COLOURS if colours is None else colours)[0]
        unmatched = int((full == 255).sum()) - (outside if black == 255 else 0)   # inside the image only
        rec = record(VP_SCENESEG, ch * cw, freq, unmatched, outside)
    else:
        full = crop_px
        rec = record(VP_DOMAINSEG, ch * cw, (int((full != 0).sum()), 0, 0), 0, outside)
    gt = full[nearest_index(ch, out_hw[0])][:, nearest_index(cw, out_hw[1])]
    return np.ascontiguousarray(gt), rec


def extremes(v):
    """numpy's min and max; a zero extreme is -0.0 as the minimum if the plane holds one, +0.0 as the maximum if it holds one"""
    mn, mx = np.min(v), np.max(v)
    if mn == 0:
        mn = v.dtype.type(-0.0 if (np.signbit(v) & (v == 0)).any() else 0.0)
    if mx == 0:
        mx = v.dtype.type(0.0 if (~np.signbit(v) & (v == 0)).any() else -0.0)
    return mn, mx


def depth_ref(label, out_hw):
    """(ground truth float32 [oh][ow], record) of a float32 / float64 [h][w] depth label: the loader's expression in the label's own type, then the sampling"""
    v = np.asarray(label)
    assert v.dtype in (np.float32, np.float64)
    with np.errstate(all="ignore"):
        mn, mx = extremes(v)
        g = ((v - mn) / (mx - mn)).astype(np.float32)
    gt = g[nearest_index(v.shape[0], out_hw[0])][:, nearest_index(v.shape[1], out_hw[1])]
    return np.ascontiguousarray(gt), record(VP_SCENE3D, v.size, nonfinite=int((~np.isfinite(v)).sum()), mn=mn, mx=mx)


# ---- comparisons
def same_f32(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool((na == nb).all()) and bool((a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())


def same_f64(a, b):
    a, b = np.float64(a), np.float64(b)
    return (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


def assert_record(got, want):
    """a fetched LABEL_FRAME_DTYPE record against the reference's dict"""
    assert int(got["kind"]) == want["kind"] and int(got["n"]) == want["n"], (got, want)
    assert tuple(int(f) for f in got["freq"]) == want["freq"], (got, want)
    assert int(got["unmatched"]) == want["unmatched"] and int(got["outside"]) == want["outside"] and int(got["nonfinite"]) == want["nonfinite"], (got, want)
    assert same_f64(got["min"], want["min"]) and same_f64(got["max"], want["max"]), (got, want)


# ---- colour and mask cases: name -> (label, crop, colours, out_hw)
def palette_image(h, w, seed, stray=0.05):
    """random pixels of the nine colours, a share `stray` of them with one channel off by one"""
    rng = np.random.default_rng(seed)
    img = COLOURS[rng.integers(0, 9, (h, w)), :3].copy()
    off = rng.random((h, w)) < stray
    chan = rng.integers(0, 3, (h, w))
    for c in range(3):
        sel = off & (chan == c)
        img[sel, c] = np.where(img[sel, c] == 255, 254, img[sel, c] + 1)
    return img


def strided(img, pad_px, poison):
    """the same pixels as a view into rows `pad_px` pixels longer, the padding filled with `poison` (a pixel's bytes)"""
    buf = np.empty((img.shape[0], img.shape[1] + pad_px) + img.shape[2:], dtype=img.dtype)
    buf[...] = poison
    buf[:, :img.shape[1]] = img
    return buf[:, :img.shape[1]]


def nine_colours():
    """every colour exact, with each channel off by one, and in its five other channel orders"""
    rows = []
    for r, g, b, _ in COLOURS.astype(np.int64):
        px = [(r, g, b)]
        for c in range(3):
            v = [r, g, b]
            v[c] = v[c] - 1 if v[c] == 255 else v[c] + 1
            px.append(tuple(v))
        px += [(r, b, g), (g, r, b), (g, b, r), (b, r, g), (b, g, r)]
        rows.append(px)
    return np.tile(np.array(rows, dtype=np.uint8), (2, 3, 1))   # 18 x 27


def colour_case(name):
    road = COLOURS[8, :3]
    if name == "shrink":
        return palette_image(37, 53, 1), None, None, (16, 24)
    if name == "enlarge":
        return palette_image(5, 7, 2), None, None, (16, 24)
    if name == "dropped_column":
        return palette_image(20, 34, 3), (0, 0, 33, 20), None, (16, 24)
    if name == "padded_rows":
        return palette_image(40, 64, 4), (0, 10, 63, 50), None, (16, 24)
    if name == "stride_odd":       # rows of 171 bytes: byte-wise runs
        return strided(palette_image(37, 53, 5), 4, road), None, None, (16, 24)
    if name == "stride_16":        # rows of 240 bytes, 192 used: 16-byte runs next to poisoned padding
        return strided(palette_image(19, 64, 6), 16, road), None, None, (16, 24)
    if name == "nine_colours":
        return nine_colours(), None, None, (16, 24)
    if name == "two_rows":
        return palette_image(37, 53, 7), None, TWO_ROWS, (16, 24)
    if name == "large":            # 257 * 33 runs: several workgroups, ragged rows
        return palette_image(257, 515, 8), None, None, (32, 64)
    if name == "wide_crop":        # rows of 1584 bytes and a box that starts 48 bytes in: 16-byte runs behind a crop, pads right and below
        return palette_image(70, 528, 9), (16, 3, 540, 75), None, (32, 64)
    if name == "negative_box":
        return palette_image(12, 20, 10), (-3, -2, 15, 9), None, (16, 24)
    raise KeyError(name)


COLOUR_CASES = ("shrink", "enlarge", "dropped_column", "padded_rows", "stride_odd", "stride_16", "nine_colours", "two_rows", "large", "wide_crop", "negative_box")
MASK_CASES = ("shrink", "enlarge", "dropped_column", "padded_rows", "stride_odd", "stride_16", "large", "wide_crop", "negative_box")
EMULATED_COLOUR = ("shrink", "enlarge", "dropped_column", "padded_rows", "stride_16", "nine_colours", "two_rows", "negative_box")
EMULATED_MASK = ("shrink", "padded_rows", "stride_16")


def mask_case(name):
    """the colour case's geometry with a mask of 0 / 1 / 128 / 255"""
    img, crop, _, out_hw = colour_case(name)
    rng = np.random.default_rng(100 + len(name))
    m = np.array([0, 1, 128, 255], np.uint8)[rng.integers(0, 4, img.shape[:2])]
    if img.strides[0] != img.shape[1] * 3:
        m = strided(m, img.strides[0] // 3 - img.shape[1], 255)
    return m, crop, None, out_hw


# ---- depth cases: name -> float64 plane; the fp32 case is its rounding
def depth_case(name, dtype):
    rng = np.random.default_rng(200 + len(name))
    if name == "random":
        v = rng.random((37, 53)) * 80.0 + 0.5
    elif name == "negative_and_zero":
        v = rng.random((37, 53)) * 6.0 - 3.0
        v[rng.random(v.shape) < 0.1] = -0.0
        v[rng.random(v.shape) < 0.1] = 0.0
    elif name == "constant":
        v = np.full((9, 11), 2.5)
    elif name == "one_nan":
        v = rng.random((37, 53)) * 10.0
        v[11, 17] = np.nan
    elif name == "one_inf":
        v = rng.random((37, 53)) * 10.0
        v[30, 2] = np.inf
    elif name == "large":
        v = rng.random((257, 515)) * 120.0
    elif name == "strided":
        v = strided((rng.random((21, 30)) * 5.0).astype(dtype), 3, 1e30)
    else:
        raise KeyError(name)
    return v.astype(dtype) if name != "strided" else v


DEPTH_CASES = ("random", "negative_and_zero", "constant", "one_nan", "one_inf", "large", "strided")
DEPTH_OUT = {"large": (32, 64)}
EMULATED_DEPTH = ("random", "negative_and_zero", "constant", "one_nan", "one_inf", "strided")


# ---- checks shared by the emulated and the device suite (lib: autoware_vision_pilot_amd.lib, bound to either library)
def check_colour(lib, name):
    img, crop, colours, out_hw = colour_case(name)
    gt, rec = lib.label_gt(img, out_hw, crop=crop, colours=colours)
    want_gt, want = seg_ref(img, out_hw, crop, colours)
    assert gt.tobytes() == want_gt.tobytes(), name
    assert_record(rec, want)
    return want


def check_mask(lib, name):
    m, crop, _, out_hw = mask_case(name)
    gt, rec = lib.label_gt(m, out_hw, crop=crop)
    want_gt, want = seg_ref(m, out_hw, crop)
    assert gt.tobytes() == want_gt.tobytes(), name
    assert_record(rec, want)
    return want


def check_depth(lib, name, dtype):
    v = depth_case(name, dtype)
    out_hw = DEPTH_OUT.get(name, (16, 24))
    gt, rec = lib.label_depth_gt(v, out_hw)
    want_gt, want = depth_ref(v, out_hw)
    assert same_f32(gt, want_gt), name
    assert_record(rec, want)
    return gt, want


def random_logits(c, out_hw, seed):
    return np.random.default_rng(seed).standard_normal((c,) + tuple(out_hw)).astype(np.float32)


def check_fused(lib):
    """the label forms' vp_metric_frame records are the bytes of add_seg_logits / add_depth_plane fed the host-prepared ground truth; label records in order"""
    m = lib.Metric(max_frames=16)
    try:
        wants = []
        for i, name in enumerate(("shrink", "padded_rows", "two_rows")):
            img, crop, colours, out_hw = colour_case(name)
            lg = random_logits(3, out_hw, 40 + i)
            want_gt, want = seg_ref(img, out_hw, crop, colours)
            m.add_seg_logits_label(lg, img, crop=crop, colours=colours)
            m.add_seg_logits(lg, want_gt, "label")
            wants.append(want)
        mk, crop, _, out_hw = mask_case("stride_16")
        lg = random_logits(1, out_hw, 50)
        want_gt, want = seg_ref(mk, out_hw, crop)
        m.add_seg_logits_label(lg, mk, crop=crop)
        m.add_seg_logits(lg, want_gt, "label")
        wants.append(want)
        for i, dtype in enumerate((np.float32, np.float64)):
            v = depth_case("random", dtype)
            pred = np.random.default_rng(60 + i).random((16, 24)).astype(np.float32)
            want_gt, want = depth_ref(v, (16, 24))
            m.add_depth_plane_label(pred, v)
            m.add_depth_plane(pred, want_gt)
            wants.append(want)
        assert m.frames() == 12 and m.label_frames() == 6
        rec, _ = m.fetch()
        for k in range(0, 12, 2):
            assert rec[k:k + 1].tobytes() == rec[k + 1:k + 2].tobytes(), k
        assert rec[0]["P"].sum() > 0 and np.isfinite(rec[8]["mae"])
        labels = m.fetch_labels()
        assert len(labels) == 6
        for got, want in zip(labels, wants):
            assert_record(got, want)
        m.reset()
        assert m.frames() == 0 and m.label_frames() == 0 and len(m.fetch_labels()) == 0
    finally:
        m.close()


def check_one_buffer(lib):
    """three adds queued back to back from ONE host buffer overwritten right after each call returns: the label is copied before the call returns and
    the metric's stream keeps the order"""
    m = lib.Metric(max_frames=12)
    try:
        lg = random_logits(3, (16, 24), 70)
        imgs = [palette_image(37, 53, 80 + i) for i in range(3)]
        buf = np.empty_like(imgs[0])
        for img in imgs:
            buf[...] = img
            m.add_seg_logits_label(lg, buf)
            buf[...] = 255
        planes = [depth_case("random", np.float64) + i for i in range(3)]
        pred = np.random.default_rng(71).random((16, 24)).astype(np.float32)
        dbuf = np.empty_like(planes[0])
        for v in planes:
            dbuf[...] = v
            m.add_depth_plane_label(pred, dbuf)
            dbuf[...] = np.nan
        for img in imgs:
            m.add_seg_logits(lg, seg_ref(img, (16, 24))[0], "label")
        for v in planes:
            m.add_depth_plane(pred, depth_ref(v, (16, 24))[0])
        rec, _ = m.fetch()
        assert len(rec) == 12
        for k in range(6):
            assert rec[k:k + 1].tobytes() == rec[6 + k:7 + k].tobytes(), k
        labels = m.fetch_labels()
        for got, img in zip(labels[:3], imgs):
            assert_record(got, seg_ref(img, (16, 24))[1])
        for got, v in zip(labels[3:], planes):
            assert_record(got, depth_ref(v, (16, 24))[1])
    finally:
        m.close()


def refusals(lib):
    """(call on a Metric, what it is): every refusal of the operator forms; each is a ValueError and leaves the counts alone"""
    img = palette_image(12, 20, 90)
    lg3, lg1 = random_logits(3, (16, 24), 91), random_logits(1, (16, 24), 92)
    pred = np.zeros((16, 24), np.float32)
    v = np.ones((12, 20), np.float32)
    big = np.lib.stride_tricks.as_strided(np.zeros(16385 * 3, np.uint8), shape=(1, 16385, 3), strides=(16385 * 3, 3, 1))
    tall = np.lib.stride_tricks.as_strided(np.zeros(3, np.uint8), shape=(16385, 1, 3), strides=(0, 3, 1))
    P = lib._P
    raw = lambda m, *a: m._ck(m._lib.vp_metric_add_seg_logits_label(m._h, lib._ptr(lg3), 0, 3, 16, 24, *a))   # noqa: E731
    rawd = lambda m, *a: m._ck(m._lib.vp_metric_add_depth_plane_label(m._h, lib._ptr(pred), 0, 16, 24, *a))  # noqa: E731
    tab = np.ascontiguousarray(COLOURS)
    return [
        (lambda m: raw(m, P(img.ctypes.data), 2, 12, 20, 60, None, lib._ptr(tab), 9), "channels 2"),
        (lambda m: raw(m, P(img.ctypes.data), 4, 12, 20, 80, None, lib._ptr(tab), 9), "channels 4"),
        (lambda m: m.add_seg_logits_label(lg3, img, colours=np.zeros((0, 4), np.uint8)), "no colours"),
        (lambda m: m.add_seg_logits_label(lg3, img, colours=np.zeros((17, 4), np.uint8)), "17 colours"),
        (lambda m: raw(m, P(img.ctypes.data), 3, 12, 20, 60, None, None, 9), "a null table"),
        (lambda m: m.add_seg_logits_label(lg3, img, colours=[(1, 2, 3, 3)]), "class 3"),
        (lambda m: m.add_seg_logits_label(lg3, img, crop=(5, 0, 5, 12)), "cw 0"),
        (lambda m: m.add_seg_logits_label(lg3, img, crop=(0, 7, 20, 6)), "ch -1"),
        (lambda m: m.add_seg_logits_label(lg3, img, crop=(0, 0, 40000, 12)), "a coordinate out of range"),
        (lambda m: m.add_seg_logits_label(lg3, big), "w 16385"),
        (lambda m: m.add_seg_logits_label(lg3, tall), "h 16385"),
        (lambda m: raw(m, P(img.ctypes.data), 3, 12, 20, 59, None, lib._ptr(tab), 9), "a stride below the row"),
        (lambda m: raw(m, None, 3, 12, 20, 60, None, lib._ptr(tab), 9), "a null label"),
        (lambda m: m._ck(m._lib.vp_metric_add_seg_logits_label(m._h, None, 0, 3, 16, 24, P(img.ctypes.data), 3, 12, 20, 60, None, lib._ptr(tab), 9)), "null logits"),
        (lambda m: m.add_seg_logits_label(random_logits(2, (16, 24), 93), img), "c 2"),
        (lambda m: m.add_seg_logits_label(lg1[:, :0], img[..., 0]), "oh 0"),
        (lambda m: rawd(m, P(v.ctypes.data), 2, 12, 20, 20), "dtype 2"),
        (lambda m: rawd(m, P(v.ctypes.data), -1, 12, 20, 20), "dtype -1"),
        (lambda m: rawd(m, P(v.ctypes.data), 0, 12, 20, 19), "a stride below the row"),
        (lambda m: rawd(m, P(v.ctypes.data), 0, 12, 16385, 16385), "w 16385"),
        (lambda m: rawd(m, P(v.ctypes.data), 0, 0, 20, 20), "h 0"),
        (lambda m: rawd(m, None, 0, 12, 20, 20), "a null label"),
        (lambda m: m.add_depth_plane_label(np.zeros((7, 24), np.float32), v), "a plane of 7 rows"),
    ]


def check_refusals(lib):
    import pytest

    m = lib.Metric(max_frames=2)
    try:
        for call, what in refusals(lib):
            with pytest.raises(ValueError):
                call(m)
                raise AssertionError("accepted: " + what)
            assert m.frames() == 0 and m.label_frames() == 0, what
        img = palette_image(12, 20, 94)
        for bad in (lambda: lib.label_gt(img, (0, 24)), lambda: lib.label_gt(img, (16, 24), crop=(3, 3, 3, 9)), lambda: lib.label_gt(img, (16, 24), colours=[(0, 0, 0, 7)]),
                    lambda: lib.label_depth_gt(np.ones((4, 4), np.float32), (16, 0)), lambda: lib.label_depth_gt(np.ones((4, 4), np.int32), (16, 24))):
            with pytest.raises(ValueError):
                bad()
        lg = random_logits(3, (16, 24), 95)
        m.add_seg_logits_label(lg, img)
        m.add_seg_logits_label(lg, img)
        with pytest.raises(lib.VpError, match="full"):
            m.add_seg_logits_label(lg, img)
        assert m.frames() == 2 and m.label_frames() == 2
    finally:
        m.close()
