"""Shared cases of the Python-wrapper AutoSpeed stages (vp_detect_preprocess_pil, vp_detect_postprocess_agnostic) for the emulated and the device
suite: small frames for the Pillow letterbox into a 64 x 128 network input, hand-built raw tensors of 42 boxes (the levels 4x8, 2x4, 1x2 of that
input) for the class-agnostic decode, and the comparison against tests/autospeed_py_ref.py."""
import os

import numpy as np
from PIL import Image

import autospeed_py_ref as ref

NET_H, NET_W, BOXES = 64, 128, 42
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "autospeed_py.npz")
# (h, w) into 64 x 128: pads left and right; pads left and right (new_w 71); pads top and bottom (new_h 51); no resize and no padding; one pixel
LETTERBOX_FRAMES = [(37, 53), (90, 100), (40, 100), (64, 128), (1, 1)]


def frame(h, w, seed):
    """HxWx3 uint8 RGB noise over smooth ramps; every byte value occurs when the frame has 256 pixels or more (the / 255 table is then checked whole
    on a frame that is not resized)."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if h * w >= 256:
        f.reshape(-1, 3)[:256] = np.arange(256, dtype=np.uint8)[:, None]
    return f


def letterbox_want(frame_rgb, net_h=NET_H, net_w=NET_W):
    """Pillow itself + / 255: ([3][net_h][net_w] float32, (scale, pad_x, pad_y))"""
    return ref.letterbox_pil(Image.fromarray(frame_rgb), (net_w, net_h))


def check_letterbox(det, vp_rgb8, vp_bgr8, f):
    """both byte orders of one frame through Detector.preprocess_pil, bit for bit against Pillow; the stored geometry is the reference's"""
    want, (scale, pad_x, pad_y) = letterbox_want(f, det.net_h, det.net_w)
    for fmt, view in ((vp_rgb8, f), (vp_bgr8, np.ascontiguousarray(f[:, :, ::-1]))):
        got, geom = det.preprocess_pil(view, fmt)
        assert (geom[0], geom[1], geom[2]) == (np.float32(scale), pad_x, pad_y)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (f.shape, fmt)
    return want, (pad_x, pad_y)


def _raw(nc, boxes):
    """[4 + nc][42]: `boxes` = {index: (cx, cy, w, h, class, raw score)}; every other column is a far-away box whose scores are -6 (sigmoid 0.0025)"""
    raw = np.full((4 + nc, BOXES), -6.0, np.float32)
    raw[:4] = np.array([1000.0, 1000.0, 2.0, 2.0], np.float32)[:, None]
    for i, (cx, cy, w, h, c, s) in boxes.items():
        raw[:4, i] = (cx, cy, w, h)
        raw[4 + c, i] = s
    return raw


def decode_cases():
    """(name, raw, conf, iou, (scale, pad_x, pad_y), orig_w, orig_h, cap or None, kept box indices in output order or None).  IoUs of 10 x 10 boxes
    shifted by 3 / 6 pixels are 7/13 = 0.54 and 4/16 = 0.25: clear of the 0.45 threshold; raw scores are 0.25 apart or more."""
    geom, ow, oh = (0.5, 10, 4), 216, 112
    cases = []
    # equal scores: three separate boxes come out in index order; of two overlapping boxes with one score the lower index stays
    b = {30: (20, 20, 10, 10, 0, 1.5), 5: (50, 20, 10, 10, 0, 1.5), 17: (80, 20, 10, 10, 0, 1.5), 8: (20, 45, 10, 10, 0, 1.0), 20: (23, 45, 10, 10, 0, 1.0)}
    cases.append(("equal scores", _raw(1, b), 0.6, 0.45, geom, ow, oh, None, [5, 17, 30, 8]))
    # the same boxes in another class are suppressed all the same (the C++ decode would keep them); the first maximum names the class
    b = {3: (30, 30, 10, 10, 0, 2.0), 9: (33, 30, 10, 10, 2, 1.0), 12: (90, 30, 10, 10, 3, 1.25), 13: (90, 33, 10, 10, 1, 0.75)}
    raw = _raw(4, b)
    raw[4 + 3, 3] = 2.0                                    # box 3: classes 0 and 3 tie -> class 0
    cases.append(("cross-class suppression", raw, 0.6, 0.45, geom, ow, oh, None, [3, 12]))
    # A suppresses B; B would have suppressed C, but B is gone: C stays
    b = {2: (30, 30, 10, 10, 1, 2.0), 1: (33, 30, 10, 10, 1, 1.5), 0: (36, 30, 10, 10, 1, 1.0)}
    cases.append(("chain", _raw(4, b), 0.6, 0.45, geom, ow, oh, None, [2, 0]))
    # sigmoid(0) is 0.5 in every arithmetic: the comparison is strict
    b = {7: (30, 30, 10, 10, 0, 0.0), 11: (60, 30, 10, 10, 0, 0.25)}
    cases.append(("score equal to conf", _raw(1, b), 0.5, 0.45, geom, ow, oh, None, [11]))
    cases.append(("zero kept", _raw(4, b), 0.9, 0.45, geom, ow, oh, None, []))
    # boxes over the edges of the letterbox content: clamped to [0, orig] on both sides
    b = {4: (8, 6, 12, 12, 0, 2.0), 6: (120, 62, 14, 10, 1, 1.0)}
    cases.append(("clamped", _raw(4, b), 0.6, 0.45, geom, ow, oh, None, [4, 6]))
    # every box a candidate, none overlapping: 42 kept, a buffer of 5 gets the first 5 and the full count
    b = {i: (6 + (i % 8) * 15, 5 + (i // 8) * 10, 8, 8, i % 4, 3.0 - 0.05 * ((i * 17) % BOXES)) for i in range(BOXES)}
    order = sorted(range(BOXES), key=lambda i: (i * 17) % BOXES)
    cases.append(("more than cap", _raw(4, b), 0.6, 0.45, geom, ow, oh, 5, order))
    cases.append(("all kept", _raw(4, b), 0.6, 0.45, (1.0, 0, 0), NET_W, NET_H, None, order))
    return cases


LARGE_BOXES = 2100


def large_case(boxes=LARGE_BOXES):
    """(raw [8][boxes], conf, iou, geometry, orig_w, orig_h): more than 1024 candidates, so the sort holds several keys per thread and the compaction
    several rows per thread.  10 x 10 boxes on a 15-pixel grid of 68 columns, every one a candidate; every odd k with (k // 2) % 5 == 0 sits 3 pixels
    right of box k - 1 instead (IoU 7/13 = 0.54 against the 0.45 threshold: one of the two goes, a tenth of all boxes), every other pair is disjoint.
    Raw scores 3.0 - 0.001 * ((k * 997) % 2100) in class k % 4 are all different (997 is prime): their sigmoids are 4.5e-5 apart or more, about
    750 fp32 ulps, and 0.11 or more above conf."""
    k = np.arange(boxes)
    raw = np.full((8, boxes), -6.0, np.float32)
    raw[0] = 6 + (k % 68) * 15
    raw[1] = 6 + (k // 68) * 15
    near = (k % 2 == 1) & ((k // 2) % 5 == 0)
    raw[0, near] = raw[0, k[near] - 1] + 3
    raw[1, near] = raw[1, k[near] - 1]
    raw[2:4] = 10.0
    raw[4 + k % 4, k] = (3.0 - 0.001 * ((k * 997) % 2100)).astype(np.float32)
    return raw, 0.6, 0.45, (0.5, 10, 4), 2028, 1016


def fixture_cases():
    """the fixture's candidate columns (the reference module's raw near or above the threshold) with the fixture's geometry: the kept rows are the
    reference wrapper's own"""
    g = np.load(GOLDEN)
    out = []
    for fi, (h, w, _) in enumerate(g["frames"]):
        geom = (float(g[f"geom_{fi}"][0]), int(g[f"geom_{fi}"][1]), int(g[f"geom_{fi}"][2]))
        out.append((g[f"cand_raw_{fi}"], float(g["conf"]), float(g["iou"]), geom, int(w), int(h), g[f"rows_{fi}"]))
    return out


def pin_cases(large_boxes=(LARGE_BOXES, 1100)):
    """{key: (raw, conf, iou, geometry, orig_w, orig_h)} of everything tests/golden/detect_agnostic_parent.npz holds (tools/pin_detect_agnostic.py)"""
    out = {"decode_%d" % i: c[1:7] for i, c in enumerate(decode_cases())}
    out.update({"fixture_%d" % i: c[:6] for i, c in enumerate(fixture_cases())})
    out.update({"large_%d" % n: large_case(n) for n in large_boxes})
    return out


def pin_record(det, raw, conf, iou, geom, ow, oh):
    """what the pin holds of one case: the rows of a call with room for every box, and the two counts -- that call's and the one a buffer of PIN_CAP
    rows gets (whose rows must be the first PIN_CAP of the full call's)"""
    det.set_letterbox(np.float32(geom[0]), geom[1], geom[2], ow, oh)
    rows, n = det.postprocess_agnostic(raw, conf, iou)
    head, n_cap = det.postprocess_agnostic(raw, conf, iou, cap=PIN_CAP)
    assert np.array_equal(head.view(np.uint32), rows[:PIN_CAP].view(np.uint32))
    return rows, np.array([n, n_cap], np.int32)


PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect_agnostic_parent.npz")
PIN_CAP = 5
PIN_EXACT_COLUMNS = [0, 1, 2, 3, 5]      # plain fp32 + - / : independent of expf.  Column 4 is a sigmoid and keeps the 1e-3 bar of check_decode


def check_parent_pin(det, key):
    """the case `key` against the rows the two-kernel library before the fold gave: counts, row order, corners and class bit-identical"""
    pin = np.load(PIN)
    rows, counts = pin_record(det, *pin_cases()[key])
    want = pin[key + "_rows"]
    assert np.array_equal(counts, pin[key + "_counts"]), (counts, pin[key + "_counts"])
    assert rows.shape == want.shape
    assert np.array_equal(rows[:, PIN_EXACT_COLUMNS].view(np.uint32), want[:, PIN_EXACT_COLUMNS].view(np.uint32))


def rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()) if want.size else 0.0


def check_decode(det, raw, conf, iou, geom, ow, oh, cap=None, want=None):
    """Detector.postprocess_agnostic against the restatement (or `want`): count, order and class equal, floats within 1e-3 * max(1, |ref|)"""
    if want is None:
        want = ref.decode(raw, geom, ow, oh, conf, iou)
    det.set_letterbox(np.float32(geom[0]), geom[1], geom[2], ow, oh)
    got, n = det.postprocess_agnostic(raw, conf, iou, cap=cap)
    assert n == len(want), (n, len(want))
    want = want if cap is None else want[:cap]
    assert got.shape == want.shape
    assert np.array_equal(got[:, 5], want[:, 5])
    err = rel(got[:, :5], want[:, :5])
    assert err <= 1e-3, err
    return got, n, err
