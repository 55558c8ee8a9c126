"""Cases of the production lane filter (vp_lanes), shared by tests/test_lane_filter_host.py, test_lane_filter_emulated.py and test_gpu_lane_filter.py:
hand-made planes of a few set pixels with literal expectations, a seeded generator of 400 frames, and the comparison of a library record with the numpy
twin (tests/lane_filter_ref.py).  Importing the module runs the twin over the generated set once (a few seconds) and asserts that the set still holds
enough lanes of every outcome and enough hits of every branch, so a change to the generator cannot hollow the tests."""
import ctypes as ct
import functools
import math

import numpy as np

import lane_filter_ref as ref

H, W = ref.H, ref.W
NEW_SYMBOLS = ("vp_lanes_create", "vp_lanes_destroy", "vp_lanes_last_error", "vp_lanes_set_smoothing", "vp_lanes_reset", "vp_lanes_add", "vp_lanes_add_logits",
               "vp_lanes_pending", "vp_lanes_fetch", "vp_lanes_fetch_points", "vp_lanes_fit")
SEED, N_FRAMES = 20260101, 400


def planes(left=(), right=(), other=(), on=1.0, off=-1.0):
    """logits [3][80][160]: `on` at the listed (x, y) pixels, `off` elsewhere"""
    lg = np.full((3, H, W), off, dtype=np.float32)
    for c, px in enumerate((left, right, other)):
        for x, y in px:
            lg[c, y, x] = on
    return lg


def vline(x, y0, y1):
    """the pixels (x, y0 .. y1) inclusive"""
    return [(x, y) for y in range(y0, y1 + 1)]


def _special_values():
    """threshold 0.5 over logits of 0.3 / 0.7, with a NaN, a -inf and a +inf inside the left lane's column"""
    lg = planes(vline(60, 40, 79), vline(100, 40, 79), on=0.7, off=0.3)
    lg[0, 79, 60] = np.nan         # never set: the start moves one row up
    lg[0, 78, 61] = np.inf         # set: a second pixel in row 78, and the start point (the highest x)
    lg[0, 70, 60] = -np.inf        # not set
    lg[1, 79, 100] = 0.5           # not above the threshold
    return lg


# name -> (logits, threshold)
HAND = {
    "empty": (planes(), 0.0),
    "above_only": (planes(vline(60, 5, 39), vline(100, 5, 39)), 0.0),
    "two_lines": (planes(vline(60, 40, 79), vline(100, 40, 79)), 0.0),
    "top_clip": (planes(vline(70, 0, 40), vline(90, 0, 40)), 0.0),
    "edges": (planes(vline(0, 40, 79), vline(159, 40, 79)), 0.0),
    "bridged_below": (planes(vline(50, 70, 79) + vline(50, 40, 57), other=vline(50, 58, 69)), 0.0),
    "unbridged_above": (planes(vline(50, 40, 45) + vline(50, 8, 27), other=vline(50, 28, 39)), 0.0),
    "two_pixel_window": (planes(vline(60, 77, 79)), 0.0),
    "long_gap": (planes(vline(60, 72, 79) + vline(60, 0, 15)), 0.0),
    "start_row_78": (planes(vline(60, 70, 78), vline(100, 66, 79)), 0.0),
    "n3": (planes(vline(60, 76, 79)), 0.0),
    "n4": (planes(vline(60, 75, 79)), 0.0),
    "n29": (planes(vline(60, 62, 79) + [(61, 64)]), 0.0),
    "n30": (planes(vline(60, 61, 79) + [(61, 63), (61, 66)]), 0.0),
    "one_row": (planes([(60, 78)] + [(x, 76) for x in range(58, 62)]), 0.0),
    "special_values": (_special_values(), 0.5),
}

# name -> per lane (start, (windows up, down), (points up, down), order, singular, (a, b, c) or None), worked out from the definition:
#   a column of one pixel per row gives 4 pixels per window and a centroid 1.5 rows above the window's bottom row, which rounds (half away from zero)
#   to 2 rows above: an upward run climbs 2 rows a step and meets most pixels twice.  From row 79 over rows 40 .. 79: 18 full windows (y = 79 .. 45),
#   3 pixels at y = 43, 1 at y = 41 (not taken): 75 points in 20 windows.  The downward run starts at row 83: no window.
NO = ((-1, -1), (0, 0), (0, 0), 0, False, None)
EXPECT = {
    "empty": (NO, NO),
    "above_only": (NO, NO),
    "two_lines": (((60, 79), (20, 0), (75, 0), 2, False, (0.0, 0.0, 60.0)), ((100, 79), (20, 0), (75, 0), 2, False, (0.0, 0.0, 100.0))),
    # from row 40 the 20 steps stand at y = 40, 38, .. 2: 19 full windows, the last is rows [0, 2), clipped at the top, 2 pixels, not taken; the downward
    # run finds nothing from row 44 on and advances blindly 4 rows a step: 9 windows until row 80
    "top_clip": (((70, 40), (20, 9), (76, 0), 2, False, (0.0, 0.0, 70.0)), ((90, 40), (20, 9), (76, 0), 2, False, (0.0, 0.0, 90.0))),
    "edges": (((0, 79), (20, 0), (75, 0), 2, False, (0.0, 0.0, 0.0)), ((159, 79), (20, 0), (75, 0), 2, False, (0.0, 0.0, 159.0))),
    # y = 79, 77, 75: 4 ego pixels each; 73: ego rows 70 .. 72; 71: one ego pixel, other rows 67 .. 69 taken; 68, 66, 64, 62: 4 other pixels each; 60: two
    # of each, nothing taken, blind to 56; 56 .. 44: 4 ego pixels each; 42: two; 38 and 34: none
    "bridged_below": (((50, 79), (20, 0), (62, 0), 2, False, (0.0, 0.0, 50.0)), NO),
    # y = 45: 4; 43: 3; 41 (still >= 40): the other plane's rows 37 .. 39 are taken; 38, 34, 30 (< 40): the other plane is not looked at, blind advances
    # over its rows 28 .. 36; 26 .. 12: 4 ego pixels each; 10: two, and y < 20 ends the run.  Down: blind from row 49 to 77
    "unbridged_above": (((50, 45), (15, 8), (42, 0), 2, False, (0.0, 0.0, 50.0)), NO),
    "two_pixel_window": (((60, 79), (12, 0), (0, 0), 0, False, None), NO),
    # 4 + 4 + 3 points, then 12 empty windows in a row end the run (the far piece in rows 0 .. 15 is never reached)
    "long_gap": (((60, 79), (15, 0), (11, 0), 1, False, (0.0, 0.0, 60.0)), NO),
    # starts on rows 78 and 79: the downward run begins at row 82 / 83, outside the plane, and records no window
    "start_row_78": (((60, 78), (15, 0), (12, 0), 1, False, (0.0, 0.0, 60.0)), ((100, 79), (18, 0), (23, 0), 1, False, (0.0, 0.0, 100.0))),
    # one taken window, then the 12th empty one in a row ends the run
    "n3": (((60, 79), (13, 0), (3, 0), 0, False, None), NO),
    "n4": (((60, 79), (13, 0), (4, 0), 1, False, (0.0, 0.0, 60.0)), NO),
    # 29 points: still a line; 30: a quadratic (the coefficients: the twin's exact rationals, which test_lane_filter_host.py holds against numpy's lstsq)
    "n29": (((60, 79), (19, 0), (29, 0), 1, False, (0.0, -13 / 1085, 66051 / 1085)), NO),
    "n30": (((60, 79), (19, 0), (30, 0), 2, False, (17231 / 8335824, -2560435 / 8335824, 1771287 / 24809)), NO),
    # the start pixel itself lies in no window (the upward window ends above it, the downward run begins 4 rows below): the 4 points are row 76's
    "one_row": (((60, 78), (13, 0), (4, 0), 0, True, None), NO),
    # the NaN at (60, 79) is clear, the +inf at (61, 78) is set and is the start; the right lane's 0.5 at row 79 is not above 0.5
    "special_values": (((61, 78), (20, 0), (69, 0), 2, False, (0.0, 0.0, 60.0)), ((100, 78), (20, 0), (72, 0), 2, False, (0.0, 0.0, 100.0))),
}
HAND_NAMES = tuple(HAND)


def lane_tuple(r):
    """a twin lane in the form of EXPECT"""
    co = None if r["exact"] is None else tuple(float(v) for v in r["exact"])
    return (tuple(r["start"]), (len(r["windows_up"]), len(r["windows_down"])), (len(r["points_up"]), len(r["points_down"])), r["order"], r["singular"], co)


# ---- the generated set
def _curve(rng, left):
    c = rng.uniform(15, 76) if left else rng.uniform(84, 145)
    b = rng.uniform(-0.4, 1.3) * (1 if left else -1)
    a = rng.uniform(-0.012, 0.012)
    return lambda y: c + b * (79 - y) + a * (79 - y) ** 2


def _draw(plane, rng, curve, y0, y1, thick, dropout):
    for y in range(y0, y1 + 1):
        if rng.random() < dropout:
            continue
        x = int(round(curve(y)))
        for xx in range(x, x + thick):
            if 0 <= xx < W:
                plane[y, xx] = True


def frame(i, seed=SEED):
    """frame i of the generated set: logits [3][80][160] (2.0 set, -2.0 clear)"""
    rng = np.random.default_rng([seed, i])
    m = np.zeros((3, H, W), dtype=bool)
    missing = rng.integers(0, 8) == 0
    missing_side = int(rng.integers(0, 2))
    cut_left = rng.integers(0, 8) == 0
    for side in (0, 1):
        curve = _curve(rng, side == 0)
        short = rng.integers(0, 4) == 0                         # a stub of a few rows: the linear fits and the early stops
        y1 = int(rng.integers(60, 80))
        y0 = int(rng.integers(max(40, y1 - 9), y1 - 1)) if short else int(rng.integers(0, 45))
        thick, dropout = int(rng.integers(1, 4)), rng.uniform(0.0, 0.35)
        if missing and side == missing_side:
            continue
        _draw(m[side], rng, curve, y0, y1, thick, dropout)
        if side == 0 and cut_left:
            lower = m[0, 45:].copy()
            m[0, 45:] = False
            m[0, 76:] = lower[31:]                               # the start stays; rows 45 .. 75 of the ego plane are gone ...
            if rng.integers(0, 2):
                m[2, 45:76] |= lower[:31]                        # ... and reappear in the other-lane plane half of the time
    for _ in range(int(rng.integers(0, 3))):
        _draw(m[2], rng, _curve(rng, bool(rng.integers(0, 2))), int(rng.integers(0, 45)), int(rng.integers(60, 80)), int(rng.integers(1, 4)), rng.uniform(0.0, 0.35))
    noise = (0.0, 0.002, 0.01, 0.05)[int(rng.integers(0, 4))]
    if noise:
        m |= rng.random(m.shape) < noise
    return np.where(m, np.float32(2.0), np.float32(-2.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def generated():
    """(frames [400][3][80][160], twin results per frame (no smoothing state: a fresh twin per frame), branch statistics, outcome counts)"""
    frames = np.stack([frame(i) for i in range(N_FRAMES)])
    stats, outcomes, results = {}, {"no_start": 0, "no_fit": 0, "linear": 0, "quadratic": 0}, []
    for lg in frames:
        res = ref.LaneFilterRef().update(lg, 0.0, stats)
        results.append(res)
        for r in res:
            key = "no_start" if r["start"] == (-1, -1) else ("no_fit" if r["order"] == 0 else ("linear" if r["order"] == 1 else "quadratic"))
            outcomes[key] += 1
    return frames, results, stats, outcomes


def assert_coverage():
    _, _, stats, outcomes = generated()
    for k, v in outcomes.items():
        assert v >= 20, ("outcome", k, outcomes)
    for k in ref.BRANCHES:
        if k != "clip_top":                                      # the hand-made case top_clip covers it
            assert stats.get(k, 0) >= 3, ("branch", k, stats)


assert_coverage()
EMULATED_FRAMES = tuple(range(0, N_FRAMES, N_FRAMES // 20))[:20]


# ---- a library record against the twin
def ulp(v):
    return math.ulp(v) if v != 0.0 else 5e-324


def check_lane(got, pts, want, prev=None, smoothing=0.5):
    """got: one LANES_LANE_DTYPE element; pts: uint8 [n][2] of fetch_points; want: the twin's lane; prev: the handle's previous fit of this lane (a list
    of six, or None).  Integers bit for bit; the raw coefficients within one ulp of the correctly rounded exact solution (exact integer determinants, one
    rounded quotient); the smoothed coefficients bit for bit from the record's own raw ones.  Returns the handle's previous fit after this record."""
    assert (int(got["start_x"]), int(got["start_y"])) == tuple(want["start"])
    wins = want["windows_up"] + want["windows_down"]
    assert (int(got["n_windows_up"]), int(got["n_windows_down"])) == (len(want["windows_up"]), len(want["windows_down"]))
    assert got["windows"][:len(wins)].tolist() == [list(w) for w in wins]
    allp = want["points_up"] + want["points_down"]
    assert (int(got["n_points_up"]), int(got["n_points_down"])) == (len(want["points_up"]), len(want["points_down"]))
    assert pts.tolist() == [list(p) for p in allp]
    assert got["S"].tolist() == list(want["S"]) and got["T"].tolist() == list(want["T"])
    assert (int(got["min_y"]), int(got["max_y"])) == (want["min_y"], want["max_y"])
    assert int(got["order"]) == want["order"]
    assert bool(int(got["flags"]) & 1) == want["singular"]
    if tuple(want["start"]) == (-1, -1):
        prev = None
    if not want["order"]:
        assert got["raw_coeffs"].tolist() == [0.0] * 6 and got["coeffs"].tolist() == [0.0] * 6 and int(got["coeffs_valid"]) == 0 and not int(got["flags"]) & 2
        return prev
    raw = got["raw_coeffs"].tolist()
    for g, w in zip(raw, want["raw"]):
        assert abs(g - w) <= ulp(w), (g, w)
    exp = raw if prev is None else ref.blend(raw, prev, smoothing)
    assert got["coeffs"].tolist() == exp and int(got["coeffs_valid"]) == 1 and bool(int(got["flags"]) & 2) == (prev is not None)
    return exp


def run_and_check(lib, frames, thresholds, wants, capacity=8):
    """frames through lib.Lanes.add_logits in batches of `capacity` on ONE handle; every record and point list against the twin results `wants`, the
    smoothing state followed from record to record"""
    lanes = lib.Lanes(capacity=capacity)
    prev = [None, None]
    try:
        i = 0
        while i < len(frames):
            n = min(capacity, len(frames) - i)
            for k in range(n):
                lanes.add_logits(frames[i + k], thresholds[i + k])
            assert lanes.pending() == n
            pts = [[lanes.fetch_points(k, lane) for lane in (0, 1)] for k in range(n)]
            recs = lanes.fetch()
            assert len(recs) == n and lanes.pending() == 0
            for k in range(n):
                for lane in (0, 1):
                    prev[lane] = check_lane(recs[k]["lane"][lane], pts[k][lane], wants[i + k][lane], prev[lane])
            i += n
    finally:
        lanes.close()


SEQUENCE = ("two_lines", "top_clip", "empty", "edges", "n3", "two_lines")   # fit, fit, start lost, fit, start but n < 4 (left; right lost), fit


def check_sequence(lib, smoothing=(0.5, 0.25)):
    """six frames on one handle, fetched at once; the smoothed coefficients and the previous-fit rules against the twin; again after reset() with another factor"""
    lanes = lib.Lanes(capacity=8)
    try:
        for s in smoothing:
            lanes.set_smoothing(s)
            twin = ref.LaneFilterRef(s)
            for k in SEQUENCE:
                lanes.add_logits(*HAND[k])
            pts = [[lanes.fetch_points(i, lane) for lane in (0, 1)] for i in range(len(SEQUENCE))]
            recs = lanes.fetch()
            assert len(recs) == len(SEQUENCE)
            prev = [None, None]
            for i, k in enumerate(SEQUENCE):
                want = twin.update(*HAND[k])
                for lane in (0, 1):
                    got = recs[i]["lane"][lane]
                    prev[lane] = check_lane(got, pts[i][lane], want[lane], prev[lane], s)
                    if want[lane]["coeffs"] is None:
                        assert int(got["coeffs_valid"]) == 0
                    else:                                        # raw is the correctly rounded exact solution here, so the twin's blend is the record's
                        assert got["coeffs"].tolist() == want[lane]["coeffs"] and bool(int(got["flags"]) & 2) == want[lane]["smoothed"]
            flags = [[bool(int(recs[i]["lane"][lane]["flags"]) & 2) for lane in (0, 1)] for i in range(len(SEQUENCE))]
            assert flags == [[False, False], [True, True], [False, False], [False, False], [False, False], [True, False]]
            t = float(np.float32(1.0) - np.float32(s))
            # frame 5, left: two_lines (c = 60) over the fit of `edges` (c = 0), which the fitless frame 4 left untouched; right: lost in frame 4, so unsmoothed
            assert recs[5]["lane"][0]["coeffs"].tolist() == [0.0, 0.0, 0.0, float(np.float32(s)) * 60.0, float(np.float32(s)) * 40.0 + t * 40.0, 78.0]
            assert recs[5]["lane"][1]["coeffs"].tolist() == [0.0, 0.0, 0.0, 100.0, 40.0, 78.0]
            lanes.reset()
            lanes.add_logits(*HAND["two_lines"])
            first = lanes.fetch()[0]
            assert not int(first["lane"][0]["flags"]) & 2 and first["lane"][0]["coeffs"].tolist() == [0.0, 0.0, 0.0, 60.0, 40.0, 78.0]
            lanes.reset()
    finally:
        lanes.close()


def check_refusals_no_engine(lib):
    """every refusal that needs no engine: the code, a text, and nothing changed"""
    for cap in (0, -1, 4097):
        try:
            lib.Lanes(capacity=cap)
        except ValueError as ex:
            assert "capacity" in str(ex)
        else:
            raise AssertionError("capacity %d accepted" % cap)
    so = lib.load()
    assert so.vp_lanes_pending(None) == -1 and so.vp_lanes_reset(None) == -1 and so.vp_lanes_add_logits(None, None, 0.0) == -1
    assert so.vp_lanes_create(None, 0, 4, None, 0) == -1
    lanes = lib.Lanes(capacity=2)
    try:
        def refused(exc, fn, *a):
            try:
                fn(*a)
            except exc as ex:
                assert exc is ValueError or not isinstance(ex, ValueError), ex
                assert len(str(ex)) > 20
            else:
                raise AssertionError("not refused")

        refused(lib.VpError, lanes.fetch_points, 0, 0)           # nothing pending
        refused(ValueError, lanes.add_logits, None)
        refused(ValueError, lanes.add, None)
        refused(ValueError, lanes.set_smoothing, 1.5)
        lanes.add_logits(*HAND["two_lines"])
        lanes.add_logits(*HAND["n4"])
        refused(lib.VpError, lanes.add_logits, *HAND["edges"])    # `capacity` records pending already
        refused(lib.VpError, lanes.reset)                         # records pending
        refused(ValueError, lanes.fetch_points, 2, 0)
        refused(ValueError, lanes.fetch_points, -1, 0)
        refused(ValueError, lanes.fetch_points, 0, 2)
        n = ct.c_int(-7)
        assert so.vp_lanes_fetch(lanes._h, None, 1, ct.byref(n)) == -1 and n.value == -7
        assert so.vp_lanes_fetch(lanes._h, None, 0, None) == -1
        assert so.vp_lanes_fetch_points(lanes._h, 0, 0, None, 4, ct.byref(n)) == -1 and n.value == -7
        assert lanes.pending() == 2
        one = lanes.fetch(1)                                     # max below pending: the oldest record alone
        assert len(one) == 1 and lanes.pending() == 1 and int(one[0]["lane"][0]["n_points_up"]) == 75
        rest = lanes.fetch()
        assert len(rest) == 1 and int(rest[0]["lane"][0]["n_points_up"]) == 4 and bool(int(rest[0]["lane"][0]["flags"]) & 2)
        assert len(lanes.fetch()) == 0
    finally:
        lanes.close()
    for bad in ((3, [4, 6, 14, 36, 98]), (0, [4, 6, 14, 36, 98]), (1, [1 << 40, 0, 0, 0, 0])):
        try:
            lib.lanes_fit(bad[1], [10, 20, 50], bad[0])
        except ValueError:
            pass
        else:
            raise AssertionError("vp_lanes_fit accepted %r" % (bad,))
    assert so.vp_lanes_fit(None, None, 1, None, None) == -1
