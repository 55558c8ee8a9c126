"""The production lane filter restated in numpy, from the definition in include/vp_hip.h (vp_lanes): start points, the sliding-window runs, the integer
moments, the exact least-squares fit (fractions.Fraction) and the temporal smoothing.  The float steps of the search use np.float32 one operation at a
time, as the device does; the fit is exact rational arithmetic, rounded once by float(Fraction).  Nothing here calls the library."""
from fractions import Fraction

import numpy as np

H, W = 80, 160
F32 = np.float32
# the branches a run can take; run_search counts them into `stats`
BRANCHES = ("blind", "other", "clip_left", "clip_right", "clip_top", "clip_bottom", "oob", "horizon", "empty12", "forced_up", "forced_down", "duplicates")


def masks_of(logits, threshold):
    """bool [3][80][160]: logit > threshold (a NaN is never set)"""
    lg = np.asarray(logits, dtype=np.float32)
    assert lg.shape == (3, H, W)
    with np.errstate(invalid="ignore"):
        return lg > F32(threshold)


def start_points(m):
    """((x, y) or None) for the left and the right lane"""
    left = right = None
    for y in range(H - 1, H // 2 - 1, -1):
        xs = np.flatnonzero(m[0, y, :W // 2])
        if xs.size:
            left = (int(xs[-1]), y)
            break
    for y in range(H - 1, H // 2 - 1, -1):
        xs = np.flatnonzero(m[1, y, W // 2:])
        if xs.size:
            right = (W // 2 + int(xs[0]), y)
            break
    return left, right


def _round_half_away(v):
    """roundf of a non-negative float32"""
    return int(np.floor(np.float64(v) + 0.5))


def run_search(m, plane, start, down, stats=None):
    """one run from `start`: (windows [(x, y, w, h)], points [(x, y)]) in order"""
    st = stats if stats is not None else {}

    def hit(k):
        st[k] = st.get(k, 0) + 1

    x, y = start
    if down:
        y += 4
    dirx, diry = F32(0.0), F32(1.0 if down else -1.0)
    empty = 0
    windows, points = [], []
    for _ in range(20):
        if x < 0 or x >= W:
            hit("oob")
            break
        if (down and y >= H) or (not down and y < 0):
            hit("oob")
            break
        hw = 1 if y < 40 else 6
        if down:
            ylo, yhi = y, min(H, y + 4)
            if y + 4 > H:
                hit("clip_bottom")
        else:
            ylo, yhi = max(0, y - 4), y
            if y - 4 < 0:
                hit("clip_top")
        xlo, xhi = max(0, x - hw), min(W, x + hw)
        if x - hw < 0:
            hit("clip_left")
        if x + hw > W:
            hit("clip_right")
        windows.append((xlo, ylo, xhi - xlo, yhi - ylo))
        ego = [(xx, yy) for yy in range(ylo, yhi) for xx in range(xlo, xhi) if m[plane, yy, xx]]
        other = [(xx, yy) for yy in range(ylo, yhi) for xx in range(xlo, xhi) if m[2, yy, xx]] if y >= 40 else []
        taken = ego if len(ego) >= 3 else (other if len(other) >= 3 else None)
        if taken is not None:
            if taken is other:
                hit("other")
            points.extend(taken)
            n = F32(len(taken))
            cx = F32(sum(p[0] for p in taken)) / n
            cy = F32(sum(p[1] for p in taken)) / n
            dx, dy = cx - F32(x), cy - F32(y)
            ln = np.sqrt(dx * dx + dy * dy)          # float32 products, sum and root, one rounding each
            assert ln.dtype == np.float32
            if ln > F32(0.1):
                dirx, diry = dx / ln, dy / ln
            x, y = _round_half_away(cx), _round_half_away(cy)
            empty = 0
        else:
            if not down and y < H // 4:
                hit("horizon")
                break
            empty += 1
            if empty >= 12:
                hit("empty12")
                break
            hit("blind")
            x += int(dirx * F32(4.0))                # truncation toward zero
            y += int(diry * F32(4.0))
        if not down and y >= yhi - 1:
            hit("forced_up")
            y -= 4
        if down and y <= ylo + 1:
            hit("forced_down")
            y += 4
    return windows, points


def moments(points):
    S = [sum(y ** k for _, y in points) for k in range(5)]
    T = [sum(x * y ** k for x, y in points) for k in range(3)]
    return S, T


def fit_exact(S, T, order):
    """the least-squares solution as Fractions (a, b, c), a = 0 for a line; None when the normal equations are singular"""
    s0, s1, s2, s3, s4 = (int(v) for v in S)
    t0, t1, t2 = (int(v) for v in T)
    if order == 1:
        det = s2 * s0 - s1 * s1
        if det == 0:
            return None
        return Fraction(0), Fraction(t1 * s0 - t0 * s1, det), Fraction(s2 * t0 - s1 * t1, det)
    rows = [[Fraction(s4), Fraction(s3), Fraction(s2), Fraction(t2)], [Fraction(s3), Fraction(s2), Fraction(s1), Fraction(t1)], [Fraction(s2), Fraction(s1), Fraction(s0), Fraction(t0)]]
    for c in range(3):                               # Gauss-Jordan in exact arithmetic, independent of the library's Cramer form
        piv = next((r for r in range(c, 3) if rows[r][c] != 0), None)
        if piv is None:
            return None
        rows[c], rows[piv] = rows[piv], rows[c]
        rows[c] = [v / rows[c][c] for v in rows[c]]
        for r in range(3):
            if r != c and rows[r][c] != 0:
                rows[r] = [a - rows[r][c] * b for a, b in zip(rows[r], rows[c])]
    return rows[0][3], rows[1][3], rows[2][3]


def blend(raw, prev, smoothing):
    """s * raw + (1.0f - s) * prev: the factors are floats, the products and the sum doubles"""
    s, t = float(F32(smoothing)), float(F32(1.0) - F32(smoothing))
    return [s * a + t * b for a, b in zip(raw, prev)]


class LaneFilterRef:
    """the whole filter with its smoothing state: update(logits, threshold) -> a dict per frame"""

    def __init__(self, smoothing=0.5):
        self.s = F32(smoothing)
        self.reset()

    def reset(self):
        self.prev = [None, None]

    def update(self, logits, threshold=0.0, stats=None):
        m = masks_of(logits, threshold)
        out = []
        for lane, start in enumerate(start_points(m)):
            r = {"start": start if start else (-1, -1), "windows_up": [], "windows_down": [], "points_up": [], "points_down": [], "order": 0, "singular": False,
                 "smoothed": False, "raw": None, "coeffs": None, "exact": None, "S": [0] * 5, "T": [0] * 3, "min_y": H, "max_y": -1}
            out.append(r)
            if start is None:
                self.prev[lane] = None
                continue
            r["windows_up"], r["points_up"] = run_search(m, lane, start, False, stats)
            r["windows_down"], r["points_down"] = run_search(m, lane, start, True, stats)
            pts = r["points_up"] + r["points_down"]
            if stats is not None and len(set(pts)) < len(pts):
                stats["duplicates"] = stats.get("duplicates", 0) + 1
            r["S"], r["T"] = moments(pts)
            if pts:
                r["min_y"], r["max_y"] = min(y for _, y in pts), max(y for _, y in pts)
            if len(pts) < 4:
                continue
            order = 1 if len(pts) < 30 else 2
            ex = fit_exact(r["S"], r["T"], order)
            if ex is None:
                r["singular"] = True
                continue
            r["order"], r["exact"] = order, ex
            raw = [0.0, float(ex[0]), float(ex[1]), float(ex[2]), float(r["min_y"]), float(r["max_y"])]
            r["raw"] = raw
            cur = list(raw)
            if self.prev[lane] is not None:
                cur = blend(raw, self.prev[lane], self.s)
                r["smoothed"] = True
            self.prev[lane] = cur
            r["coeffs"] = cur
        return out
