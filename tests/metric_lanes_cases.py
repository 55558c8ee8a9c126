"""vp_metric, lane part: restatements of the lane networks' validation scores and the cases the emulated library (tests/test_metric_lanes_host.py) and
the MI355X (tests/test_gpu_metric_lanes.py) both run.

The definitions restated here (no reference text is copied):
  lane masks  Models/training/ego_lanes_trainer.py:127-140 (the two 3x3 filters), 214-222 (two 2x2 max pools of the label), 280-356 (the loss)
  lane rows   Models/training/auto_steer_trainer.py:203-222 (the per-line stage of val()), auto_steer_util.py:353-399 (compute_vector_ap)
The lane-mask loss is PINNED: tools/pin_metric_lanes.py runs the trainer's own methods in fp32 and fp64 into tests/golden/metric_lanes.npz, and
compute_vector_ap likewise.  The per-line stage sits inside val(), which needs CUDA and a dataset: it is restated here, not pinned."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from metric_cases import same_f32

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_lanes.npz")
NEW_SYMBOLS = ("vp_metric_add_lanes", "vp_metric_add_lanes_pair", "vp_metric_add_lanes_logits", "vp_metric_lanes_frames", "vp_metric_fetch_lanes", "vp_metric_add_rows",
               "vp_metric_add_rows_pair", "vp_metric_add_rows_raw", "vp_metric_rows_lines", "vp_metric_fetch_rows", "vp_metric_rows_ap")
GX = ((0.125, 0.0, -0.125), (0.25, 0.0, -0.25), (0.125, 0.0, -0.125))
GY = ((0.125, 0.25, 0.125), (0.0, 0.0, 0.0), (-0.125, -0.25, -0.125))
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def key(shape):
    return "%dx%d" % tuple(shape)


# ---------------------------------------------------------------------------------------------------------------- lane masks
def threshold_plane(x):
    """T of the edge term: R = relu(x) where R > 0, and 1.0 where R is 0 -- torch.nn.Threshold(0, 1), not a step function"""
    r = torch.relu(torch.as_tensor(x))
    return torch.where(r > 0, r, torch.ones_like(r))


def _edge(a, b, gx, gy):
    return (torch.abs(F.conv2d(a, gx, padding=1) - F.conv2d(b, gx, padding=1)) + torch.abs(F.conv2d(a, gy, padding=1) - F.conv2d(b, gy, padding=1))).mean()


def lanes_ref(logits, planes, dtype=torch.float32):
    """the frame's scores from logits [3][h][w] and ground-truth planes [3][h][w], in `dtype`, filters applied to both sides as the trainer does"""
    gx, gy = (torch.tensor(m, dtype=dtype).view(1, 1, 3, 3) for m in (GX, GY))
    out, t = {"bce": [], "edge": [], "loss": []}, []
    for c in range(3):
        x = torch.as_tensor(logits[c], dtype=dtype)[None]
        g = torch.as_tensor(planes[c], dtype=dtype)[None]
        bce = F.binary_cross_entropy_with_logits(x, g)
        r = torch.relu(x)
        a, b = threshold_plane(r), g
        e = [_edge(r, g, gx, gy)]
        for _ in range(4):
            a, b = F.avg_pool2d(a, 2, 2), F.avg_pool2d(b, 2, 2)
            e.append(_edge(a, b, gx, gy))
        edge = (e[0] + e[1] + e[2] + e[3] + e[4]) / 5
        out["bce"].append(bce.item())
        out["edge"].append([v.item() for v in e])
        out["loss"].append((edge + bce).item())
        t.append(edge + bce)
    out["score"] = (2 * t[0] + 2 * t[1] + t[2]).item()
    return out


def planes_of_bits(bits):
    return np.stack([((bits >> c) & 1).astype(np.float32) for c in range(3)])


def bits_4x(bits, seed):
    """a label of four times the size whose 4x4 maxima are `bits`: every set bit lands on one to three pixels of its block"""
    rng = np.random.default_rng(seed)
    h, w = bits.shape
    big = np.zeros((4 * h, 4 * w), np.uint8)
    for c in range(3):
        on = (bits >> c) & 1
        for _ in range(3):
            dy, dx = rng.integers(0, 4, (h, w)), rng.integers(0, 4, (h, w))
            ys, xs = np.nonzero(on)
            big[4 * ys + dy[ys, xs], 4 * xs + dx[ys, xs]] |= np.uint8(1 << c)
    return big


def exact_inputs(shape, seed=0):
    """logits: multiples of 1/8 in [-2, 2] with zeros and negative zeros; binary ground truth, about one pixel in eight set"""
    rng = np.random.default_rng(seed + 100 * shape[0] + shape[1])
    lg = (rng.integers(-16, 17, (3,) + tuple(shape)) / 8.0).astype(np.float32)
    lg[:, 1, 2] = -0.0
    bits = (rng.integers(0, 8, shape) == 0).astype(np.uint8) | ((rng.integers(0, 8, shape) == 0).astype(np.uint8) << 1) | ((rng.integers(0, 8, shape) == 0).astype(np.uint8) << 2)
    return lg, bits.astype(np.uint8)


def general_inputs(shape, seed=1):
    """random logits of standard deviation 4, 10 % ground truth"""
    rng = np.random.default_rng(seed + 100 * shape[0] + shape[1])
    lg = (4.0 * rng.standard_normal((3,) + tuple(shape))).astype(np.float32)
    bits = np.zeros(shape, np.uint8)
    for c in range(3):
        bits |= (rng.random(shape) < 0.1).astype(np.uint8) << c
    return lg, bits


EXACT_SHAPES = ((16, 16), (16, 32), (32, 64))
# 16x16: the smallest; 17x33: odd drops at scales 0, 1 and 4; 80x160: the production size and the last of the two-launch shape; 81x160 and 100x260: the
# seven-launch shape, one and several workgroups per plane
GENERAL_SHAPES = ((16, 16), (17, 33), (48, 80), (80, 160), (81, 160), (100, 260))


def _from_golden(prefix, shape, make):
    g = golden()
    lg, bits = make(shape)
    k = prefix + key(shape)
    assert np.array_equal(lg.view(np.uint32), g[k + "_logits"].view(np.uint32)) and np.array_equal(bits, g[k + "_bits"]), "the golden inputs are the generator's"
    unpack = lambda v: {"bce": v[0:3].tolist(), "edge": v[3:18].reshape(3, 5).tolist(), "loss": v[18:21].tolist(), "score": float(v[21])}  # noqa: E731
    return lg, bits, unpack(g[k + "_ref32"]), unpack(g[k + "_ref64"])


def pack(r):
    return np.array(list(r["bce"]) + [v for row in r["edge"] for v in row] + list(r["loss"]) + [r["score"]], np.float64)


def exact_case(shape):
    """inputs and the reference's fp32 results; the property the case rests on is asserted here, on the reference side: its fp32 and fp64 runs agree bit
    for bit (as fp32) in every edge value"""
    lg, bits, r32, r64 = _from_golden("exact_", shape, exact_inputs)
    for c in range(3):
        for s in range(5):
            assert same_f32(r32["edge"][c][s], r64["edge"][c][s]), (shape, c, s, r32["edge"][c][s], r64["edge"][c][s])
    return lg, bits, r32, r64


def general_case(shape):
    return _from_golden("general_", shape, general_inputs)


# roundings of 2^-24 relative to S = max|x| + 1 (no intermediate exceeds it) per element, and a mean is no farther off than its worst element:
#   bce   1 - g, the product, exp (2 ulp), log1p (2 ulp), two sums, the mean's division: 8
#   edge  R - g or T - g (1), four pools of three operations (12), the filter's seven operations on each of Gx and Gy, |.| + |.| and the division: 24 at most
#   loss  edge's (24, the sum of five and the division by 5 add 1 each ... within the 24 of the coarsest scale) + bce's 8 + 1: 33
#   score 2 l0 + 2 l1 + l2: five times the loss's + 3
ROUNDINGS = {"bce": 8, "edge": 24, "loss": 33, "score": 168}


def lanes_bars(lg, r32, r64):
    """per term: the larger of 4 x the reference fp32 run's own distance from its fp64 run and the rounding floor above -- the rule of depth_bars"""
    S = float(np.abs(lg).max()) + 1.0
    flat = lambda r, k: np.asarray(r[k], np.float64).reshape(-1)  # noqa: E731
    return {k: np.maximum(4 * np.abs(flat(r32, k) - flat(r64, k)), n * 2.0 ** -24 * S) for k, n in ROUNDINGS.items()}


def one_record(lib, lg, gt, form="bits"):
    m = lib.Metric(max_frames=1)
    try:
        m.add_lanes_logits(lg, gt, form)
        assert m.lanes_frames() == 1 and m.frames() == 0 and m.det_frames() == 0
        rec, _ = m.fetch_lanes()
    finally:
        m.close()
    return rec[0]


def check_lanes_exact(lib, shape):
    lg, bits, r32, r64 = exact_case(shape)
    r = one_record(lib, lg, bits)
    assert int(r["n"]) == shape[0] * shape[1] and int(r["nonfinite"]) == 0
    for c in range(3):
        for s in range(5):
            assert same_f32(r["edge"][c][s], r64["edge"][c][s]), (c, s, float(r["edge"][c][s]), r64["edge"][c][s])
    return r


def check_lanes_general(lib, shape, report=None):
    lg, bits, r32, r64 = general_case(shape)
    r = one_record(lib, lg, bits)
    bars = lanes_bars(lg, r32, r64)
    assert int(r["n"]) == shape[0] * shape[1] and int(r["nonfinite"]) == 0
    worst = {}
    for k in ROUNDINGS:
        got = np.asarray(r[k], np.float64).reshape(-1)
        dist = np.abs(got - np.asarray(r64[k], np.float64).reshape(-1))
        worst[k] = float((dist / bars[k]).max())
        line = "lanes %dx%d %-5s |lib - fp64| %.3e (bar %.3e, reference fp32 %.3e)" % (shape[0], shape[1], k, dist.max(), bars[k][dist.argmax()],
                                                                                 np.abs(np.asarray(r32[k], np.float64).reshape(-1) - np.asarray(r64[k], np.float64).reshape(-1)).max())
        print(line)
        if report is not None:
            report.append(line)
    for k, v in worst.items():
        assert v <= 1.0, (k, v)
    return r


def check_lanes_gt_forms(lib, shape=(17, 33)):
    """the three ground-truth forms of the same planes: byte-identical records"""
    lg, bits = general_inputs(shape, seed=5)
    big = bits_4x(bits, 9)
    pooled = torch.nn.MaxPool2d(2, stride=2)(torch.nn.MaxPool2d(2, stride=2)(torch.from_numpy(planes_of_bits(big))))   # the trainer's reduction of its label
    assert np.array_equal(pooled.numpy(), planes_of_bits(bits)) and (big != 0).sum() > (bits != 0).sum()
    recs = [one_record(lib, lg, planes_of_bits(bits), "planes"), one_record(lib, lg, bits, "bits"), one_record(lib, lg, big, "bits4x")]
    assert recs[0].tobytes() == recs[1].tobytes() == recs[2].tobytes() and np.isfinite(recs[0]["score"])
    soft = planes_of_bits(bits) * np.float32(0.75)                           # the fp32 form takes any finite planes
    r = one_record(lib, lg, soft, "planes")
    want = lanes_ref(lg, soft, torch.float64)
    assert abs(float(r["score"]) - want["score"]) <= lanes_bars(lg, want, want)["score"][0]


def check_lanes_nan_answers(lib):
    """a NaN or infinite logit, a NaN ground-truth value: every score NaN, the values counted, the frame left out of the means and reported"""
    lg, bits = general_inputs((16, 24), seed=7)
    planes = planes_of_bits(bits)
    a, b, c = lg.copy(), lg.copy(), planes.copy()
    a[1, 3, 4] = np.nan
    b[0, 0, 0], b[2, 15, 23] = np.inf, -np.inf
    c[2, 5, 5] = np.nan
    m = lib.Metric(max_frames=4)
    try:
        for x, g in ((a, planes), (b, planes), (lg, c), (lg, planes)):
            m.add_lanes_logits(x, g, "planes")
        rec, s = m.fetch_lanes()
        assert rec["nonfinite"].tolist() == [1, 2, 1, 0]
        for r in rec[:3]:
            assert np.isnan(r["score"]) and np.isnan(r["bce"]).all() and np.isnan(r["edge"]).all() and np.isnan(r["loss"]).all()
        assert np.isfinite(rec[3]["score"]) and s["frames"] == 4 and s["nan_frames"] == 3 and s["score"] == float(rec[3]["score"])
    finally:
        m.close()


def check_lanes_accumulator(lib, VpError):
    frames = [general_inputs(s, seed=11 + i) for i, s in enumerate(((16, 16), (17, 33), (16, 24)))]
    m = lib.Metric(max_frames=3)
    try:
        empty, s0 = m.fetch_lanes()
        assert len(empty) == 0 and s0["frames"] == 0 and np.isnan(s0["score"])
        for lg, bits in frames:
            m.add_lanes_logits(lg, bits)
        rec, s = m.fetch_lanes()
        assert m.lanes_frames() == 3 and m.frames() == 0 and s["frames"] == 3 and s["nan_frames"] == 0
        f64 = lambda k: rec[k].astype(np.float64)  # noqa: E731
        assert abs(s["score"] - f64("score").mean()) <= 1e-15 * s["score"]
        for c in range(3):
            assert abs(s["loss"][c] - f64("loss")[:, c].mean()) <= 1e-15 * s["loss"][c] and abs(s["bce"][c] - f64("bce")[:, c].mean()) <= 1e-15 * s["bce"][c]
            assert abs(s["edge"][c] - (f64("edge")[:, c, :].sum(axis=1) / 5).mean()) <= 1e-15 * s["edge"][c]
        try:
            m.add_lanes_logits(*frames[0])
        except VpError as ex:
            assert "full" in str(ex)
        else:
            raise AssertionError("a fourth frame was accepted")
        assert m.lanes_frames() == 3
        m.reset()
        assert m.lanes_frames() == 0 and len(m.fetch_lanes()[0]) == 0
        for lg, bits in frames:
            m.add_lanes_logits(lg, bits)
        assert m.fetch_lanes()[0].tobytes() == rec.tobytes()
    finally:
        m.close()


def check_lanes_refusals(lib):
    lg, bits = general_inputs((16, 16))
    m = lib.Metric(max_frames=2)
    try:
        for bad in (lambda: m.add_lanes_logits(lg[:, :15], bits[:15]), lambda: m.add_lanes_logits(lg[:, :, :15], bits[:, :15]), lambda: m.add_lanes_logits(lg, bits, 3),
                    lambda: m.add_lanes_logits(lg, bits[:8]), lambda: m.add_lanes_logits(0, 0, "bits", device_hw=(16, 16)),
                    lambda: m.add_lanes_logits(1 << 20, 1 << 20, "bits", device_hw=(2049, 2048)), lambda: m.add_lanes_logits(1 << 20, (1 << 20) + 2, "planes", device_hw=(16, 16)),
                    lambda: m.add_rows_raw(np.zeros((9, 4)), np.zeros((9, 4)), np.zeros((9, 4)), np.zeros((9, 4))),
                    lambda: m.add_rows_raw(np.zeros(1025), np.zeros(1025), np.zeros(1025), np.zeros(1025)),
                    lambda: m.add_rows_raw(np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4), thr=np.zeros(9)),
                    lambda: m.add_rows_raw(np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4), thr=[]),
                    lambda: m.add_rows_raw(np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4), thr=[0.05, np.nan])):
            try:
                bad()
            except ValueError:
                continue
            raise AssertionError("a bad argument was accepted")
        assert m.lanes_frames() == 0 and m.rows_lines() == 0
        m.add_rows_raw(np.zeros(4), np.ones(4), np.zeros(4), np.ones(4))
        for other in ([0.02, 0.05], [0.02, 0.05, 0.1000001]):            # another table than the run's
            try:
                m.add_rows_raw(np.zeros(4), np.ones(4), np.zeros(4), np.ones(4), thr=other)
            except ValueError as ex:
                assert "table" in str(ex)
            else:
                raise AssertionError("a second threshold table was accepted")
        m.add_rows_raw(np.zeros(4), np.ones(4), np.zeros(4), np.ones(4))
        try:
            m.add_rows_raw(np.zeros(4), np.ones(4), np.zeros(4), np.ones(4))
        except ValueError:
            raise AssertionError("a full accumulator is a state error")
        except lib.VpError as ex:
            assert "full" in str(ex)
        else:
            raise AssertionError("a third line was accepted")
        m.reset()
        m.add_rows_raw(np.zeros(4), np.ones(4), np.zeros(4), np.ones(4), thr=[0.5])    # a new run, a new table
        assert m.rows_lines() == 1
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------- lane rows
THR = (0.02, 0.05, 0.10)


def rows_ref(xp, hv, txp, thv, thr=THR):
    """per line: the terms in fp32 as the trainer forms them, their mean in fp64; tp bits by the fp64 mean"""
    xp, hv, txp, thv = (np.atleast_2d(np.asarray(v, np.float32)) for v in (xp, hv, txp, thv))
    with np.errstate(invalid="ignore"):
        m, mt = (hv > 0.5).astype(np.float32), (thv > 0.5).astype(np.float32)
    term = np.abs(xp * m - txp * mt)
    assert term.dtype == np.float32
    dist = term.astype(np.float64).mean(axis=1)
    conf = hv.astype(np.float64).mean(axis=1)
    with np.errstate(invalid="ignore"):
        tp = sum(((dist < t).astype(np.uint32) << k) for k, t in enumerate(thr))
    return {"dist": dist, "conf": conf, "tp": tp.astype(np.uint32), "valid": m.sum(axis=1).astype(np.uint32), "target_valid": mt.sum(axis=1).astype(np.uint32)}


def rows_torch32(xp, hv, txp, thv):
    """the trainer's own expressions on one line in torch fp32: (dist, conf) as .item() gives them"""
    xp, hv, txp, thv = (torch.as_tensor(np.asarray(v, np.float32)) for v in (xp, hv, txp, thv))
    line = (xp * (hv > 0.5).float()).view(-1)
    target = (txp * (thv > 0.5).float()).view(-1)
    return torch.abs(line - target).mean().item(), hv.mean().item()


def rows_dyadic(n_lines, rows, seed):
    """multiples of 1/64 in [0, 1], h values of 0.25 / 0.5 / 0.75 / 1 (0.5 itself is not valid): every sum is exact; rows a power of two: every mean too.
    Line 0 is its own target (dist 0)."""
    rng = np.random.default_rng(seed)
    xp = (rng.integers(0, 65, (n_lines, rows)) / 64.0).astype(np.float32)
    txp = np.clip(xp + rng.integers(-3, 4, (n_lines, rows)) / 64.0, 0, 1).astype(np.float32)
    hv = (rng.integers(1, 5, (n_lines, rows)) / 4.0).astype(np.float32)
    thv = (rng.integers(1, 5, (n_lines, rows)) / 4.0).astype(np.float32)
    txp[0], thv[0] = xp[0], hv[0]
    return xp, hv, txp, thv


def rows_general(n_lines, rows, seed):
    """lines of sigmoid-like values around their targets at distances spread over the thresholds; every line sits at least 1e-5 from every threshold, by
    the fp64 restatement AND by the trainer's expressions in torch fp32 -- asserted here, no case is left out"""
    rng = np.random.default_rng(seed)
    txp = rng.random((n_lines, rows)).astype(np.float32)
    thv = (rng.random((n_lines, rows)) < 0.7).astype(np.float32)
    spread = np.array([0.004, 0.03, 0.07, 0.2, 0.012, 0.09, 0.055, 0.5])[:n_lines, None]
    xp = (txp + spread * rng.standard_normal((n_lines, rows))).astype(np.float32)
    hv = np.clip(thv * 0.8 + 0.1 + 0.2 * rng.standard_normal((n_lines, rows)), 0, 1).astype(np.float32)
    want = rows_ref(xp, hv, txp, thv)
    for k in range(n_lines):
        d32, _ = rows_torch32(xp[k], hv[k], txp[k], thv[k])
        for t in THR:
            assert abs(want["dist"][k] - t) >= 1e-5 and abs(d32 - t) >= 1e-5, (n_lines, rows, seed, k, t)
        assert abs(d32 - want["dist"][k]) <= 2.0 ** -20 * max(want["dist"][k], 2.0 ** -10)
    return xp, hv, txp, thv


ROWS_DYADIC = ((1, 64, 0), (8, 1024, 1), (3, 1, 2), (2, 256, 3))
ROWS_GENERAL = ((1, 64, 0), (8, 64, 1), (4, 100, 2), (8, 1000, 3), (2, 257, 4))


def fetch_rows_of(lib, arrays, thr=None):
    m = lib.Metric(max_frames=8)
    try:
        m.add_rows_raw(*arrays, thr=thr)
        assert m.rows_lines() == np.atleast_2d(arrays[0]).shape[0] and m.frames() == 0 and m.lanes_frames() == 0
        return m.fetch_rows()
    finally:
        m.close()


def check_rows_dyadic(lib, case):
    arrays = rows_dyadic(*case)
    want = rows_ref(*arrays)
    rec, s = fetch_rows_of(lib, arrays)
    assert s["lines"] == case[0] and s["n_thr"] == 3
    for k, r in enumerate(rec):
        assert same_f32(r["dist"], want["dist"][k]) and same_f32(r["conf"], want["conf"][k]), (k, float(r["dist"]), want["dist"][k])
        assert float(np.float32(want["dist"][k])) == want["dist"][k]                         # the case is exact
        assert int(r["tp"]) == int(want["tp"][k]) and int(r["valid"]) == int(want["valid"][k]) and int(r["target_valid"]) == int(want["target_valid"][k])
    assert float(rec[0]["dist"]) == 0.0 and int(rec[0]["tp"]) == 7
    return rec


def check_rows_general(lib, case):
    arrays = rows_general(*case)
    want = rows_ref(*arrays)
    rec, s = fetch_rows_of(lib, arrays)
    for k, r in enumerate(rec):
        assert abs(float(r["dist"]) - want["dist"][k]) <= 2.0 ** -23 * want["dist"][k] and abs(float(r["conf"]) - want["conf"][k]) <= 2.0 ** -23 * want["conf"][k]
        assert int(r["tp"]) == int(want["tp"][k]) and int(r["valid"]) == int(want["valid"][k]) and int(r["target_valid"]) == int(want["target_valid"][k])
    want_ap = vector_ap(rec["tp"], rec["conf"])
    for k in ("precision", "recall", "mean_ap", "map50"):
        assert abs(s[k] - want_ap[k]) <= 1e-12, k
    return rec


def check_rows_special(lib):
    """a NaN in xp: a NaN dist and no tp bit; a NaN h is not valid; a table of one entry without 0.05: map50 is NaN; thresholds compare in double"""
    xp, hv, txp, thv = rows_dyadic(2, 64, 5)
    xp[1, 3] = np.nan
    hv[0, 7] = np.nan
    rec, s = fetch_rows_of(lib, (xp, hv, txp, thv), thr=[0.5])
    assert np.isnan(rec[1]["dist"]) and int(rec[1]["tp"]) == 0 and np.isnan(rec[0]["conf"]) and int(rec[0]["valid"]) == int((hv[0] > 0.5).sum())
    assert np.isnan(s["map50"]) and s["n_thr"] == 1
    # dist = fp32(0.05) exactly, which is ABOVE the double 0.05: not below it; just below fp32(0.05): below
    f = np.float32(0.05)
    one = lambda v: (np.array([v], np.float32), np.ones(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32))  # noqa: E731
    assert float(f) > 0.05
    assert int(fetch_rows_of(lib, one(f), thr=[0.05])[0][0]["tp"]) == 0 and int(fetch_rows_of(lib, one(np.nextafter(f, np.float32(0))), thr=[0.05])[0][0]["tp"]) == 1


# ---------------------------------------------------------------------------------------------------------------- compute_vector_ap
def vector_ap(tp, conf, thr=THR):
    """compute_vector_ap restated on tp words: per entry the lines by descending conf (stable), cumulative precision and recall, the envelope, the
    101-point interpolation and the trapezoid sum"""
    tp = np.asarray(tp, np.uint32)
    conf = np.asarray(conf, np.float64)
    n = tp.size
    order = np.argsort(-conf, kind="stable")
    aps, ps, rs = [], [], []
    for k in range(len(thr)):
        t = ((tp[order] >> k) & 1).astype(np.int64)
        tpc, fpc = t.cumsum(), (1 - t).cumsum()
        precision = tpc / (tpc + fpc + 1e-16)
        recall = tpc / (n + 1e-16)
        m_rec = np.concatenate(([0.0], recall, [1.0]))
        m_pre = np.concatenate(([0.0], precision, [0.0]))
        m_pre = np.flip(np.maximum.accumulate(np.flip(m_pre)))
        x = np.linspace(0, 1, 101)
        y = np.interp(x, m_rec, m_pre)
        aps.append(float(((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2.0).sum()))
        ps.append(precision.mean())
        rs.append(recall.mean())
    at50 = [a for a, t in zip(aps, thr) if t == 0.05]
    return {"precision": float(np.mean(ps)), "recall": float(np.mean(rs)), "mean_ap": float(np.mean(aps)), "map50": at50[0] if at50 else float("nan"), "ap": aps}


def ap_inputs(name):
    """(tp words, conf) of the pinned AP cases: `tie` has two pairs of lines of equal conf and different tp words among 12 lines; `many` 300 lines of
    distinct conf"""
    rng = np.random.default_rng({"tie": 3, "many": 4}[name])
    n = {"tie": 12, "many": 300}[name]
    conf = rng.random(n).astype(np.float32)
    dist = rng.random(n) * 0.15
    tp = sum(((dist < t).astype(np.uint32) << k) for k, t in enumerate(THR)).astype(np.uint32)
    if name == "tie":
        conf[5], conf[9] = conf[2], conf[7]
        tp[2], tp[5], tp[7], tp[9] = 7, 0, 4, 7
    else:
        assert np.unique(conf).size == n
    return tp, conf


AP_CASES = ("tie", "many")
