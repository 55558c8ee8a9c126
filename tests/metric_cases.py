"""vp_metric: restatements of the reference's validation scores and the cases the emulated library (tests/test_metric_host.py) and the MI355X
(tests/test_gpu_metric.py) both run.

The definitions restated here (no reference text is copied):
  segmentation  Models/training/scene_seg_trainer.py:206-244 (calc_IoU_val's cascade, IoU with its +1 smoothing), domain_seg_trainer.py:236-252
  depth         Models/training/scene_3d_trainer.py:94-109 (the two 3x3 filters), 159-162 (the normalisation), 171-210 (robust mAE, multi-scale edge loss)
Depth is restated twice: in torch fp32 on the CPU -- the reference's own arithmetic, torch.quantile and conv2d included -- and in fp64."""
import numpy as np
import torch
import torch.nn.functional as F

VP_SCENESEG, VP_SCENE3D, VP_DOMAINSEG = 0, 1, 2
NEW_SYMBOLS = ("vp_metric_create", "vp_metric_destroy", "vp_metric_last_error", "vp_metric_reset", "vp_metric_add_seg", "vp_metric_add_depth", "vp_metric_add_seg_pair",
               "vp_metric_add_depth_pair", "vp_metric_frames", "vp_metric_fetch", "vp_metric_add_seg_logits", "vp_metric_add_depth_plane", "vp_op_select_f32")


# ---------------------------------------------------------------------------------------------------------------- segmentation
def cascade(logits):
    """calc_IoU_val's three branches on [3][h][w]: the class index, 3 where no branch holds (a NaN logit)"""
    with np.errstate(invalid="ignore"):
        a, b, c = logits
        first = (a >= b) & (a >= c)
        second = ~first & (b >= a) & (b >= c)
        third = ~first & ~second & (c >= a) & (c >= b)
    return np.where(first, 0, np.where(second, 1, np.where(third, 2, 3))).astype(np.int64)


def predict(logits):
    """class index per pixel, 3 = none; C = 1: class 0 (positive) where logit > 0"""
    if logits.shape[0] == 3:
        return cascade(logits)
    with np.errstate(invalid="ignore"):
        return np.where(logits[0] > 0, 0, 3).astype(np.int64)


def truth_planes(gt, c, gt_form):
    """[c][h][w] booleans"""
    gt = gt.astype(np.int64)
    if gt_form == "bits":
        return np.stack([(gt >> k) & 1 == 1 for k in range(c)])
    if c == 1:
        return (gt != 0)[None]
    return np.stack([gt == k for k in range(c)])


def seg_counts(logits, planes):
    """integer counts of one frame: I, P, G per class and the pixels with a NaN logit"""
    c = logits.shape[0]
    pred = predict(logits)
    I = [int(((pred == k) & planes[k]).sum()) for k in range(c)]
    P = [int((pred == k).sum()) for k in range(c)]
    G = [int(planes[k].sum()) for k in range(c)]
    return {"I": I, "P": P, "G": G, "nonfinite": int(np.isnan(logits).any(axis=0).sum())}


def seg_scores(I, P, G):
    """(iou per class, iou_full), Python doubles"""
    U = [p + g - i for i, p, g in zip(I, P, G)]
    return [(i + 1) / (u + 1) for i, u in zip(I, U)], (sum(I) + 1) / (sum(U) + 1)


def seg_logits(c, h, w, seed):
    """multiples of 1/4 (ties everywhere), every pairwise tie and the triple tie forced, a NaN, a +inf and a -inf"""
    rng = np.random.default_rng(seed)
    lg = (rng.integers(-8, 9, (c, h, w)) / 4.0).astype(np.float32)
    flat = lg.reshape(c, -1)
    if c == 3:
        forced = [(2.0, 2.0, 1.0), (2.0, 1.0, 2.0), (1.0, 2.0, 2.0), (0.5, 0.5, 0.5), (np.nan, 9.0, 0.0), (0.0, np.nan, 9.0), (9.0, 0.0, np.nan), (np.inf, 0.0, 1.0),
                  (0.0, -np.inf, -1.0), (np.inf, np.inf, 0.0), (-np.inf, -np.inf, -np.inf)]
    else:
        forced = [(0.0,), (-0.0,), (np.nan,), (np.inf,), (-np.inf,), (0.25,)]
    for k, v in enumerate(forced):
        flat[:, (k * 7 + 3) % flat.shape[1]] = v
    return lg


def seg_truth(c, h, w, seed, gt_form):
    rng = np.random.default_rng(seed + 1000)
    if gt_form == "bits":
        return rng.integers(0, 256, (h, w)).astype(np.uint8)          # overlapping planes, bits beyond the classes
    return rng.integers(0, 6 if c == 3 else 3, (h, w)).astype(np.uint8)   # labels beyond the classes


SEG_SHAPES = ((3, 8, 8), (3, 5, 13), (3, 33, 67), (1, 9, 31), (3, 320, 640), (1, 320, 640))


def expected_seg_record(logits, gt, gt_form):
    c = logits.shape[0]
    want = seg_counts(logits, truth_planes(gt, c, gt_form))
    want["kind"] = VP_SCENESEG if c == 3 else VP_DOMAINSEG
    want["n"] = logits.shape[1] * logits.shape[2]
    return want


def assert_seg_record(rec, want):
    c = 3 if want["kind"] == VP_SCENESEG else 1
    assert int(rec["kind"]) == want["kind"] and int(rec["n"]) == want["n"]
    for key in ("I", "P", "G"):
        assert rec[key][:c].tolist() == want[key], (key, rec[key].tolist(), want[key])
        assert not rec[key][c:].any()
    assert int(rec["nonfinite"]) == want["nonfinite"]


def check_seg(lib, shape, seed=5):
    """the ten counts bit for bit in both ground-truth forms, the scores equal to the double expression"""
    c, h, w = shape
    lg = seg_logits(c, h, w, seed)
    m = lib.Metric(max_frames=2)
    try:
        wants = []
        for form in ("label", "bits"):
            gt = seg_truth(c, h, w, seed, form)
            m.add_seg_logits(lg, gt, form)
            wants.append(expected_seg_record(lg, gt, form))
        rec, summary = m.fetch()
        assert len(rec) == 2 and wants[0]["nonfinite"] > 0
        for r, want in zip(rec, wants):
            assert_seg_record(r, want)
        scores = [seg_scores(want["I"], want["P"], want["G"]) for want in wants]
        if c == 3:
            for k in range(3):
                assert summary["sceneseg_iou"][k] == (scores[0][0][k] + scores[1][0][k]) / 2
            assert summary["sceneseg_iou_full"] == (scores[0][1] + scores[1][1]) / 2 and summary["sceneseg_frames"] == 2
        else:
            assert summary["domainseg_iou"] == (scores[0][1] + scores[1][1]) / 2 and summary["domainseg_frames"] == 2
            assert scores[0][0][0] == scores[0][1]                                  # DomainSeg: iou[0] and iou_full coincide
    finally:
        m.close()


def check_seg_absent_class(lib):
    """class 2 neither predicted nor labelled: I = P = G = 0 there and its score is (0 + 1) / (0 + 1)"""
    lg = seg_logits(3, 12, 20, 9)
    lg[2] = -50.0
    lg = np.nan_to_num(lg, nan=1.0, posinf=3.0, neginf=-3.0)
    gt = (seg_truth(3, 12, 20, 9, "label") % 2).astype(np.uint8)
    m = lib.Metric(max_frames=1)
    try:
        m.add_seg_logits(lg, gt, "label")
        rec, summary = m.fetch()
        assert_seg_record(rec[0], expected_seg_record(lg, gt, "label"))
        assert rec[0]["P"][2] == 0 and rec[0]["G"][2] == 0 and summary["sceneseg_iou"][2] == 1.0
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------- depth
GX = ((0.125, 0.0, -0.125), (0.25, 0.0, -0.25), (0.125, 0.0, -0.125))
GY = ((0.125, 0.25, 0.125), (0.0, 0.0, 0.0), (-0.125, -0.25, -0.125))


def quantile_ranks(n):
    """(lo, hi, w) of the 0.9 quantile with linear interpolation, in fp32 as torch.quantile forms them"""
    r = np.float32(0.9) * np.float32(n - 1)
    lo = int(np.floor(r))
    return lo, min(lo + 1, n - 1), np.float32(r - np.float32(lo))


def lerp32(a, b, w):
    """torch.lerp in fp32"""
    a, b, w = np.float32(a), np.float32(b), np.float32(w)
    return np.float32(a + w * (b - a)) if w < np.float32(0.5) else np.float32(b - np.float32(b - a) * np.float32(np.float32(1) - w))


def _depth(p, g, dtype):
    """the trainer's validate() arithmetic in `dtype`: scores and the intermediate values the record carries"""
    p = torch.from_numpy(np.asarray(p)).to(dtype)[None, None]
    g = torch.from_numpy(np.asarray(g)).to(dtype)[None, None]

    def ssi(t):
        return (t - torch.min(t)) / (torch.max(t) - torch.mean(t))

    sp, sg = ssi(p), ssi(g)
    A = torch.abs(sp - sg)
    n = A.numel()
    lo, hi, _ = quantile_ranks(n)
    if torch.isnan(A).any():
        q = torch.tensor(float("nan"), dtype=dtype)
        q_lo = q_hi = float("nan")
    else:
        q = torch.quantile(A, 0.9, interpolation="linear")
        s = torch.sort(A.reshape(-1)).values
        q_lo, q_hi = s[lo].item(), s[hi].item()
    kept = A[A < q]
    mae = torch.mean(kept)
    gx = torch.tensor(GX, dtype=dtype).view(1, 1, 3, 3)
    gy = torch.tensor(GY, dtype=dtype).view(1, 1, 3, 3)

    def edge(a, b):
        return torch.mean(torch.abs(F.conv2d(a, gx, padding=1) - F.conv2d(b, gx, padding=1)) + torch.abs(F.conv2d(a, gy, padding=1) - F.conv2d(b, gy, padding=1)))

    total = edge(sp, sg)
    a, b = sp, sg
    for _ in range(3):
        a, b = F.avg_pool2d(a, 2, stride=2), F.avg_pool2d(b, 2, stride=2)
        total = total + edge(a, b)
    mel = total / 4
    S = max(torch.abs(sp).max().item(), torch.abs(sg).max().item())
    return {"q_lo": q_lo, "q_hi": q_hi, "q": q.item(), "kept": int(kept.numel()), "mae": mae.item(), "mel": mel.item(), "S": S, "n": n}


def depth_torch32(p, g):
    return _depth(p, g, torch.float32)


def depth_f64(p, g):
    return _depth(p, g, torch.float64)


def same_f32(a, b):
    """two values equal as float32 bit patterns (NaN equals NaN)"""
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


def dyadic_pair(h, w, seed):
    """planes of multiples of 1/8 in [0, 3] with min 0, max 3 and mean exactly 1, so max - mean = 2: every value of the chain is a dyadic rational
    that fp32 holds, and A takes few values (ties at the quantile)"""
    rng = np.random.default_rng(seed)
    n = h * w

    def fix(v):
        v = np.clip(v, 0, 24)
        v[0], v[1] = 0, 24
        d = 8 * n - int(v.sum())
        while d:
            i = int(rng.integers(2, n))
            step = 1 if d > 0 else -1
            if 0 <= v[i] + step <= 24:
                v[i] += step
                d -= step
        return v

    g = fix(rng.integers(0, 17, n))
    p = fix(g + rng.integers(-3, 4, n))
    return (p / 8.0).astype(np.float32).reshape(h, w), (g / 8.0).astype(np.float32).reshape(h, w)


def exact_case(shape):
    """the dyadic pair of `shape` and its scores; the property the case rests on is asserted here: the torch fp32 restatement equals the fp64 one,
    rounded to fp32, bit for bit in every value the record carries, and the quantile sits on a tie (q_lo == q_hi)"""
    p, g = dyadic_pair(shape[0], shape[1], EXACT_SEEDS[shape])
    r32, r64 = depth_torch32(p, g), depth_f64(p, g)
    for key in ("q_lo", "q_hi", "q", "mae", "mel"):
        assert same_f32(r32[key], r64[key]), (shape, key, r32[key], r64[key])
    assert r32["kept"] == r64["kept"] and r32["q_lo"] == r32["q_hi"] and 0 < r32["kept"] <= quantile_ranks(p.size)[0]
    return p, g, r32


EXACT_SEEDS = {(8, 8): 0, (16, 24): 0}


def check_depth_exact(lib, shape):
    p, g, want = exact_case(shape)
    m = lib.Metric(max_frames=1)
    try:
        m.add_depth_plane(p, g)
        rec, _ = m.fetch()
        r = rec[0]
        assert int(r["kind"]) == VP_SCENE3D and int(r["n"]) == p.size and int(r["nonfinite"]) == 0
        assert int(r["kept"]) == want["kept"]
        for key in ("q_lo", "q_hi", "mae", "mel"):
            assert same_f32(r[key], want[key]), (key, float(r[key]), want[key])
    finally:
        m.close()


GENERAL_SHAPES = ((8, 8), (9, 15), (37, 53), (64, 200), (320, 640))


def general_pair(h, w, seed=3):
    """a random plane and a correlated one: scaled, shifted, perturbed"""
    rng = np.random.default_rng(seed + 31 * h + w)
    g = (rng.random((h, w)) * 40.0 + 2.0).astype(np.float32)
    p = (0.7 * g + 1.5 + 3.0 * rng.standard_normal((h, w))).astype(np.float32)
    return p, g


_general = {}


def general_case(shape):
    """(p, g, torch fp32 restatement, fp64 restatement), computed once per shape"""
    if shape not in _general:
        p, g = general_pair(*shape)
        _general[shape] = (p, g, depth_torch32(p, g), depth_f64(p, g))
    return _general[shape]


def depth_bars(r32, r64):
    """per score: the larger of 4 x the torch-fp32 restatement's own distance from fp64 and 2^-21 x S (about eight fp32 roundings of at most 2^-24 x S
    per element of A; a mean is no farther off than its worst element)"""
    floor = 2.0 ** -21 * r64["S"]
    return {k: max(4 * abs(r32[k] - r64[k]), floor) for k in ("mae", "mel")}


def check_depth_general(lib, shape, report=None):
    p, g, r32, r64 = general_case(shape)
    m = lib.Metric(max_frames=1)
    try:
        m.add_depth_plane(p, g)
        rec, _ = m.fetch()
    finally:
        m.close()
    r = rec[0]
    bars = depth_bars(r32, r64)
    dist = {k: abs(float(r[k]) - r64[k]) for k in ("mae", "mel")}
    line = "depth %dx%d: |mae - fp64| %.3e (bar %.3e, torch fp32 %.3e)  |mel - fp64| %.3e (bar %.3e, torch fp32 %.3e)  kept %d / %d" % (
        shape[0], shape[1], dist["mae"], bars["mae"], abs(r32["mae"] - r64["mae"]), dist["mel"], bars["mel"], abs(r32["mel"] - r64["mel"]), int(r["kept"]), r32["kept"])
    print(line)
    if report is not None:
        report.append(line)
    assert int(r["nonfinite"]) == 0 and int(r["n"]) == p.size
    if r32["q_hi"] > r32["q_lo"]:
        assert int(r["kept"]) == r32["kept"]
    for k in ("mae", "mel"):
        assert dist[k] <= bars[k], (k, dist[k], bars[k])
    assert abs(float(r["q"]) - r64["q"]) <= 2.0 ** -20 * r64["S"] and float(r["q_lo"]) <= float(r["q"]) <= float(r["q_hi"])


def check_depth_nan_answers(lib):
    """what the reference answers: p identical to g -> NaN mae (an empty mean), mel 0; a constant plane -> both NaN; a NaN input -> both NaN and a count.
    The summary reports the three in nan_frames and forms its means from the fourth.  A side of 7 is refused."""
    p, g = general_pair(12, 20)
    const = np.full((12, 20), 2.5, np.float32)
    bad = p.copy()
    bad[3, 4] = np.nan
    m = lib.Metric(max_frames=8)
    try:
        for a, b in ((g, g), (const, g), (bad, g), (p, g)):
            m.add_depth_plane(a, b)
        rec, summary = m.fetch()
        want = [depth_torch32(a, b) for a, b in ((g, g), (const, g))]
        assert np.isnan(want[0]["mae"]) and want[0]["mel"] == 0.0 and np.isnan(want[1]["mae"]) and np.isnan(want[1]["mel"])   # torch on the CPU agrees
        assert np.isnan(rec[0]["mae"]) and rec[0]["mel"] == 0.0 and rec[0]["kept"] == 0 and rec[0]["nonfinite"] == 0
        assert np.isnan(rec[1]["mae"]) and np.isnan(rec[1]["mel"]) and rec[1]["nonfinite"] == 0
        assert np.isnan(rec[2]["mae"]) and np.isnan(rec[2]["mel"]) and rec[2]["nonfinite"] == 1
        assert np.isfinite(rec[3]["mae"]) and np.isfinite(rec[3]["mel"])
        assert summary["scene3d_frames"] == 4 and summary["nan_frames"] == 3
        assert summary["mae"] == float(rec[3]["mae"]) and summary["mel"] == float(rec[3]["mel"])
        for h, w in ((7, 20), (20, 7)):
            try:
                m.add_depth_plane(np.zeros((h, w), np.float32), np.ones((h, w), np.float32))
            except ValueError:
                pass
            else:
                raise AssertionError("a side of 7 was accepted")
        assert m.frames() == 4
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------- select
SELECT_SIZES = (1, 2, 63, 64, 65, 257, 4099, 204800)


def select_inputs(n, seed=7):
    rng = np.random.default_rng(seed + n)
    fmax = np.finfo(np.float32).max
    sub = np.float32(1e-45)
    mixed = rng.choice(np.array([0.0, sub, 3 * sub, np.float32(1.1e-38), fmax, np.nextafter(fmax, np.float32(0)), fmax / 2, 1.0], np.float32), n)
    ramp = np.linspace(0.0, 1000.0, n, dtype=np.float32)
    return {"random": rng.random(n, dtype=np.float32) * np.float32(3.0), "equal": np.full(n, 0.375, np.float32),
            "two": rng.choice(np.array([0.5, 0.5000001], np.float32), n), "extremes": mixed.astype(np.float32), "ramp": ramp, "reversed": ramp[::-1].copy()}


def check_select(lib, n):
    """bit for bit against np.partition at k = 0, n / 2, floor(0.9 (n - 1)) and n - 1"""
    for name, v in select_inputs(n).items():
        for k in sorted({0, n // 2, int(np.floor(0.9 * (n - 1))), n - 1}):
            want = np.partition(v, k)[k]
            got = lib.select_f32(v, k)
            assert same_f32(got, want), (name, n, k, got, want)


def check_select_refusals(lib):
    for v, k in ((np.array([1.0, -0.0], np.float32), 0), (np.array([1.0, np.inf], np.float32), 0), (np.array([np.nan], np.float32), 0), (np.ones(4, np.float32), 4),
                 (np.ones(4, np.float32), -1), (np.zeros(0, np.float32), 0)):
        try:
            lib.select_f32(v, k)
        except ValueError:
            continue
        raise AssertionError("vp_op_select_f32 accepted %r, k = %d" % (v, k))


# ---------------------------------------------------------------------------------------------------------------- the accumulator
def five_frames():
    """(entry, arguments) of five frames of mixed kinds"""
    p, g = general_pair(9, 15)
    p2, g2 = general_pair(16, 24)
    return (("seg", (seg_logits(3, 5, 13, 1), seg_truth(3, 5, 13, 1, "label"), "label")), ("depth", (p, g)), ("seg", (seg_logits(1, 9, 31, 2), seg_truth(1, 9, 31, 2, "bits"), "bits")),
            ("depth", (p2, g2)), ("seg", (seg_logits(3, 33, 67, 3), seg_truth(3, 33, 67, 3, "bits"), "bits")))


def _add(m, frames):
    for entry, args in frames:
        (m.add_seg_logits if entry == "seg" else m.add_depth_plane)(*args)


def check_accumulator(lib, VpError):
    frames = five_frames()
    m = lib.Metric(max_frames=5)
    try:
        _add(m, frames)
        assert m.frames() == 5
        rec, s = m.fetch()
        assert [int(k) for k in rec["kind"]] == [VP_SCENESEG, VP_SCENE3D, VP_DOMAINSEG, VP_SCENE3D, VP_SCENESEG]
        for i in (0, 2, 4):
            assert_seg_record(rec[i], expected_seg_record(*frames[i][1]))
        # the summary is the host mean of the per-frame scores of the records
        sc = [seg_scores(r["I"][:3].tolist(), r["P"][:3].tolist(), r["G"][:3].tolist()) for r in (rec[0], rec[4])]
        for k in range(3):
            assert s["sceneseg_iou"][k] == (sc[0][0][k] + sc[1][0][k]) / 2
        assert s["sceneseg_iou_full"] == (sc[0][1] + sc[1][1]) / 2
        assert s["domainseg_iou"] == seg_scores(rec[2]["I"][:1].tolist(), rec[2]["P"][:1].tolist(), rec[2]["G"][:1].tolist())[1]
        assert s["mae"] == (float(rec[1]["mae"]) + float(rec[3]["mae"])) / 2 and s["mel"] == (float(rec[1]["mel"]) + float(rec[3]["mel"])) / 2
        assert (s["frames"], s["sceneseg_frames"], s["domainseg_frames"], s["scene3d_frames"], s["nan_frames"]) == (5, 2, 1, 2, 0)
        # frame max_frames + 1
        try:
            m.add_depth_plane(*frames[1][1])
        except VpError as ex:
            assert "full" in str(ex)
        else:
            raise AssertionError("a sixth frame was accepted")
        assert m.frames() == 5
        # reset, then the same five frames again: byte-identical records
        m.reset()
        assert m.frames() == 0
        empty, s0 = m.fetch()
        assert len(empty) == 0 and s0["frames"] == 0 and np.isnan(s0["mae"])
        _add(m, frames)
        again, _ = m.fetch()
        assert again.tobytes() == rec.tobytes()
    finally:
        m.close()
    other = lib.Metric(max_frames=7)          # and from another accumulator
    try:
        _add(other, frames)
        assert other.fetch()[0].tobytes() == rec.tobytes()
    finally:
        other.close()


def check_refusals(lib):
    m = lib.Metric(max_frames=2)
    try:
        lg, gt = seg_logits(3, 8, 8, 0), seg_truth(3, 8, 8, 0, "label")
        for bad in (lambda: m.add_seg_logits(np.zeros((2, 8, 8), np.float32), gt), lambda: m.add_seg_logits(lg, gt, 2),
                    lambda: m.add_seg_logits(0, 0, "label", device_chw=(3, 8, 8)), lambda: m.add_depth_plane(0, 0, device_hw=(8, 8)),
                    lambda: m.add_seg_logits(1 << 20, 1 << 20, "label", device_chw=(3, 4097, 4096))):
            try:
                bad()
            except ValueError:
                continue
            raise AssertionError("a bad argument was accepted")
        assert m.frames() == 0
    finally:
        m.close()
    for n in (0, (1 << 20) + 1):
        try:
            lib.Metric(max_frames=n)
        except ValueError:
            continue
        raise AssertionError("max_frames %d was accepted" % n)
