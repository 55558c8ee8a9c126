"""The detector-validation cases (vp_metric_add_det*, include/vp_hip.h): seeded inputs, generated and never stored.  tools/pin_detmap.py runs the
reference's own non_max_suppression / compute_metric / compute_ap on them and writes tests/golden/detmap.npz; the host, emulated and GPU tests and
tools/bench_detmap.py generate the same inputs again (the fixture keeps a hash of each) and compare.

A frame is (raw fp32 [4 + nc][nb], labels fp32 [n][5] rows cls, cx, cy, w, h normalised to NET_W x NET_H).  Scores are built from distinct integers, so no
two candidates of a frame are equal; label classes are 0, 1 and 3, class 3 never scores above the threshold (a label class with no detection) and class 2
scores without labels (a detection class with no label)."""
import hashlib

import numpy as np

NET_H, NET_W = 512, 1024
CONF, IOU = 0.001, 0.65
MAX_NMS, MAX_DET = 30000, 300
IOU_V = np.array([0x3F000000, 0x3F0CCCCD, 0x3F19999A, 0x3F266666, 0x3F333333, 0x3F400000, 0x3F4CCCCD, 0x3F59999A, 0x3F666666, 0x3F733333], dtype="<u4").view("<f4")
GRID = 1 << 22

# name -> (builder, seed); the order is the dataset's
FRAMES = ("small", "small_empty", "small_miss", "small_nolabel", "mid", "dense", "mid_b", "mid_c")
SINGLE = ("small", "small_empty", "small_miss", "small_nolabel", "mid", "dense")          # the cases of the issue, one frame each
EMULATED = ("small", "small_empty", "small_miss", "small_nolabel", "mid")


def _unit(rng, n, frame_id):
    """n distinct values in (0, 1), float64: distinct integers of a 2^22 grid, shifted by a fraction of a step per frame"""
    u = rng.permutation(GRID)[:n].astype(np.float64)
    return (u + (frame_id + 0.5) / 16.0) / GRID


def _labels(rng, n):
    box = rng.random((n, 4))
    box[:, :2] = 0.15 + 0.7 * box[:, :2]
    box[:, 2:] = 0.05 + 0.2 * box[:, 2:]
    cls = rng.choice(np.array([0.0, 1.0, 3.0]), n)
    cls[:3] = (0.0, 1.0, 3.0)[:n]
    return np.concatenate((cls[:, None], box), 1).astype(np.float32)


def _jittered(rng, labels, nb, nc, frame_id, dense):
    """boxes jittered around the labels; each box scores high for its label's class"""
    scale = np.array((NET_W, NET_H, NET_W, NET_H), np.float64)
    idx = rng.integers(0, labels.shape[0], nb)
    box = labels[idx, 1:].astype(np.float64) * scale * (1.0 + 0.15 * rng.standard_normal((nb, 4)))
    u = _unit(rng, nb * nc, frame_id).reshape(nb, nc)
    sc = 0.002 + 0.99 * u if dense else u ** 6
    own = labels[idx, 0].astype(np.int64)
    if not dense:
        sc[np.arange(nb), own] = u[np.arange(nb), own] ** 2
    if nc > 3:
        sc[:, 3] = 0.0005 * u[:, 3]                      # class 3 never is a candidate
    raw = np.empty((4 + nc, nb), np.float32)
    raw[:4] = box.T
    raw[4:] = sc.T
    return raw


def small(kind, seed=11):
    """nb 64, nc 1: one workgroup, fewer candidates than a wave"""
    rng = np.random.default_rng(seed)
    labels = _labels(rng, 2)
    labels[:, 0] = 0.0
    fid = {"small": 0, "small_empty": 1, "small_miss": 2, "small_nolabel": 3}[kind]
    raw = _jittered(rng, labels, 64, 1, fid, False)
    u = _unit(rng, 64, fid)
    raw[4] = np.where(u < 0.6, u, 0.0005 * u)             # ~ 38 candidates
    if kind in ("small_empty", "small_miss"):
        raw[4] = 0.0005 * u                               # no candidate
    if kind in ("small_empty", "small_nolabel"):
        labels = labels[:0]
    return raw, labels


def mid(seed, frame_id):
    """nb 1344, nc 4, 6 labels: several workgroups, not a power of two, more than 300 survivors, same-class and cross-class overlaps"""
    rng = np.random.default_rng(seed)
    labels = _labels(rng, 6)
    return _jittered(rng, labels, 1344, 4, frame_id, False), labels


def dense(seed=5):
    """nb 10752, nc 4: 32 256 candidates, above the 30 000 that go on; a NaN score and two coincident zero-area boxes are planted"""
    rng = np.random.default_rng(seed)
    labels = _labels(rng, 6)
    raw = _jittered(rng, labels, 10752, 4, 5, True)
    raw[4 + 1, 777] = np.nan
    for i, s in ((100, 0.99951), (9000, 0.99947)):        # 0 / 0 between them: NaN, suppresses nothing
        raw[:4, i] = (400.0, 200.0, 0.0, 0.0)
        raw[4 + 0, i] = s
    return raw, labels


def frame(name):
    if name.startswith("small"):
        return small(name)
    if name == "dense":
        return dense()
    return mid(*{"mid": (3, 4), "mid_b": (7, 6), "mid_c": (9, 7)}[name])


def digest(raw, labels):
    return hashlib.sha256(np.ascontiguousarray(raw).tobytes() + np.ascontiguousarray(labels).tobytes()).hexdigest()


def labels_px(labels):
    """rows [cls, x1, y1, x2, y2] in pixels, fp32 operation for operation as the device forms them"""
    lb = np.asarray(labels, np.float32).reshape(-1, 5)
    two = np.float32(2)
    W, H = np.float32(NET_W), np.float32(NET_H)
    out = np.empty_like(lb)
    out[:, 0] = lb[:, 0]
    out[:, 1] = (lb[:, 1] - lb[:, 3] / two) * W
    out[:, 2] = (lb[:, 2] - lb[:, 4] / two) * H
    out[:, 3] = (lb[:, 1] + lb[:, 3] / two) * W
    out[:, 4] = (lb[:, 2] + lb[:, 4] / two) * H
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def golden():
    import os

    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detmap.npz"))


# ---- what the emulated and the GPU tests share
def dataset_arrays(items):
    """items: (rows [k][6 or structured], tp [k], labels [n][5]) per frame -> (tp, conf, det_cls, label_cls) under the trainer's bookkeeping: concatenation
    (a frame with neither rows nor labels adds nothing, one without rows only its label classes, one without labels its rows with tp 0)"""
    tp = np.concatenate([np.asarray(t, np.uint32).reshape(-1) for _, t, _ in items])
    conf = np.concatenate([np.asarray(r, np.float32).reshape(-1, 6)[:, 4] for r, _, _ in items])
    cls = np.concatenate([np.asarray(r, np.float32).reshape(-1, 6)[:, 5] for r, _, _ in items])
    lab = np.concatenate([np.asarray(lb, np.float32).reshape(-1, 5)[:, 0] for _, _, lb in items])
    return tp, conf, cls, lab


def golden_frame(g, name):
    return g[name + "_rows"], g[name + "_tp"], tuple(int(v) for v in g[name + "_counts"])


def rows_of(rec):
    """the six floats of structured METRIC_DET_ROW_DTYPE rows"""
    return np.stack([rec[k] for k in ("x1", "y1", "x2", "y2", "conf", "cls")], 1).astype(np.float32).reshape(-1, 6)


def check_validate(lib, name):
    """vp_op_detect_validate against the fixture, floats as bits"""
    g = golden()
    raw, labels = frame(name)
    assert digest(raw, labels) == str(g[name + "_sha256"])
    want_rows, _, want_counts = golden_frame(g, name)
    rows, counts = lib.detect_validate(raw, CONF, IOU)
    assert (counts["candidates"], counts["ranked"], counts["kept"]) == want_counts
    assert np.array_equal(bits(rows), bits(want_rows))


def check_frames(lib, names, runs=2):
    """add_det_raw / fetch_det for the frames `names` in one accumulator: frame records, rows and tp words against the fixture bit for bit, the summary
    against the fixture (the whole dataset) or the host entry on the fixture's arrays; `runs` runs give equal records"""
    g = golden()
    m = lib.Metric(max_frames=len(names))
    try:
        seen = []
        for _ in range(runs):
            m.reset()
            for name in names:
                raw, labels = frame(name)
                m.add_det_raw(raw, labels, (NET_H, NET_W), CONF, IOU, IOU_V)
            assert m.det_frames() == len(names) and m.frames() == 0
            seen.append(m.fetch_det())
        fr, rows, s = seen[0]
        for other in seen[1:]:
            assert other[0].tobytes() == fr.tobytes() and other[1].tobytes() == rows.tobytes()
        first = 0
        items = []
        for f, name in zip(fr, names):
            want_rows, want_tp, want_counts = golden_frame(g, name)
            labels = frame(name)[1]
            assert (int(f["candidates"]), int(f["ranked"]), int(f["kept"])) == want_counts, name
            assert int(f["labels"]) == labels.shape[0] and int(f["first_row"]) == first, name
            mine = rows[first:first + want_counts[2]]
            assert np.array_equal(bits(rows_of(mine)), bits(want_rows)), name
            assert np.array_equal(mine["tp"], want_tp), name
            first += want_counts[2]
            items.append((want_rows, want_tp, labels))
        assert rows.shape[0] == first == s["rows"] and s["frames"] == len(names)
        want = lib.det_ap(*dataset_arrays(items), n_iou=IOU_V.size)
        for k in ("labels", "classes", "grid_index", "precision", "recall", "map50", "map"):
            assert s[k] == want[k], k
        for k in ("class_id", "class_labels", "ap50", "ap", "tp", "fp"):
            assert np.array_equal(s[k], want[k]), k
        if tuple(names) == FRAMES:
            assert s["grid_index"] == int(g["ds_grid_index"]) and np.abs(np.array([s["precision"], s["recall"], s["map50"], s["map"]]) - g["ds_scores"]).max() <= 1e-12
        return s
    finally:
        m.close()
