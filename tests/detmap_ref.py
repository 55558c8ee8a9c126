"""A numpy restatement of the detector's validation chain as include/vp_hip.h defines it ("vp_metric: the detector's validation mAP"): candidates, rank,
class-offset suppression, the tp words of the matching, and the dataset scores.  tests/test_detmap_host.py holds it to tests/golden/detmap.npz (the
reference's own code, run by tools/pin_detmap.py); the GPU tests and tools/bench_detmap.py use it where the fixture has no vector.  fp32 stages use one
numpy float32 operation per operation of the definition; the dataset scores are double."""
import numpy as np

MAX_WH = np.float32(7680.0)
F = np.float32


def validate(raw, conf=0.001, iou=0.65, max_nms=30000, max_det=300):
    """raw fp32 [4 + nc][nb] -> (rows [kept][6] x1, y1, x2, y2, score, cls; counts (candidates, ranked, kept))"""
    raw = np.asarray(raw, np.float32)
    sc = raw[4:].T                                                  # [nb][nc]: candidate order is box major, class minor
    with np.errstate(invalid="ignore"):
        i, c = np.nonzero(sc > F(conf))                             # a NaN is no candidate
    s = sc[i, c]
    candidates = int(s.size)
    order = np.argsort(-s, kind="stable")[:max_nms]                 # equal scores keep candidate order
    i, c, s = i[order], c[order], s[order]
    cx, cy, w, h = raw[0][i], raw[1][i], raw[2][i], raw[3][i]
    box = np.stack((cx - w / F(2), cy - h / F(2), cx + w / F(2), cy + h / F(2)), 1).astype(np.float32)
    off = (c.astype(np.float32) * MAX_WH)[:, None]
    keep = greedy(box + off, F(iou), max_det)
    rows = np.concatenate((box[keep], s[keep, None], c[keep, None].astype(np.float32)), 1).astype(np.float32).reshape(-1, 6)
    return rows, (candidates, int(s.size), int(len(keep)))


def greedy(b, thr, max_det):
    """torchvision's rule on boxes in rank order, stopped at max_det kept: fmax / fmin as the device's fmaxf / fminf, 0 / 0 = NaN suppresses nothing"""
    n = b.shape[0]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = np.zeros(n, bool)
    keep = []
    for k in range(n):
        if dead[k]:
            continue
        keep.append(k)
        if len(keep) == max_det:
            break
        r = b[k + 1:]
        iw = np.fmax(F(0), np.fmin(b[k, 2], r[:, 2]) - np.fmax(b[k, 0], r[:, 0]))
        ih = np.fmax(F(0), np.fmin(b[k, 3], r[:, 3]) - np.fmax(b[k, 1], r[:, 1]))
        inter = iw * ih
        with np.errstate(invalid="ignore", divide="ignore"):
            ovr = inter / ((area[k] + area[k + 1:]) - inter)
            dead[k + 1:] |= ovr > thr
    return np.array(keep, np.int64)


def pair_iou(rows, labels_px):
    """fp32 [labels][rows]: the matching's IoU, NaN-propagating as torch.min / torch.max / clamp are"""
    rows = np.asarray(rows, np.float32).reshape(-1, 6)
    lb = np.asarray(labels_px, np.float32).reshape(-1, 5)
    a1, a2, b1, b2 = lb[:, None, 1:3], lb[:, None, 3:5], rows[None, :, 0:2], rows[None, :, 2:4]
    with np.errstate(invalid="ignore", divide="ignore"):
        side = np.minimum(a2, b2) - np.maximum(a1, b1)
        side = np.where(side < 0, F(0), side)
        inter = side[..., 0] * side[..., 1]
        area_l = (a2 - a1)[..., 0] * (a2 - a1)[..., 1]
        area_d = (b2 - b1)[..., 0] * (b2 - b1)[..., 1]
        return inter / (((area_l + area_d) - inter) + F(1e-7))


def match(rows, labels_px, iou_v):
    """tp word per kept row.  labels_px: rows [cls, x1, y1, x2, y2] in pixels.  The best label of a detection is its same-class label of highest IoU
    (the first of equals); among the detections eligible at a threshold that share a best label, the one of lowest index is correct."""
    rows = np.asarray(rows, np.float32).reshape(-1, 6)
    lb = np.asarray(labels_px, np.float32).reshape(-1, 5)
    tp = np.zeros(rows.shape[0], np.uint32)
    if not rows.shape[0] or not lb.shape[0]:
        return tp
    iou = pair_iou(rows, lb)
    assert iou.dtype == np.float32
    same = lb[:, None, 0] == rows[None, :, 5]
    cand = np.where(same & ~np.isnan(iou), iou, F(-np.inf))
    best_lab = np.argmax(cand, 0)                                    # the first maximum
    best_iou = cand[best_lab, np.arange(rows.shape[0])]
    has = np.isfinite(best_iou) | (best_iou == np.inf)
    for t, thr in enumerate(np.asarray(iou_v, np.float32)):
        ok = has & (best_iou >= thr)
        taken = set()
        for d in np.nonzero(ok)[0]:
            if best_lab[d] not in taken:
                taken.add(best_lab[d])
                tp[d] |= np.uint32(1 << t)
    return tp


def interp(x, xp, fp, left, right):
    return np.interp(x, xp, fp, left=left, right=right)


def dataset_scores(tp, conf, det_cls, label_cls, n_iou=10):
    """the dataset scores in double, as the header states them; tp: words, bit t = correct at threshold t"""
    tp = np.asarray(tp, np.uint32).reshape(-1)
    conf = np.asarray(conf, np.float32).reshape(-1)
    det_cls = np.asarray(det_cls, np.float32).reshape(-1)
    classes, nt = np.unique(np.asarray(label_cls, np.float32).reshape(-1), return_counts=True)
    nc = classes.size
    out = {"classes": classes, "class_labels": nt, "grid_index": -1, "precision": 0.0, "recall": 0.0, "map50": 0.0, "map": 0.0, "ap50": np.zeros(nc),
           "ap": np.zeros(nc), "tp": np.zeros(nc), "fp": np.zeros(nc)}
    hit = ((tp[:, None] >> np.arange(n_iou, dtype=np.uint32)[None, :]) & 1).astype(np.int64)      # [rows][n_iou]
    if not hit.any() or nc == 0:
        return out
    order = np.argsort(-conf, kind="stable")
    hit, conf, det_cls = hit[order], conf[order], det_cls[order]
    grid = np.linspace(0.0, 1.0, 1000)
    x101 = np.linspace(0.0, 1.0, 101)
    eps = 1e-16
    p = np.zeros((nc, 1000))
    r = np.zeros((nc, 1000))
    ap = np.zeros((nc, n_iou))
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    for k, c in enumerate(classes):
        sel = det_cls == c
        if not sel.any() or nt[k] == 0:
            continue
        tpc = hit[sel].cumsum(0)
        fpc = (1 - hit[sel]).cumsum(0)
        rec = tpc / (nt[k] + eps)
        pre = tpc / (tpc + fpc)
        neg = -conf[sel].astype(np.float64)
        r[k] = interp(-grid, neg, rec[:, 0], 0.0, None)
        p[k] = interp(-grid, neg, pre[:, 0], 1.0, None)
        for j in range(n_iou):
            xr = np.concatenate(([0.0], rec[:, j], [1.0]))
            env = np.concatenate(([1.0], pre[:, j], [0.0]))
            env = np.maximum.accumulate(env[::-1])[::-1]
            ap[k, j] = trapezoid(np.interp(x101, xr, env), x101)
    f1 = 2 * p * r / (p + r + eps)
    curve = f1.mean(0)
    taps = 101
    padded = np.concatenate((np.full(taps // 2, curve[0]), curve, np.full(taps // 2, curve[-1])))
    smooth = np.convolve(padded, np.ones(taps) / taps, mode="valid")
    g = int(smooth.argmax())
    tpv = (r[:, g] * nt).round()
    fpv = (tpv / (p[:, g] + eps) - tpv).round()
    out.update(grid_index=g, precision=float(p[:, g].mean()), recall=float(r[:, g].mean()), map50=float(ap[:, 0].mean()), map=float(ap.mean(1).mean()), ap50=ap[:, 0],
               ap=ap.mean(1), tp=tpv, fp=fpv, smooth=smooth)
    return out


def run_frame(raw, labels_px, iou_v, conf=0.001, iou=0.65):
    rows, counts = validate(raw, conf, iou)
    return rows, match(rows, labels_px, iou_v), counts
