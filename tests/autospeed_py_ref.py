"""Restatement of the reference's PYTHON AutoSpeed wrapper, Models/inference/auto_speed_infer.py AutoSpeedNetworkInfer, around a raw detector tensor:
what infer.AutoSpeedNetworkInfer and the vp_detect_*_pil / _agnostic stages are held to.  Pillow does the resize itself; everything else is
torch / numpy fp32 on the CPU, statement for statement.  tools/pin_autospeed_py.py runs the reference class's own method bodies against this file at
distance 0.0 and writes tests/golden/autospeed_py.npz.  torchvision.ops.nms is restated from its published rule (torchvision is not installed where
the pin runs): PARITY UNPINNED, DESIGN.md section 4.
"""
import numpy as np
import torch
from PIL import Image

TRAIN_SIZE = (1024, 512)       # target width, height (:7)
CONF, IOU = 0.6, 0.45          # post_process_predictions' defaults (:63)


def letterbox_geometry(orig_w, orig_h, train_size=TRAIN_SIZE):
    """resize_letterbox :24-34 without the image: (scale, new_w, new_h, pad_x, pad_y); scale is a Python float (a double)."""
    target_w, target_h = train_size
    scale = min(target_w / orig_w, target_h / orig_h)
    new_w, new_h = int(orig_w * scale), int(orig_h * scale)
    return scale, new_w, new_h, (target_w - new_w) // 2, (target_h - new_h) // 2


def letterbox_pil(image, train_size=TRAIN_SIZE):
    """resize_letterbox + ToTensor (:24-42, without the .half() the reference needs for its half model): PIL RGB image ->
    ([3][target_h][target_w] float32, (scale, pad_x, pad_y)).  ToTensor is uint8 -> float32, one division by 255."""
    scale, new_w, new_h, pad_x, pad_y = letterbox_geometry(*image.size, train_size)
    img_resized = image.resize((new_w, new_h), Image.BILINEAR)
    padded = Image.new("RGB", train_size, (114, 114, 114))
    padded.paste(img_resized, (pad_x, pad_y))
    t = np.asarray(padded).astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    return np.ascontiguousarray(t), (scale, pad_x, pad_y)


def nms(boxes, scores, iou_thres):
    """torchvision.ops.nms as published (torchvision/csrc/ops/cpu/nms_kernel.cpp): boxes by descending score (stable: equal scores in index order),
    a kept box i suppresses every later j with inter / (area_i + area_j - inter) > iou_thres, areas and intersections on the corner boxes
    without +1, all in the boxes' dtype; the comparison promotes the ratio to the double threshold.  Returns the kept indices in that order."""
    b = np.asarray(boxes, np.float32)
    order = np.argsort(-np.asarray(scores, np.float32), kind="stable")
    x1, y1, x2, y2 = (b[order, k] for k in range(4))
    areas = (x2 - x1) * (y2 - y1)
    dead = np.zeros(len(order), bool)
    keep = []
    for i in range(len(order)):
        if dead[i]:
            continue
        keep.append(int(order[i]))
        w = np.maximum(np.float32(0), np.minimum(x2[i], x2[i + 1:]) - np.maximum(x1[i], x1[i + 1:]))
        h = np.maximum(np.float32(0), np.minimum(y2[i], y2[i + 1:]) - np.maximum(y1[i], y1[i + 1:]))
        inter = w * h
        with np.errstate(invalid="ignore", divide="ignore"):
            ovr = inter / (areas[i] + areas[i + 1:] - inter)
        dead[i + 1:] |= ovr.astype(np.float64) > iou_thres
    return np.array(keep, np.int64)


def xywh2xyxy(x):
    """:45-52"""
    y = x.clone()
    y[:, 0] = x[:, 0] - x[:, 2] / 2
    y[:, 1] = x[:, 1] - x[:, 3] / 2
    y[:, 2] = x[:, 0] + x[:, 2] / 2
    y[:, 3] = x[:, 1] + x[:, 3] / 2
    return y


def post_process(raw, conf=CONF, iou=IOU):
    """post_process_predictions + nms (:54-83): raw [4 + nc][boxes] float32 -> torch [n][6] rows x1, y1, x2, y2, score, class in LETTERBOX pixels,
    kept order.  The class scores go through a sigmoid here although the head already applied one (:69)."""
    predictions = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32)).permute(1, 0)
    boxes = predictions[:, :4]
    scores, class_ids = torch.max(predictions[:, 4:].sigmoid(), dim=1)
    mask = scores > conf
    if mask.sum() == 0:
        return torch.empty(0, 6)
    combined = torch.cat([xywh2xyxy(boxes[mask]), scores[mask].unsqueeze(1), class_ids[mask].float().unsqueeze(1)], dim=1)
    return combined[torch.from_numpy(nms(combined[:, :4].numpy(), combined[:, 4].numpy(), iou))]


def back_map(predictions, scale, pad_x, pad_y, orig_w, orig_h):
    """inference :97-108: letterbox pixels -> original image, clamped; a list of [x1, y1, x2, y2, score, class] lists."""
    if predictions.numel() == 0:
        return []
    predictions = predictions.clone()
    predictions[:, [0, 2]] = (predictions[:, [0, 2]] - pad_x) / scale
    predictions[:, [1, 3]] = (predictions[:, [1, 3]] - pad_y) / scale
    predictions[:, [0, 2]] = predictions[:, [0, 2]].clamp(0, orig_w)
    predictions[:, [1, 3]] = predictions[:, [1, 3]].clamp(0, orig_h)
    return predictions.tolist()


def decode(raw, geometry, orig_w, orig_h, conf=CONF, iou=IOU):
    """post_process + back_map as float32 rows [n][6] ([0][6] when nothing is kept); geometry = (scale, pad_x, pad_y)."""
    rows = back_map(post_process(raw, conf, iou), geometry[0], geometry[1], geometry[2], orig_w, orig_h)
    return np.array(rows, np.float32).reshape(-1, 6)


def candidate_iou_gap(raw, conf, iou):
    """smallest | IoU - iou | over all pairs of candidates (score > conf), and the smallest | sigmoid(score) - conf | over all class scores:
    the margins a fixture frame must keep for an engine within 1e-3 to keep the same set."""
    s = torch.from_numpy(np.ascontiguousarray(raw[4:], dtype=np.float32)).sigmoid().numpy()
    score_gap = float(np.abs(s.astype(np.float64) - conf).min())
    m = s.max(axis=0) > np.float32(conf)
    b = xywh2xyxy(torch.from_numpy(np.ascontiguousarray(raw[:4, m].T, dtype=np.float32))).numpy()
    gap = 1.0
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    for i in range(len(b) - 1):
        w = np.maximum(np.float32(0), np.minimum(b[i, 2], b[i + 1:, 2]) - np.maximum(b[i, 0], b[i + 1:, 0]))
        h = np.maximum(np.float32(0), np.minimum(b[i, 3], b[i + 1:, 3]) - np.maximum(b[i, 1], b[i + 1:, 1]))
        inter = w * h
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = min(gap, float(np.nanmin(np.abs((inter / (area[i] + area[i + 1:] - inter)).astype(np.float64) - iou))))
    return score_gap, gap, int(m.sum())
