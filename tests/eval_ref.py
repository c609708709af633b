"""CPU restatement of the detector evaluation for the tests (numpy + scipy's linear_sum_assignment), written from the behaviour of
the reference's eval.py and of the scikit-learn functions it calls - the yardstick of tests/test_eval_host.py and
tests/test_gpu_eval.py.  tests/test_eval_host.py pins it to scikit-learn's own output on the reference's own table
(tests/golden/eval_curves_ref.npz), so the GPU tests may use it on tables scikit-learn never saw.

Degenerate tables follow the rule of include/vbt_hip.h: a rate whose denominator is zero is NaN, and so is a scalar built on it
(no positive label: recall, tpr, AP, AUC; no negative label: fpr, AUC)."""
import numpy as np

NO_POSITIVES, NO_NEGATIVES = 1, 2


def scale_boxes(boxes, height, width):
    """Normalised float32 [n,4] ymin,xmin,ymax,xmax -> integer pixel boxes: double product with (h, w, h, w), truncated to int64."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4).astype(np.float64)
    return (b * np.array([height / 1.0, width / 1.0] * 2)).astype(np.int64)


def iou_int(det, gt):
    det, gt = [int(v) for v in det], [int(v) for v in gt]
    ih = max(0, min(det[2], gt[2]) - max(det[0], gt[0]))
    iw = max(0, min(det[3], gt[3]) - max(det[1], gt[1]))
    inter = ih * iw
    union = (det[2] - det[0]) * (det[3] - det[1]) + (gt[2] - gt[0]) * (gt[3] - gt[1]) - inter
    return float(np.float64(inter) / np.float64(union)) if union > 0 else 0.0


def iou_matrix(gt, det):
    gt, det = np.asarray(gt, np.int64).reshape(-1, 4), np.asarray(det, np.int64).reshape(-1, 4)
    m = np.zeros((len(gt), len(det)))
    for i in range(len(gt)):
        for j in range(len(det)):
            m[i, j] = iou_int(det[j], gt[i])
    return m


def match(gt, det):
    """(gt_idx, det_idx, iou) of one image: square padded IoU matrix, scipy's assignment on 1 - IoU, assignments to padding COLUMNS
    dropped, rows kept in row order (a gt_idx >= len(gt) is a padding row)."""
    from scipy.optimize import linear_sum_assignment
    m = iou_matrix(gt, det)
    n_gt, n_pred = m.shape
    n = max(n_gt, n_pred)
    sq = np.zeros((n, n))
    sq[:n_gt, :n_pred] = m
    rows, cols = linear_sum_assignment(1 - sq)
    keep = cols < n_pred
    return rows[keep].astype(np.int32), cols[keep].astype(np.int32), sq[rows[keep], cols[keep]]


def match_image(boxes, scores, count, height, width, gt):
    """one image of the table: (score f32, iou f64, det_idx i32, gt_idx i32) from the detector's outputs at threshold 0"""
    n = int(min(max(int(count), 0), 25))
    det = scale_boxes(np.asarray(boxes)[:n], height, width)
    gi, di, iou = match(gt, det)
    return np.asarray(scores, np.float32)[di], iou, di, gi


class Curves:
    pass


def curves(scores, ious, iou_threshold):
    scores = np.asarray(scores, np.float32)
    label = np.asarray(ious, np.float64) > iou_threshold
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    s, lab = scores[order], label[order]
    n = len(s)
    last = np.r_[np.nonzero(s[1:] != s[:-1])[0], n - 1].astype(np.int64) if n else np.zeros(0, np.int64)
    tps = np.cumsum(lab.astype(np.int64))[last] if n else np.zeros(0, np.int64)
    fps = 1 + last - tps
    thr = s[last]
    n_pos, n_neg = int(label.sum()), int(n - label.sum())
    c = Curves()
    c.n_rows, c.n_pos, c.n_neg = n, n_pos, n_neg
    c.flags = (NO_POSITIVES if n_pos == 0 else 0) | (NO_NEGATIVES if n_neg == 0 else 0)
    f8 = np.float64
    with np.errstate(invalid="ignore", divide="ignore"):
        prec = tps.astype(f8) / (tps + fps).astype(f8)
        rec = tps.astype(f8) / f8(n_pos) if n_pos else np.full(len(tps), np.nan)
        c.precision, c.recall, c.pr_thresholds = np.r_[prec[::-1], 1.0], np.r_[rec[::-1], 0.0], thr[::-1].copy()
        c.ap = max(0.0, float(-np.sum(np.diff(c.recall) * c.precision[:-1]))) if n_pos else float("nan")
        keep = np.ones(len(tps), bool)
        if len(tps) > 2:
            keep[1:-1] = (np.diff(fps, 2) != 0) | (np.diff(tps, 2) != 0)
        rf, rt = np.r_[0, fps[keep]].astype(f8), np.r_[0, tps[keep]].astype(f8)
        c.fpr = rf / f8(n_neg) if n_neg else np.full(len(rf), np.nan)
        c.tpr = rt / f8(n_pos) if n_pos else np.full(len(rt), np.nan)
        c.roc_thresholds = np.r_[np.float32(np.inf), thr[keep]].astype(np.float32)
        c.auc = float(np.sum(np.diff(c.fpr) * (c.tpr[1:] + c.tpr[:-1]) / 2.0)) if n_pos and n_neg else float("nan")
    return c
