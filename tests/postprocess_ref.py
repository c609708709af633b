"""Plain numpy restatement of the decode + NMS contract (TFLite_Detection_PostProcess, fast path, one class per
detection), for crafted head bytes: the reference of tests/test_gpu_postprocess.py (the HIP kernel) and of
tests/test_postprocess_ref_host.py (the C oracle's run_postprocess).  It shares no code with either: everything comes from the
container (anchors, thresholds, tensor quantisation, decode scales) and from quant.postprocess_tables, which test_quant_kat.py pins.

  per-anchor score = max over the C class columns of the float score; class = FIRST column holding that score (two class bytes on one
  plateau of the LOGISTIC table are one score); keep score >= threshold; stable sort by score, descending (ties: anchor order);
  centre-size decode with double intermediates and one rounding to float32 per quantity; float32 IoU, 0 when either area is not
  positive; suppress on IoU > threshold; stop at max_detections; rows above count are zero.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F = np.float32
OP_POSTPROCESS = 7
POST_CAP = 2048     # the kernel's constants, restated for rounds(): candidates per round,
POST_FAST = 1024    # counting-sort limit,
POST_THREADS = 1024  # threads per frame


class PostModel:
    """What the post-process op of a container reads: tables, anchors, thresholds and the ten per-level head tensors."""

    def __init__(self, path):
        from vbt_amd import quant
        from vbt_amd.container import Container
        c = Container(path)
        h = c.header
        self.path = path
        self.op_index = len(c.ops) - 1
        op = c.ops[self.op_index]
        assert int(op["type"]) == OP_POSTPROCESS
        n = int(op["n_inputs"])
        self.inputs = [int(t) for t in op["inputs"][:n]]            # class tensors of the levels, then their box tensors
        self.nl = n // 2
        self.A, self.maxdet = int(h["num_anchors"]), int(h["max_detections"])
        self.C = int(h["num_classes"]) or 1
        self.thr, self.iou = F(h["nms_score_threshold"]), F(h["nms_iou_threshold"])
        tc, tb = c.tensors[self.inputs[0]], c.tensors[self.inputs[self.nl]]
        scales = c.f32(int(op["aux2_off"]) + 256 * 4 * 2 + 256 * 8 * 2, 4)     # y, x, h, w: the end of the table blob
        assert scales[0] == scales[1] and scales[2] == scales[3]
        self.score, _, self.dq, self.ex = quant.postprocess_tables(float(tc["scale"]), int(tc["zero_point"]), float(tb["scale"]),
                                                                   int(tb["zero_point"]), float(scales[0]), float(scales[2]))
        self.anchors = c.f32(int(op["aux_off"]), self.A * 4).reshape(-1, 4).copy()      # ycenter, xcenter, h, w
        self.shapes = [(int(c.tensors[t]["h"]), int(c.tensors[t]["w"]), int(c.tensors[t]["c"])) for t in self.inputs]
        self.level_anchors = [hh * ww * cc // self.C for hh, ww, cc in self.shapes[:self.nl]]
        assert [hh * ww * cc // 4 for hh, ww, cc in self.shapes[self.nl:]] == self.level_anchors and sum(self.level_anchors) == self.A
        self.base = np.concatenate([[0], np.cumsum(self.level_anchors)]).astype(int)    # first anchor of each level, base[-1] = A
        q = np.nonzero(self.score >= self.thr)[0] - 128
        self.bmin = int(q.min()) if len(q) else 128                 # lowest class byte whose score reaches the threshold

    def to_levels(self, cls, box):
        """cls int8 [A, C], box int8 [A, 4] in anchor order -> the ten [h, w, c] tensors in the order of the op's inputs (channel =
        anchor_in_location * C + class, resp. * 4 + coordinate)."""
        cls, box = np.asarray(cls, np.int8).reshape(self.A, self.C), np.asarray(box, np.int8).reshape(self.A, 4)
        out = []
        for flat, shapes in ((cls, self.shapes[:self.nl]), (box, self.shapes[self.nl:])):
            for l, shp in enumerate(shapes):
                out.append(np.ascontiguousarray(flat[self.base[l]:self.base[l + 1]].reshape(shp)))
        return out

    def from_levels(self, tensors):
        cls = np.concatenate([np.asarray(t, np.int8).reshape(-1, self.C) for t in tensors[:self.nl]])
        box = np.concatenate([np.asarray(t, np.int8).reshape(-1, 4) for t in tensors[self.nl:]])
        return cls, box


def decode(m, box, idx):
    """Boxes [n, 4] float32 (ymin, xmin, ymax, xmax) of the anchors idx: DecodeCenterSizeBoxes."""
    an = m.anchors[idx].astype(np.float64)
    b = box[idx].astype(np.int64) + 128
    yc = (m.dq[b[:, 0]] * an[:, 2] + an[:, 0]).astype(F)
    xc = (m.dq[b[:, 1]] * an[:, 3] + an[:, 1]).astype(F)
    hh = (0.5 * m.ex[b[:, 2]] * an[:, 2]).astype(F)
    hw = (0.5 * m.ex[b[:, 3]] * an[:, 3]).astype(F)
    return np.stack([yc - hh, xc - hw, yc + hh, xc + hw], axis=1).astype(F)


def _suppressed(sel, sel_area, boxes, areas, thr):
    """[n] bool: IoU(sel, boxes[i]) > thr, every operation in float32 and in the order of detection_postprocess.cc."""
    ih = np.maximum(np.minimum(sel[2], boxes[:, 2]) - np.maximum(sel[0], boxes[:, 0]), F(0))
    iw = np.maximum(np.minimum(sel[3], boxes[:, 3]) - np.maximum(sel[1], boxes[:, 1]), F(0))
    inter = ih * iw
    with np.errstate(divide="ignore", invalid="ignore"):
        v = inter / ((sel_area + areas) - inter)
    return (sel_area > 0) & (areas > 0) & (v > thr)


def postprocess_ref(m, cls, box, chunk=512):
    """cls int8 [A, C], box int8 [A, 4] -> namespace: boxes [maxdet, 4], scores, classes [maxdet] float32, count; hist = [(score, number
    of candidates)] by descending score; n_cand; visited = how many positions of the sorted order were examined; selected = the
    surviving anchors in output order; order = every candidate anchor in sorted order."""
    cls, box = np.asarray(cls, np.int8).reshape(m.A, m.C), np.asarray(box, np.int8).reshape(m.A, 4)
    cols = m.score[cls.astype(np.int64) + 128]                   # [A, C] float32
    sc, cid = cols.max(axis=1), cols.argmax(axis=1)              # argmax: the first column holding the maximum
    idx = np.nonzero(sc >= m.thr)[0]
    order = idx[np.argsort(-sc[idx].astype(np.float64), kind="stable")]
    u, cnt = np.unique(sc[idx], return_counts=True)
    hist = [(float(a), int(b)) for a, b in zip(u[::-1], cnt[::-1])]
    selected, sel_box, sel_area = [], [], []
    visited = 0
    # the greedy walk, a chunk of the order at a time: first against what is selected already, then the chunk's own survivors one by one
    for c0 in range(0, len(order), chunk):
        if len(selected) == m.maxdet:
            break
        ids = order[c0:c0 + chunk]
        bx = decode(m, box, ids)
        ar = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
        dead = np.zeros(len(ids), bool)
        for s, sa in zip(sel_box, sel_area):
            dead |= _suppressed(s, sa, bx, ar, m.iou)
        visited = c0 + len(ids)
        while True:
            alive = np.nonzero(~dead)[0]
            if not len(alive):
                break
            j = int(alive[0])
            selected.append(int(ids[j]))
            sel_box.append(bx[j].copy())
            sel_area.append(ar[j])
            dead[j] = True
            if len(selected) == m.maxdet:
                visited = c0 + j + 1
                break
            dead[j + 1:] |= _suppressed(bx[j], ar[j], bx[j + 1:], ar[j + 1:], m.iou)
    n = len(selected)
    boxes, scores, classes = np.zeros((m.maxdet, 4), F), np.zeros(m.maxdet, F), np.zeros(m.maxdet, F)
    if n:
        boxes[:n] = np.stack(sel_box)
        scores[:n] = sc[selected]
        classes[:n] = cid[selected].astype(F)
    return SimpleNamespace(boxes=boxes, scores=scores, classes=classes, count=n, hist=hist, n_cand=len(order), visited=visited,
                           selected=selected, order=order, cand_score=sc[order])


def rounds(m, r):
    """The rounds the kernel's schedule (k_postprocess.hip: postprocess_kernel, step 3) must run for the reference result r, from the
    reference's histogram, order and `visited` alone: [(kind, n)] with kind 'count4' .. 'count1' (counting sort, threads per key),
    'bitonic', and the same with the prefix 'slice:' for a range of 2048 anchor indices of an oversized bin ('slice:empty': no
    candidate in it).  Ranks are added from the top while fewer than 256 candidates are held and the next bin still fits 2048; the
    walk ends with the round in which max_detections is reached."""
    out, pos, i = [], 0, 0
    hist = r.hist

    def kind(n):
        if n == 0:
            return "empty"
        return f"count{min(POST_THREADS // n, 4)}" if n <= POST_FAST else "bitonic"
    while i < len(hist):
        if hist[i][1] > POST_CAP:                                 # sliced by anchor index
            anchors = np.sort(r.order[pos:pos + hist[i][1]])
            for s0 in range(0, m.A, POST_CAP):
                n = int(((anchors >= s0) & (anchors < s0 + POST_CAP)).sum())
                out.append(("slice:" + kind(n), n))
                pos += n
                if r.count == m.maxdet and pos >= r.visited:
                    return out
            i += 1
            continue
        n = 0
        while i < len(hist) and n < 256 and n + hist[i][1] <= POST_CAP:
            n += hist[i][1]
            i += 1
        out.append((kind(n), n))
        pos += n
        if r.count == m.maxdet and pos >= r.visited:
            return out
    return out
