"""COCO detection metrics on the CPU: a numpy restatement of COCOeval's evaluateImg / accumulate / summarize for ONE category without
crowd boxes, written from the published behaviour of pycocotools' cocoeval.py as the literal loops (threshold, detection, ground truth),
not the way the device kernels are organised (vbt_amd/csrc/evaluate_coco.hip: a wavefront per image, one reduction per selection).

pycocotools is not installed where this suite runs, so this restatement is NOT pinned to the library.  It is pinned by
tests/test_coco_ref_host.py instead: a case worked out by hand, the two tables against np.linspace, and the recall denominators of the
reference's own training logs (tests/golden/coco_log_metrics.json), which show that the reference's evaluator saw the same 105 boxes in the
same area classes.  `cli eval --coco_dump` writes what pycocotools needs for a cross-check on a machine that has it.

Box contract (include/vbt_hip.h, "COCO metrics"), all in double: a detection's normalised float32 corners ymin,xmin,ymax,xmax and the
source size (H, W) give x = xmin W, y = ymin H, w = xmax W - x, h = ymax H - y; ground truth as integer VOC corners gives x = xmin,
y = ymin, w = xmax - xmin, h = ymax - ymin; area = w h for both (loadRes' bbox area); IoU is maskApi's bbIou on xywh.
An image: (boxes f32 [25,4], scores f32 [25], count, height, width, gt int [n,4] = ymin,xmin,ymax,xmax), as tests/test_gpu_eval.py.
"""
import numpy as np

# == np.linspace(.5, .95, 10): the step is (0.95 - 0.5) / 9 = 0.049999999999999996 in double, not the literal 0.45 / 9 (which rounds to
# 0.05 and differs from numpy at i = 7 and 8); the end point is the stop value itself
IOU_THRS = np.array([0.5 + i * ((0.95 - 0.5) / 9) for i in range(9)] + [0.95])
REC_THRS = np.array([i * 0.01 for i in range(100)] + [1.0])                       # == np.linspace(0, 1, 101); i / 100 is not
AREA_RNG = [(0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10)]      # all, small, medium, large
MAX_DETS = [1, 10, 100]
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "ARmax1", "ARmax10", "ARmax100", "ARs", "ARm", "ARl")
T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)


def det_xywh(boxes, height, width):
    """float32 normalised corners -> double [n,5] = x, y, w, h, area"""
    b = np.asarray(boxes, np.float32).reshape(-1, 4).astype(np.float64)
    x, y = b[:, 1] * float(width), b[:, 0] * float(height)
    w, h = b[:, 3] * float(width) - x, b[:, 2] * float(height) - y
    return np.stack([x, y, w, h, w * h], axis=1)


def gt_xywh(gt):
    g = np.asarray(gt, np.int64).reshape(-1, 4).astype(np.float64)
    w, h = g[:, 3] - g[:, 1], g[:, 2] - g[:, 0]
    return np.stack([g[:, 1], g[:, 0], w, h, w * h], axis=1)


def bb_iou(d, g):
    """maskApi.c bbIou, no crowd"""
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    return i / (d[2] * d[3] + g[2] * g[3] - i)


def evaluate_img(image):
    """evaluateImg for all four area ranges: None for an image with neither boxes nor detections, else a dict with
    scores f32 [nd] (descending, stable), det (original index) [nd], matched / ignored bool [A,T,nd], gt_ignore bool [A,ng]."""
    if isinstance(image, dict):             # boxes given as x, y, w, h, area already (what a COCO json file holds): no corner arithmetic
        d, g = np.asarray(image["det"], np.float64).reshape(-1, 5), np.asarray(image["gt"], np.float64).reshape(-1, 5)
        s, nd = np.asarray(image["scores"], np.float32), len(d)
    else:
        boxes, scores, count, height, width, gt = image
        nd = int(min(max(int(count), 0), 25))
        d = det_xywh(np.asarray(boxes)[:nd], height, width)
        s = np.asarray(scores, np.float32)[:nd]
        g = gt_xywh(gt)
    ng = len(g)
    if nd == 0 and ng == 0:
        return None
    dtind = np.argsort(-s.astype(np.float64), kind="mergesort")                  # (maxDets[-1] = 100 never cuts 25 detections)
    d, s = d[dtind], s[dtind]
    ious_all = np.zeros((nd, ng))
    for di in range(nd):
        for gi in range(ng):
            ious_all[di, gi] = bb_iou(d[di], g[gi])
    matched, ignored, gt_ignore = np.zeros((A, T, nd), bool), np.zeros((A, T, nd), bool), np.zeros((A, ng), bool)
    for a, (lo, hi) in enumerate(AREA_RNG):
        ig = np.array([bool(x[4] < lo or x[4] > hi) for x in g], bool)
        gtind = np.argsort(ig.astype(np.int64), kind="mergesort")               # non-ignored first, stable
        gt_ig = ig[gtind]
        ious = ious_all[:, gtind] if ng else ious_all
        gtm = np.zeros((T, ng), bool)
        for tind, t in enumerate(IOU_THRS):
            for dind in range(nd):
                iou = min(t, 1 - 1e-10)
                m = -1
                for gind in range(ng):
                    if gtm[tind, gind]:
                        continue
                    if m > -1 and not gt_ig[m] and gt_ig[gind]:
                        break
                    if ious[dind, gind] < iou:
                        continue
                    iou = ious[dind, gind]
                    m = gind
                if m == -1:
                    continue
                ignored[a, tind, dind] = gt_ig[m]
                matched[a, tind, dind] = True
                gtm[tind, m] = True
        out = np.array([bool(x[4] < lo or x[4] > hi) for x in d], bool).reshape(1, nd)
        ignored[a] = ignored[a] | (~matched[a] & out)
        gt_ignore[a] = ig
    return {"scores": s, "det": dtind, "matched": matched, "ignored": ignored, "gt_ignore": gt_ignore}


def mask_of(flags):
    """bool [A,T] -> the 40-bit mask, bit a * 10 + t"""
    v = 0
    for a in range(A):
        for t in range(T):
            if flags[a, t]:
                v |= 1 << (a * 10 + t)
    return v


def table(images):
    """rows in image order, inside an image by descending score: score f32, image i32, rank i32, matched u64, ignored u64; and
    n_gt int64 [A], n_images"""
    score, image, rank, matched, ignored = [], [], [], [], []
    n_gt = np.zeros(A, np.int64)
    for i, im in enumerate(images):
        e = evaluate_img(im)
        if e is None:
            continue
        n_gt += (~e["gt_ignore"]).sum(axis=1)
        for k in range(len(e["scores"])):
            score.append(e["scores"][k]); image.append(i); rank.append(k)
            matched.append(mask_of(e["matched"][:, :, k])); ignored.append(mask_of(e["ignored"][:, :, k]))
    return {"score": np.array(score, np.float32), "image": np.array(image, np.int32), "rank": np.array(rank, np.int32),
            "matched": np.array(matched, np.uint64), "ignored": np.array(ignored, np.uint64), "n_gt": n_gt, "n_images": len(images)}


def accumulate(tab):
    """precision [T,R,A,M], recall [T,A,M], scores [T,R,A,M] of COCOeval.accumulate (the category axis, of length 1, left out)"""
    precision, recall, scores = -np.ones((T, R, A, M)), -np.ones((T, A, M)), -np.ones((T, R, A, M))
    for a in range(A):
        for m, max_det in enumerate(MAX_DETS):
            sel = tab["rank"] < max_det                                         # e['dtScores'][0:maxDet] of every image, concatenated
            dt_scores = tab["score"][sel].astype(np.float64)
            inds = np.argsort(-dt_scores, kind="mergesort")
            sorted_scores = dt_scores[inds]
            npig = int(tab["n_gt"][a])
            if npig == 0:
                continue
            for t in range(T):
                bit = np.uint64(1 << (a * 10 + t))
                dtm = ((tab["matched"][sel] & bit) != 0)[inds]
                dt_ig = ((tab["ignored"][sel] & bit) != 0)[inds]
                tp = np.cumsum(dtm & ~dt_ig).astype(np.float64)
                fp = np.cumsum(~dtm & ~dt_ig).astype(np.float64)
                nd = len(tp)
                rc = tp / npig
                pr = (tp / (fp + tp + np.spacing(1))).tolist()
                q, ss = [0.0] * R, [0.0] * R
                recall[t, a, m] = rc[-1] if nd else 0
                for i in range(nd - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                pis = np.searchsorted(rc, REC_THRS, side="left")
                for ri, pi in enumerate(pis):
                    if pi >= nd:
                        break
                    q[ri] = pr[pi]
                    ss[ri] = sorted_scores[pi]
                precision[t, :, a, m] = q
                scores[t, :, a, m] = ss
    return precision, recall, scores


def summarize(precision, recall):
    """the 12 stats of COCOeval.summarize in its order: {name: value}; -1 where the slice has no entry above -1"""
    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if len(s) else -1.0
    stats = [mean(precision[:, :, 0, 2]), mean(precision[0, :, 0, 2]), mean(precision[5, :, 0, 2]), mean(precision[:, :, 1, 2]),
             mean(precision[:, :, 2, 2]), mean(precision[:, :, 3, 2]), mean(recall[:, 0, 0]), mean(recall[:, 0, 1]), mean(recall[:, 0, 2]),
             mean(recall[:, 1, 2]), mean(recall[:, 2, 2]), mean(recall[:, 3, 2])]
    return dict(zip(STAT_NAMES, stats))


def evaluate(images):
    """(table, precision, recall, scores, stats) of a list of images"""
    tab = table(images)
    precision, recall, scores = accumulate(tab)
    return tab, precision, recall, scores, summarize(precision, recall)


def pad(boxes, scores):
    b, s = np.zeros((25, 4), np.float32), np.zeros(25, np.float32)
    b[:len(boxes)] = np.asarray(boxes, np.float32).reshape(-1, 4)
    s[:len(scores)] = scores
    return b, s, len(scores)


def image_of(height, width, gt_xyxy, det_xyxy, scores):
    """an image from pixel corners (x1,y1,x2,y2): exact when height and width are powers of two"""
    g = np.asarray(gt_xyxy, np.int64).reshape(-1, 4)
    d = np.asarray(det_xyxy, np.float64).reshape(-1, 4)
    norm = np.stack([d[:, 1] / height, d[:, 0] / width, d[:, 3] / height, d[:, 2] / width], axis=1)
    return (*pad(norm, scores), height, width, g[:, [1, 0, 3, 2]].copy())


def hand_case():
    """the hand-worked image of tests/test_coco_ref_host.py"""
    return image_of(128, 128, [(16, 16, 64, 64), (80, 80, 110, 110)], [(16, 16, 64, 64), (70, 5, 95, 25), (87, 80, 117, 110)], [0.9, 0.8, 0.7])


HAND_STATS = {"AP": 61 / 101, "AP50": (51 + 50 * (2 / 3)) / 101, "AP75": 51 / 101, "APs": 0.15, "APm": 1.0, "APl": -1.0, "ARmax1": 0.5,
              "ARmax10": 0.65, "ARmax100": 0.65, "ARs": 0.3, "ARm": 1.0, "ARl": -1.0}
