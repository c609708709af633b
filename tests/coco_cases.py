"""Inputs of the COCO-metrics tests (tests/test_coco_ref_host.py on the CPU, tests/test_gpu_eval_coco.py on the GPU): crafted images, one
rule of COCOeval.evaluateImg each, and seeded sets.  An image is coco_ref's tuple (boxes f32 [25,4], scores f32 [25], count, height,
width, gt int [n,4]).  Crafted sizes are powers of two, so the normalised corners and their products with the size are exact."""
import json
import os

import numpy as np

import coco_ref as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def crafted():
    """{name: [image, ...]}"""
    out = {}
    out["hand-worked"] = [C.hand_case()]
    # two identical boxes: the detection takes the last one.  tie: the detection of score 0.9 has IoU 0.75 with both boxes and must take
    # the LAST; then the one of score 0.8 (IoU 1 with the first box, 0.5 with the last) still finds the first free at thresholds above 0.5
    out["identical boxes"] = [C.image_of(64, 64, [(8, 8, 24, 24), (8, 8, 24, 24)], [(8, 8, 24, 24), (8, 8, 24, 24), (8, 8, 24, 24)], [0.9, 0.8, 0.7])]
    out["tie takes the last"] = [C.image_of(64, 64, [(16, 16, 48, 40), (16, 24, 48, 48)], [(16, 16, 48, 48), (16, 16, 48, 40)], [0.9, 0.8])]
    # a small box (900) and a medium box (1600) under one detection (1225): IoU 900/1225 = 0.7347 and 1225/1600 = 0.7656.  medium range:
    # the walk ends at the ignored small box.  small range at t = 0.75: only the ignored medium box qualifies - matched, and ignored
    out["small and medium"] = [C.image_of(256, 256, [(10, 10, 40, 40), (10, 10, 50, 50)], [(10, 10, 45, 45)], [0.5])]
    out["unmatched outside the range"] = [C.image_of(256, 256, [(10, 10, 40, 40)], [(100, 100, 250, 250), (60, 60, 70, 70)], [0.9, 0.8])]
    out["iou exactly 0.5"] = [C.image_of(16, 16, [(0, 0, 8, 8)], [(0, 0, 8, 4)], [0.5])]
    out["iou exactly 1"] = [C.image_of(16, 16, [(2, 2, 10, 10)], [(2, 2, 10, 10)], [0.5])]
    out["areas on the range borders"] = [C.image_of(256, 256, [(0, 0, 32, 32), (100, 100, 196, 196)], [(0, 0, 32, 32), (100, 100, 196, 196)], [0.6, 0.7])]
    some = [(8, 8, 40, 40), (50, 50, 120, 100)]
    out["boxes without detections"] = [C.image_of(128, 128, some, [], []), C.image_of(128, 128, some, some[:1], [0.5])]
    out["detections without boxes"] = [C.image_of(128, 128, [], some, [0.5, 0.25]), C.image_of(128, 128, some, some[:1], [0.5])]
    out["neither"] = [C.image_of(128, 128, [], [], []), C.image_of(128, 128, some, some, [0.5, 0.75]), C.image_of(64, 64, [], [], [])]
    # unsorted scores inside an image (with a tie and a -0.0 / +0.0 pair), equal scores across images: both sorts are stable
    a = C.image_of(128, 128, some, [(8, 8, 40, 44), (50, 50, 120, 100), (8, 8, 40, 40), (0, 0, 5, 5), (1, 1, 6, 6)], [0.25, 0.5, 0.5, -0.0, 0.0])
    b = C.image_of(128, 128, some[:1], [(60, 60, 70, 70), (8, 8, 40, 40), (8, 8, 36, 40)], [0.5, 0.25, 0.5])
    out["stable sorts"] = [a, b, a]
    rng = np.random.Generator(np.random.PCG64(5))
    gts = [(10, 10, 40, 40), (60, 60, 110, 110), (120, 20, 250, 200)]
    dets = []
    for k in range(25):
        g = gts[k % 3]
        dets.append(tuple(np.asarray(g) + rng.integers(-6, 7, 4)))
    out["25 detections on 3 boxes"] = [C.image_of(256, 256, gts, dets, (rng.integers(1, 256, 25) / 256).astype(np.float32))]
    big = [(16 * (i % 8) + 1, 16 * (i // 8) + 1, 16 * (i % 8) + 1 + 6 + (i % 9), 16 * (i // 8) + 1 + 6 + (i % 7)) for i in range(64)]
    pick = [big[i] for i in (63, 5, 17, 17, 40, 0)] + [(1, 1, 100, 100)]
    out["64 boxes"] = [C.image_of(128, 128, big, pick, [0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3])]
    out["xmax below xmin"] = [C.image_of(128, 128, some, [(40, 8, 8, 40), (8, 8, 40, 40), (120, 100, 50, 50)], [0.9, 0.8, 0.7])]
    return out


def annotations():
    return json.load(open(os.path.join(GOLDEN, "eval_annotations.json")))["images"]


def annotated(seed=2025):
    """the reference's 61 annotated images with seeded detections: each box kept with probability 0.85 and jittered by
    N(0, 0.08 side), scores k / 256, plus 0 to 5 random boxes per image"""
    rng = np.random.Generator(np.random.PCG64(seed))
    images = []
    for a in annotations():
        h, w = a["height"], a["width"]
        gt = np.asarray(a["boxes"], np.int64).reshape(-1, 4)
        dets = []
        for y0, x0, y1, x1 in gt:
            if rng.random() < 0.85:
                sy, sx = 0.08 * (y1 - y0), 0.08 * (x1 - x0)
                dets.append([(y0 + rng.normal(0, sy)) / h, (x0 + rng.normal(0, sx)) / w, (y1 + rng.normal(0, sy)) / h, (x1 + rng.normal(0, sx)) / w])
        for _ in range(int(rng.integers(0, 6))):
            y0, x0 = rng.random() * 0.8, rng.random() * 0.8
            dets.append([y0, x0, y0 + rng.random() * 0.2, x0 + rng.random() * 0.2])
        dets = np.asarray(dets[:25], np.float32).reshape(-1, 4)
        scores = (rng.integers(0, 256, len(dets)) / 256).astype(np.float32)
        images.append((*C.pad(dets, scores), h, w, gt))
    return images


def seeded(n=64, seed=77):
    """n images of 0 to 25 detections and 0 to 8 boxes on 256 x 512; detections around the boxes or anywhere, coarse scores"""
    rng = np.random.Generator(np.random.PCG64(seed))
    images = []
    for _ in range(n):
        h, w = 256, 512
        ng, nd = int(rng.integers(0, 9)), int(rng.integers(0, 26))
        gt = []
        for _ in range(ng):
            side = int(rng.choice([12, 28, 60, 120]))
            y0, x0 = int(rng.integers(0, h - side)), int(rng.integers(0, w - side))
            gt.append([y0, x0, y0 + side + int(rng.integers(0, 8)), x0 + side + int(rng.integers(0, 8))])
        gt = np.asarray(gt, np.int64).reshape(-1, 4)
        dets = []
        for _ in range(nd):
            if ng and rng.random() < 0.7:
                g = gt[int(rng.integers(0, ng))]
                d = g + rng.integers(-4, 5, 4)
            else:
                y0, x0 = int(rng.integers(0, h - 40)), int(rng.integers(0, w - 40))
                d = np.array([y0, x0, y0 + int(rng.integers(4, 40)), x0 + int(rng.integers(4, 40))])
            dets.append(d / np.array([h, w, h, w]))
        dets = np.asarray(dets, np.float32).reshape(-1, 4)
        images.append((*C.pad(dets, (rng.integers(0, 32, nd) / 32).astype(np.float32)), h, w, gt))
    return images


def write_case(path, images, result=None):
    """the case file of tests/fuzz/coco_check.cc"""
    tab, precision, recall, _, stats = result if result is not None else C.evaluate(images)
    with open(path, "wb") as f:
        f.write(np.int32(len(images)).tobytes())
        for im in images:
            boxes, scores, count, h, w, gt = im
            gt = np.asarray(gt, np.int32).reshape(-1, 4)
            f.write(np.array([count, h, w, len(gt)], np.int32).tobytes())
            f.write(np.ascontiguousarray(boxes, np.float32).tobytes() + np.ascontiguousarray(scores, np.float32).tobytes() + gt.tobytes())
            e = C.evaluate_img(im)
            if e is None:
                f.write(np.int32(0).tobytes() + np.zeros(4, np.int32).tobytes())
                continue
            nd = len(e["scores"])
            f.write(np.int32(nd).tobytes() + e["scores"].astype(np.float32).tobytes() + e["det"].astype(np.int32).tobytes())
            f.write(np.array([C.mask_of(e["matched"][:, :, k]) for k in range(nd)], np.uint64).tobytes())
            f.write(np.array([C.mask_of(e["ignored"][:, :, k]) for k in range(nd)], np.uint64).tobytes())
            f.write((~e["gt_ignore"]).sum(axis=1).astype(np.int32).tobytes())
        f.write(C.IOU_THRS.tobytes() + C.REC_THRS.tobytes() + np.ascontiguousarray(precision).tobytes() + np.ascontiguousarray(recall).tobytes())
        f.write(np.array([stats[k] for k in C.STAT_NAMES], np.float64).tobytes())
