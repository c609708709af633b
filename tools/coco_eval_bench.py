#!/usr/bin/env python3
"""Cost of the COCO metrics (vbt_coco_*, vbt_amd/csrc/evaluate_coco.hip) against the numpy restatement of the tests (tests/coco_ref.py):
on the reference's 61 annotated images with seeded detections (tests/coco_cases.py annotated()) and on a seeded set of --large images
(coco_cases.seeded).  The detections are on the device before the clock starts, as the detector leaves them there.
  device      wall time of all vbt_coco_add_detections calls (batches of 64) + vbt_coco_accumulate with its read-back, from an empty
              handle (vbt_coco_reset outside the window); `match` and `accumulate`: the two halves, each ended by a synchronisation
  restatement wall time of coco_ref.evaluate on the same images (the literal loops, one thread); --ref_reps rounds on the large set
The arrays and the 12 stats of the two are compared (`equal_to_restatement`).  Median, minimum and maximum of --reps rounds after --warmup.

  python tools/coco_eval_bench.py [--reps 7] [--warmup 2] [--large 4096] [--ref_reps 7] [--out FILE.json]

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mjpeg_bench import spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--large", type=int, default=4096)
    ap.add_argument("--ref_reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import coco_cases as K
    import coco_ref as C
    from vbt_amd import _lib, evaluate
    from vbt_amd.mem import DeviceBuffer
    L = _lib.lib()
    if L.vbt_device_count() < 1:
        raise SystemExit("coco_eval_bench: no GPU - a timing taken anywhere else says nothing")
    res = {"reps": args.reps, "batch": evaluate.BATCH}
    for name, images, ref_reps in (("annotated_61", K.annotated(), args.reps), (f"seeded_{args.large}", K.seeded(args.large), args.ref_reps)):
        n = len(images)
        parts = []
        for i0 in range(0, n, evaluate.BATCH):
            part = images[i0:i0 + evaluate.BATCH]
            bufs = [DeviceBuffer.from_host(np.stack([np.asarray(im[k], dt).reshape(shp) for im in part]))
                    for k, dt, shp in ((0, np.float32, (25, 4)), (1, np.float32, (25,)), (2, np.int32, ()))]
            parts.append((bufs, [(im[3], im[4]) for im in part], [im[5] for im in part]))
        ev = evaluate.CocoEvaluator(n * evaluate.MAX_DETECTIONS, evaluate.BATCH)
        t_ref = []
        for _ in range(max(1, ref_reps)):
            t0 = time.perf_counter()
            tab, precision, recall, scores, stats = C.evaluate(images)
            t_ref.append(time.perf_counter() - t0)
        t_all, t_match, t_acc = [], [], []
        for r in range(args.warmup + args.reps):
            ev.reset()
            t0 = time.perf_counter()
            for bufs, hw, gts in parts:
                ev.add(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, hw, gts)
            _lib.check(L.vbt_device_synchronize(0))
            t1 = time.perf_counter()
            got = ev.accumulate()
            t2 = time.perf_counter()
            if r >= args.warmup:
                t_all.append(t2 - t0); t_match.append(t1 - t0); t_acc.append(t2 - t1)
        equal = bool(np.array_equal(got.precision, precision) and np.array_equal(got.recall, recall) and np.array_equal(got.scores, scores) and
                     np.array_equal(got.n_gt, tab["n_gt"]) and max(abs(got.stats[k] - stats[k]) for k in C.STAT_NAMES) <= 1e-12)
        res[name] = {"images": n, "rows": got.n_rows, "n_gt": got.n_gt.tolist(), "AP": got.stats["AP"], "equal_to_restatement": equal,
                     "device_ms": spread([v * 1e3 for v in t_all]), "match_ms": spread([v * 1e3 for v in t_match]),
                     "accumulate_ms": spread([v * 1e3 for v in t_acc]), "restatement_s": spread(t_ref), "restatement_rounds": len(t_ref)}
        del ev, parts
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
