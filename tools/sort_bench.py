#!/usr/bin/env python3
"""The tracker walk alone, SORT against OC-SORT, on the load behind bench.py's `clip1_reference_boxes` split (bench.py itself
untouched): clip 001's boxes from tests/golden/dfs_ocsort_all.npz as detector outputs, 64 frames per launch of the time-batched walk
(vbt_tracker_update_from_detections_seq), then the clip close.

Two fresh trackers - MultiClipTracker(max_age=30, asso_func="diou", iou_threshold=0.1) as reference track.py:157 and
MultiClipSortTracker(max_age=30) as track.py:156 - run the same load in the same process.  Each is warmed up once (code objects, the
LDS opt-in of the walk), then the two alternate --reps times; every repetition is reset + walk + close between two device
synchronisations, timed with the host clock.  Prints one JSON line: us per stepped frame of both (median, min, max) and their ratio.

  python tools/sort_bench.py [--reps 9] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (sets the queue count before HIP starts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames-per-launch", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from vbt_amd import _lib
    from vbt_amd.ocsort import MultiClipTracker
    from vbt_amd.sort import MultiClipSortTracker
    L = _lib.lib()
    a = np.load(os.path.join(ROOT, "tests", "golden", "dfs_ocsort_all.npz"))
    fps = float(json.load(open(bench.CORPUS_META))["001"][1])
    g = {k: a[f"c001_{k}"] for k in ("time", "x", "y", "norm_plate_height", "norm_plate_width")}
    fno = np.rint(g["time"] * fps).astype(np.int64)                  # 1-based frame numbers (time = frame_count / fps, track.py:161,169)
    T = int(fno.max())
    boxes, scores, counts = np.zeros((T, 25, 4), np.float32), np.zeros((T, 25), np.float32), np.zeros(T, np.int32)
    for f, x, y, h, w in zip(fno, g["x"], g["y"], g["norm_plate_height"], g["norm_plate_width"]):
        i = counts[f - 1]
        boxes[f - 1, i] = (y - h / 2, x - w / 2, y + h / 2, x + w / 2)   # detector layout ymin,xmin,ymax,xmax (odt.py:64-66)
        scores[f - 1, i] = 0.9
        counts[f - 1] = i + 1
    db, ds, dc = (torch.from_numpy(v).to("cuda:0") for v in (boxes, scores, counts))
    stream = torch.cuda.current_stream().cuda_stream
    stepped = int((counts > 0).sum())
    F = args.frames_per_launch
    trackers = {"ocsort": MultiClipTracker(1, 8 * T + 75, max_age=30, asso_func="diou", iou_threshold=0.1),
                "sort": MultiClipSortTracker(1, 8 * T + 75, max_age=30)}
    res = {}

    def run(name):
        trk = trackers[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trk.reset()
        for f0 in range(0, T, F):
            run_ = (_lib.Run * 1)(_lib.Run(0, f0, 1, min(F, T - f0), f0 + 1, 1, fps))
            _lib.check(L.vbt_tracker_update_from_detections_seq(trk.handle, db.data_ptr(), ds.data_ptr(), dc.data_ptr(), T, run_, 1, 0.5, stream))
        trk.finish(0.45, stream=stream)
        best, rows_n, nph, ovf, _ = trk.summary(cap=64)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[name] = dict(rows=int(rows_n.sum()), phases=int(nph.sum()), export_id=int(best[0]), overflow=int(ovf.sum()))
        return dt

    for name in trackers:                                            # warm-up: every shape the timed window uses
        run(name)
    times = {k: [] for k in trackers}
    for _ in range(args.reps):
        for name in trackers:
            times[name].append(run(name))
    us = {k: [t / stepped * 1e6 for t in v] for k, v in times.items()}
    out = {"load": f"clip 001 boxes, {T} frames, {stepped} stepped, {float(counts.sum()) / stepped:.2f} detections per stepped frame, "
                   f"{F} frames per launch + clip close, {args.reps} alternating reps after one warm-up each",
           "us_per_stepped_frame": {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in us.items()},
           "sort_over_ocsort": float(np.median(us["sort"]) / np.median(us["ocsort"])),
           "results": res}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
