#!/usr/bin/env python3
"""Cost of the curve figure (vbt_curve_figure: include/vbt_hip.h, "Curve figure") against a copy of the frames it writes and against
the rep figure's render in the same process.

The workload of one `cli eval --fig_dir` run with six models and score thresholds: 12 figures at the default size - 2 combined ones of
six series (precision-recall and ROC, 1120 x 640) and 10 per-model ones (5 PR, 5 ROC, 1120 x 480, two annotations each) - through two
handles, as evaluate.plot_precision_recall / plot_roc use them.  The curves are computed here from seeded scores and labels, --points
detections per model: the precision-recall sawtooth (points + 1 points) and the ROC staircase.  In one process, alternating, HIP-event
times in microseconds, median with min and max of --reps after --warmup rounds, each the sum over both handles:
  set     vbt_curve_figure_set: host validation, ONE upload, the prepare launch (a workgroup per figure) and the synchronisation;
  render  vbt_curve_figure_render (one launch per handle), and of 10 back to back divided by 10;
  encode  vbt_mjpeg_encode of the rendered frames at quality 90 (the read-back is not in it);
  copy    a device-to-device hipMemcpyAsync of the same frames.
  rep_render  vbt_figure_render of tools/figure_bench.py's workload (34 x 1280 x 800, 2000 rows, 24 phases): the per-pixel yardstick.
Also the merged points per figure and which path the render's tiles take.

  python tools/curve_figure_bench.py [--points 100] [--size 1120x640] [--scale 2] [--reps 20] [--warmup 5] [--out FILE.json]

Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def make_curves(seed, n):
    """(recall, precision, pr thresholds), (fpr, tpr, roc thresholds) of n seeded detections, in scikit-learn's orders"""
    import numpy as np
    rng = np.random.default_rng(seed)
    score = np.sort(rng.random(n))[::-1]
    label = rng.random(n) < 0.15 + 0.8 * score ** (0.5 + 0.1 * (seed % 5))
    label[0], label[-1] = True, False
    tp, fp = np.cumsum(label), np.cumsum(~label)
    precision, recall = tp / (tp + fp), tp / tp[-1]
    pr = (np.r_[recall[::-1], 0.0], np.r_[precision[::-1], 1.0], np.r_[score[::-1], score[0]])
    roc = (np.r_[0.0, fp / fp[-1]], np.r_[0.0, tp / tp[-1]], np.r_[np.inf, score])
    return pr, roc


def make_figures(points):
    """([combined PR, combined ROC], [10 per-model figures])"""
    import numpy as np
    from vbt_amd import curve_figure as CF
    from vbt_amd.evaluate import closest_point
    curves = [make_curves(7 + k, points) for k in range(6)]
    combined, singles = [], []
    for kind in (0, 1):
        titles = dict(x_title="FP Rate", y_title="TP Rate") if kind else dict(x_title="Recall", y_title="Precision")
        series = [(np.stack(c[kind][:2], axis=1), f"efficientdet_lite{k // 2}{'_whole' if k % 2 else ''}, A{'UC' if kind else 'P50'}=0.{9000 - 311 * k}", k)
                  for k, c in enumerate(curves)]
        combined.append(CF.figure(series, corner=kind, minor_x=100 if kind else 0, minor_y=100, **titles))
        for k in range(5):
            thr = curves[k][kind][2]
            marks = [(0, closest_point(thr, v), f"{thr[closest_point(thr, v)]:.4f}") for v in ((0.2, 0.5) if kind else (0.5, 0.2))]
            singles.append(CF.figure([series[k]], marks, corner=kind, minor_x=50, minor_y=50, **titles))
    return combined, singles


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--size", default="1120x640")
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.lower().split("x"))
    import numpy as np
    import torch
    from figure_bench import make_figure
    from vbt_amd.curve_figure import CurveFigure
    from vbt_amd.figure import Figure
    from vbt_amd.mjpeg import Encoder
    if not torch.cuda.is_available():
        raise SystemExit("curve_figure_bench: no GPU - a timing taken anywhere else says nothing")
    so = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = ctypes.CDLL(so if os.path.exists(so) else "libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    stream = torch.cuda.current_stream().cuda_stream
    groups = []                                                   # (handle, figures, encoder, frames, copy target)
    for figs, h in zip(make_figures(args.points), (H, 3 * H // 4)):
        pts = max(sum(len(xy) for xy, _, _ in f["series"]) for f in figs)
        fig = CurveFigure(width=W, height=h, scale=args.scale, max_figures=len(figs), max_series=6, max_points=pts, max_marks=2)
        frames = torch.empty((len(figs), h, W, 3), dtype=torch.uint8, device="cuda")
        groups.append((fig, figs, Encoder(h, W, "rgb24", 90, len(figs)), frames, torch.empty_like(frames)))
    nbytes = sum(g[3].numel() for g in groups)
    rep_n, rep_w, rep_h = 34, 1280, 800
    rep = Figure(width=rep_w, height=rep_h, scale=2, max_figures=rep_n, max_rows=2000, max_phases=24)
    rep.set([make_figure(100 + i, 2000, 24) for i in range(rep_n)], stream)
    rep_frames = torch.empty((rep_n, rep_h, rep_w, 3), dtype=torch.uint8, device="cuda")
    res = {"figures": sum(len(g[1]) for g in groups), "W": W, "H": H, "scale": args.scale, "points": args.points, "reps": args.reps,
           "frame_bytes": nbytes, "pixels": nbytes // 3, "device": torch.cuda.get_device_name(0)}

    def timed(fn, k=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k                      # microseconds

    def fset():
        for fig, figs, _, _, _ in groups:
            fig.set(figs, stream)

    def render():
        for fig, figs, _, frames, _ in groups:
            fig.render(frames.data_ptr(), 0, len(figs), stream)

    def encode():
        for _, figs, enc, frames, _ in groups:
            enc.encode(frames.data_ptr(), len(figs), stream)

    def copy():
        for _, _, _, frames, dst in groups:
            rc = hip.hipMemcpyAsync(dst.data_ptr(), frames.data_ptr(), frames.numel(), 3, stream)      # hipMemcpyDeviceToDevice
            assert rc == 0, rc

    def rep_render():
        rep.render(rep_frames.data_ptr(), 0, rep_n, stream)
    t = {"set": [], "render": [], "render10": [], "encode": [], "copy": [], "rep_render": []}
    jpeg_bytes = 0
    for r in range(args.warmup + args.reps):
        one = {"set": timed(fset), "render": timed(render), "copy": timed(copy), "render10": timed(render, 10), "encode": timed(encode),
               "rep_render": timed(rep_render)}
        jpeg_bytes = sum(len(j) for g in groups for j in g[2].read())      # releases the encoders for the next round
        if r >= args.warmup:
            for k, v in one.items():
                t[k].append(v)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import curve_figure_ref as CR
    merged, paths = [], []
    for fig, figs, _, _, _ in groups:
        for i in range(len(figs)):
            counts, pts, recs = fig.table(i)
            merged.append(int(counts.sum()))
            st = CR.staged(counts.astype(np.int64), pts.astype(np.int64), recs.astype(np.int64), width=W, height=fig.H, scale=args.scale,
                           thickness=fig.params["thickness"])
            paths.append("lds" if all(st) else "global")
    med = {k: statistics.median(v) for k, v in t.items()}
    rep_pixels = rep_n * rep_w * rep_h
    res.update({k + "_us": spread(v) for k, v in t.items()})
    res.update({"render_over_copy": med["render"] / med["copy"], "copy_GBps": 2 * nbytes / med["copy"] / 1e3,
                "render_write_GBps": nbytes / med["render"] / 1e3, "render_ns_per_pixel": med["render"] * 1e3 / (nbytes // 3),
                "rep_render_ns_per_pixel": med["rep_render"] * 1e3 / rep_pixels, "jpeg_bytes": jpeg_bytes,
                "input_points_per_figure": [sum(len(xy) for xy, _, _ in f["series"]) for g in groups for f in g[1]],
                "merged_points_per_figure": merged, "figure_paths": paths})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
