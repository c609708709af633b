#!/usr/bin/env python3
"""Cost of the rep figure (vbt_figure: include/vbt_hip.h, "Rep figure") against a copy of the frames it writes.

The reference's corpus size: 34 figures of 1280 x 800, each of 2000 rows and 24 phases, seeded and generated here.  In one process,
alternating, HIP-event times in microseconds, median with min and max of --reps after --warmup rounds:
  set     vbt_figure_set: host validation, ONE upload, the prepare launch (a workgroup per figure) and the synchronisation that ends it;
  render  vbt_figure_render of the 34 figures (one launch), and of 10 back to back divided by 10;
  encode  vbt_mjpeg_encode of the 34 rendered frames at quality 90 (enqueue to the end of its last kernel; the read-back is not in it);
  copy    a device-to-device hipMemcpyAsync of the same 34 frames - the yardstick the overlay benchmarks use.  The render writes each
          byte once and reads none: half the copy's traffic.
Also which path the render's tiles take (points and records in LDS, or global memory).

  python tools/figure_bench.py [--figures 34] [--rows 2000] [--phases 24] [--size 1280x800] [--scale 2] [--reps 20] [--warmup 5] [--out FILE.json]

Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_figure(seed, T, P):
    """a set of P / 2 reps: the bar goes down and up once per rep, 30 rows a second, with detector noise"""
    import numpy as np
    rng = np.random.default_rng(seed)
    t = (1 + np.arange(T)) / 30.0
    period = t[-1] / (P / 2.0)
    y = 0.5 + 0.25 * np.sin(2 * np.pi * t / period) + rng.normal(0, 0.003, T)
    x = 0.5 + 0.02 * np.sin(2 * np.pi * t / (3.1 * period)) + rng.normal(0, 0.003, T)
    rows = np.stack([t, x, y, np.gradient(x, t), np.gradient(y, t), np.full(T, 0.2), np.full(T, 0.2)], axis=1)
    ph = [(t[0] + i * period / 2, t[0] + (i + 1) * period / 2, 0.3, 0.7, 0.4 + 0.01 * (i % 7), i % 2) for i in range(P)]
    return rows, np.array(ph, np.float64).reshape(-1, 6)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--figures", type=int, default=34)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--phases", type=int, default=24)
    ap.add_argument("--size", default="1280x800")
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.lower().split("x"))
    import numpy as np
    import torch
    from vbt_amd.figure import Figure
    from vbt_amd.mjpeg import Encoder
    if not torch.cuda.is_available():
        raise SystemExit("figure_bench: no GPU - a timing taken anywhere else says nothing")
    so = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = ctypes.CDLL(so if os.path.exists(so) else "libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    N = args.figures
    figs = [make_figure(100 + i, args.rows, args.phases) for i in range(N)]
    stream = torch.cuda.current_stream().cuda_stream
    fig = Figure(width=W, height=H, scale=args.scale, max_figures=N, max_rows=args.rows, max_phases=max(args.phases, 1))
    enc = Encoder(H, W, "rgb24", 90, N)
    frames = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(frames)
    nbytes = frames.numel()
    res = {"figures": N, "W": W, "H": H, "scale": args.scale, "rows": args.rows, "phases": args.phases, "reps": args.reps,
           "frame_bytes": nbytes, "device": torch.cuda.get_device_name(0)}

    def timed(fn, k=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k                      # microseconds

    def fset():
        fig.set(figs, stream)

    def render():
        fig.render(frames.data_ptr(), 0, N, stream)

    def encode():
        enc.encode(frames.data_ptr(), N, stream)

    def copy():
        rc = hip.hipMemcpyAsync(dst.data_ptr(), frames.data_ptr(), nbytes, 3, stream)      # hipMemcpyDeviceToDevice
        assert rc == 0, rc
    t = {"set": [], "render": [], "render10": [], "encode": [], "copy": []}
    jpeg_bytes = 0
    for r in range(args.warmup + args.reps):
        one = {"set": timed(fset), "render": timed(render), "copy": timed(copy), "render10": timed(render, 10), "encode": timed(encode)}
        jpeg_bytes = sum(len(j) for j in enc.read())              # releases the encoder for the next round
        if r >= args.warmup:
            for k, v in one.items():
                t[k].append(v)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import figure_ref as FR
    _, pts, recs = fig.table(0)
    staged = FR.staged(pts.astype(np.int64), recs.astype(np.int64), width=W, height=H, scale=args.scale, thickness=fig.params["thickness"])
    med = {k: statistics.median(v) for k, v in t.items()}
    res.update({k + "_us": spread(v) for k, v in t.items()})
    res.update({"render_over_copy": med["render"] / med["copy"], "render_back_to_back_over_copy": med["render10"] / med["copy"],
                "copy_GBps": 2 * nbytes / med["copy"] / 1e3, "render_write_GBps": nbytes / med["render"] / 1e3, "jpeg_bytes": jpeg_bytes,
                "figure0_points_in_lds": bool(staged[0]), "figure0_records_in_lds": bool(staged[1])})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
