#!/usr/bin/env python3
"""Cost of the live rep analysis at the headline configuration (bench.py's workload, bench.py itself untouched).

Two pipelines on the same resident frames as bench.py's contract run (Lite0 320x320, --clips synthetic clips, default depth): one
with live analysis off, one with it on and polled (Pipeline.live()) every --poll steps.  Each repetition runs W warm-up steps, then
K steps + clip close between two fences; the pipelines alternate, --reps times each, and the medians are compared:

  python tools/live_bench.py [--steps 256] [--warmup 16] [--reps 5] [--poll 16] [--out FILE.json]

Prints one JSON line (frames/s off and on, the relative cost against the 2 % budget).  The per-launch time of live_analyze_kernel
comes from a separate run under `rocprofv3 --kernel-trace --stats` (profiles/r06_live.md).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (sets the queue count and the pinned kernel plan before HIP starts)

os.environ.setdefault("VBT_STRICT_PLACEMENT", "0")   # two pipelines in one process; a profiler serialises the queues


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--poll", type=int, default=16, help="steps between two Pipeline.live() polls")
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--unique-steps", type=int, default=64)
    ap.add_argument("--live-only", action="store_true", help="only the live pipeline, once (for a profiler run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from vbt_amd.container import Container
    from vbt_amd.track import Pipeline
    n, K, W = args.clips, args.steps, args.warmup
    U = max(1, min(args.unique_steps, K + W))
    size = int(Container(bench.MODEL).header["image_size"])
    frames = torch.from_numpy(bench.make_frames(list(range(n)), 0, U, size)).to("cuda:0")
    fbytes = frames[0].numel()
    stream = torch.cuda.current_stream().cuda_stream
    PH = 128

    def make(live):
        p = Pipeline(bench.MODEL, n, max_frames=(K + W) + 8, fps=60.0, detection_treshold=0.5, rows_per_frame=8)
        if live:
            p.enable_live()
        return p

    def run(pipe, live):
        pipe.reset()
        for i in range(W):
            pipe.step(frames.data_ptr() + (i % U) * fbytes, stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        polls = 0
        for i in range(K):
            pipe.step(frames.data_ptr() + ((W + i) % U) * fbytes, stream)
            if live and (i + 1) % args.poll == 0:
                pipe.live()
                polls += 1
        res = bench.close_clips(pipe, PH)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, res, polls

    if args.live_only:
        pipe = make(True)
        dt, _, polls = run(pipe, True)
        print(json.dumps({"live_only": True, "frames_per_s": K * n / dt, "steps": K, "polls": polls}))
        return
    pipes = {"off": make(False), "on": make(True)}
    times = {"off": [], "on": []}
    results = {}
    for _ in range(args.reps):
        for key in ("off", "on"):
            dt, res, polls = run(pipes[key], key == "on")
            times[key].append(dt)
            results[key] = res
    same = all(np.array_equal(a, b) for a, b in zip(results["off"], results["on"]))
    med = {k: float(np.median(v)) for k, v in times.items()}
    fps = {k: K * n / med[k] for k in med}
    cost = 1.0 - fps["on"] / fps["off"]
    live = pipes["on"].live()
    out = {"config": f"Lite0 {size}x{size}, {n} clips, depth {pipes['on'].depth}, {K} steps + close, warm-up {W}, {args.reps} reps (median)",
           "frames_per_s_off": fps["off"], "frames_per_s_on": fps["on"], "ms_per_step_off": med["off"] / K * 1e3,
           "ms_per_step_on": med["on"] / K * 1e3, "poll_every_steps": args.poll, "cost_frac": cost, "budget_frac": 0.02,
           "within_budget": cost <= 0.02, "close_outputs_identical": bool(same),
           "times_s": times, "live_overflow_clips": int(sum(1 for r in live if r.overflow)),
           "placement_ok": [bool(p.info().placement_ok) for p in pipes.values()]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
