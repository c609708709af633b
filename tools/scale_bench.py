#!/usr/bin/env python3
"""Cost of the scaled export (include/vbt_hip.h, "Scaled export") against the full-size encode it stands beside.

64 frames of 1920x1080 -> 1280x720, RGB24 and NV12, quality 85, the synthetic scene of tools/mjpeg_bench.py.  Per format three routes,
each one HIP-event time of the enqueued work of one batch on one stream (the read-back is outside the window):
  a  full      vbt_mjpeg_encode of the batch at 1920x1080 - the export as it is without --display_image_height;
  b  two_step  vbt_scaler_run into a second buffer, then vbt_mjpeg_encode of that at 1280x720;
  c  fused     vbt_mjpeg_encode of a vbt_mjpeg_create_scaled handle: resized in the encoder's colour stage;
and vbt_scaler_run alone.  The routes alternate inside every round, in one process; median, minimum and maximum of --reps rounds after
--warmup.  Routes b and c must give the same bytes: checked once, before the timing.

  python tools/scale_bench.py [--frames 64] [--reps 20] [--warmup 3] [--quality 85] [--out FILE.json]

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W, DISPLAY_HEIGHT = 1080, 1920, 720


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from mjpeg_bench import scene
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.mjpeg import Encoder
    from vbt_amd.scale import Scaler, display_size
    if not torch.cuda.is_available():
        raise SystemExit("scale_bench: no GPU - a timing taken anywhere else says nothing")
    B = args.frames
    stream = torch.cuda.current_stream().cuda_stream
    res = {"frames": B, "H": H, "W": W, "quality": args.quality, "reps": args.reps, "device": torch.cuda.get_device_name(0)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                          # microseconds

    for fmt in ("rgb24", "nv12"):
        h, w = display_size(H, W, fmt, DISPLAY_HEIGHT)
        clip = scene(B, fmt)
        src = torch.from_numpy(clip).cuda()
        small_bytes = h * w * 3 if fmt == "rgb24" else h * w * 3 // 2
        small = DeviceBuffer(B * small_bytes)
        scaler = Scaler(H, W, h, w, fmt)
        full = Encoder(H, W, fmt, quality=args.quality, max_batch=B)
        plain = Encoder(h, w, fmt, quality=args.quality, max_batch=B)
        fused = Encoder(H, W, fmt, quality=args.quality, max_batch=B, out_hw=(h, w))

        def route_a():
            full.encode(src.data_ptr(), B, stream)

        def route_b():
            scaler.run(src.data_ptr(), small.ptr, B, stream)
            plain.encode(small.ptr, B, stream)

        def route_c():
            fused.encode(src.data_ptr(), B, stream)

        route_b()
        route_c()
        two, one = plain.read(), fused.read()
        if two != one:
            raise SystemExit(f"scale_bench: {fmt}: the fused encoder's bytes differ from scale + encode")
        t = {"full_us": [], "two_step_us": [], "fused_us": [], "scale_us": []}
        nbytes = {}
        for r in range(args.warmup + args.reps):
            one_round = {}
            for name, fn, enc in (("full_us", route_a, full), ("two_step_us", route_b, plain), ("fused_us", route_c, fused)):
                one_round[name] = timed(fn)
                enc.read()
                nbytes[name] = enc.last_bytes
            one_round["scale_us"] = timed(lambda: scaler.run(src.data_ptr(), small.ptr, B, stream))
            if r >= args.warmup:
                for k, v in one_round.items():
                    t[k].append(v)
        res[fmt] = {"h": h, "w": w, "batch_bytes": int(clip.nbytes), "scaled_batch_bytes": B * small_bytes,
                    "compressed_bytes_full": nbytes["full_us"], "compressed_bytes_scaled": nbytes["fused_us"],
                    **{k: spread(v) for k, v in t.items()}}
        del src, small, scaler, full, plain, fused
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
