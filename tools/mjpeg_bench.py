#!/usr/bin/env python3
"""Cost of the MJPEG export (vbt_mjpeg_encode behind vbt_overlay_draw) against the raw export it stands beside.

64 frames of 1920x1080, RGB24 and NV12, 4 rows per frame, every row with a full 120-point bar path, quality 85.  The frames are a
synthetic scene - smooth gradients, a band-limited texture and a little sensor noise, shifted from frame to frame - because pure noise
is not what a camera delivers and is the one input a JPEG encoder cannot compress.  Per format:
  device   HIP-event time of one draw + encode of the batch on one stream, and of the draw alone;
  read     host-clock time and bytes of Encoder.read() after the device is idle: the offsets, then one copy of the compressed bytes;
  export   frames/s of the whole loop, host array to file: overlay.render(sink=AviWriter) - upload, draw, encode, read, write -
           against overlay.render(out=memmap of a .npy) - upload, draw, raw copy back, write - which is the export as it was before,
           in the same process, alternating; files go to --dir (a temporary directory by default; the page cache takes them).
Median, minimum and maximum of --reps after --warmup rounds each.

  python tools/mjpeg_bench.py [--frames 64] [--reps 7] [--warmup 2] [--quality 85] [--out FILE.json]

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, FPS, TRAIL, IDS = 1080, 1920, 30.0, 120, 4


def make_rows(n_frames):
    """IDS plates on Lissajous paths, one row per plate and frame 1..n_frames (as tools/overlay_bench.py)"""
    import numpy as np
    d = {k: [] for k in ("id", "time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width")}
    f = np.arange(1, n_frames + 1)
    for i in range(IDS):
        d["id"] += [i + 1] * n_frames
        d["time"] += (f / FPS).tolist()
        d["x"] += (0.5 + 0.35 * np.sin(2 * np.pi * f / (293 + 37 * i) + i)).tolist()
        d["y"] += (0.5 + 0.35 * np.sin(2 * np.pi * f / (211 + 23 * i) + 2 * i)).tolist()
        d["dx"] += [0.0] * n_frames
        d["dy"] += [0.0] * n_frames
        d["norm_plate_height"] += [0.25] * n_frames
        d["norm_plate_width"] += [0.14] * n_frames
    return d


def scene(n, fmt):
    """n frames of the synthetic scene in `fmt`: uint8 [n, H, W, 3] or [n, H * 3 // 2, W]"""
    import numpy as np
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    tex = sum(np.sin(x * fx + y * fy + p) for fx, fy, p in ((0.021, 0.013, 0.3), (0.11, -0.07, 1.1), (0.37, 0.29, 2.0), (0.9, 0.6, 0.7)))
    base = np.stack([128 + 70 * np.sin(x / 310 + 0.5) + 14 * tex, 120 + 60 * np.cos(y / 170) + 12 * tex, 110 + 50 * np.sin((x + y) / 400) - 10 * tex], -1)
    out = []
    for t in range(n):
        f = np.roll(base, (3 * t, 5 * t), axis=(0, 1)) + rng.normal(0, 2.0, base.shape).astype(np.float32)
        f = np.clip(f, 0, 255).astype(np.uint8)
        if fmt == "rgb24":
            out.append(f)
        else:
            luma = (16 + f[..., 1].astype(np.int32) * 219 // 255).astype(np.uint8)
            uv = (128 + (f[::2, ::2, [2, 0]].astype(np.int32) - f[::2, ::2, 1:2]) * 112 // 255).clip(16, 240).astype(np.uint8)
            out.append(np.concatenate([luma.reshape(-1), uv.reshape(-1)]).reshape(H * 3 // 2, W))
    return np.stack(out)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from vbt_amd.mjpeg import AviWriter, Encoder, frame_rate
    from vbt_amd.overlay import Overlay, render
    if not torch.cuda.is_available():
        raise SystemExit("mjpeg_bench: no GPU - a timing taken anywhere else says nothing")
    B = args.frames
    rows = make_rows(TRAIL + B)
    stream = torch.cuda.current_stream().cuda_stream
    res = {"frames": B, "H": H, "W": W, "rows_per_frame": IDS, "trail": TRAIL, "quality": args.quality, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}
    tmp = args.dir or tempfile.mkdtemp(prefix="mjpeg_bench_")
    os.makedirs(tmp, exist_ok=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                          # microseconds

    for fmt in ("rgb24", "nv12"):
        clip = scene(B, fmt)
        src = torch.from_numpy(clip).cuda()
        ov = Overlay(H, W, fmt)
        ov.set_rows(rows, FPS, stream)
        enc = Encoder(H, W, fmt, quality=args.quality, max_batch=B)
        t = {"draw_encode_us": [], "draw_us": [], "read_us": []}
        nbytes = 0
        for r in range(args.warmup + args.reps):
            def both():
                ov.draw(src.data_ptr(), B, TRAIL + 1, 1, stream)
                enc.encode(src.data_ptr(), B, stream)
            one = {"draw_encode_us": timed(both)}
            t0 = time.perf_counter()
            jpegs = enc.read()
            one["read_us"] = (time.perf_counter() - t0) * 1e6
            nbytes = enc.last_bytes
            one["draw_us"] = timed(lambda: ov.draw(src.data_ptr(), B, TRAIL + 1, 1, stream))
            if r >= args.warmup:
                for k, v in one.items():
                    t[k].append(v)
        del src
        # the whole export, host array to file: the clip's frames TRAIL + 1 .. are the ones with full paths, so the rows are shifted
        shifted = dict(rows, time=[v - TRAIL / FPS for v in rows["time"]])
        raw_shape = (B,) + clip.shape[1:]
        e = {"mjpeg_s": [], "raw_s": []}
        for r in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            with AviWriter(os.path.join(tmp, f"bench_{fmt}.avi"), W, H, *frame_rate(FPS)) as sink:
                render(clip, shifted, FPS, pix_fmt=fmt, batch=B, sink=sink, quality=args.quality)
            t_mjpeg = time.perf_counter() - t0
            t0 = time.perf_counter()
            out = np.lib.format.open_memmap(os.path.join(tmp, f"bench_{fmt}.npy"), mode="w+", dtype=np.uint8, shape=raw_shape)
            render(clip, shifted, FPS, pix_fmt=fmt, batch=B, out=out)
            out.flush()
            del out
            t_raw = time.perf_counter() - t0
            if r >= args.warmup:
                e["mjpeg_s"].append(t_mjpeg)
                e["raw_s"].append(t_raw)
        avi_bytes = os.path.getsize(os.path.join(tmp, f"bench_{fmt}.avi"))
        res[fmt] = {"batch_bytes": int(clip.nbytes), "compressed_bytes": nbytes, "ratio": clip.nbytes / max(nbytes, 1),
                    "draw_encode_us": spread(t["draw_encode_us"]), "draw_us": spread(t["draw_us"]), "read_us": spread(t["read_us"]),
                    "read_GBps": nbytes / statistics.median(t["read_us"]) / 1e3,
                    "export_mjpeg_fps": spread([B / v for v in e["mjpeg_s"]]), "export_raw_fps": spread([B / v for v in e["raw_s"]]),
                    "export_speedup": statistics.median(e["raw_s"]) / statistics.median(e["mjpeg_s"]),
                    "avi_bytes": avi_bytes, "raw_file_bytes": int(clip.nbytes), "frames_decoded": len(jpegs)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
