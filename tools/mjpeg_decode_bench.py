#!/usr/bin/env python3
"""Cost of the MJPEG import (vbt_mjpeg_decode) against the route a caller had before it: decode on the CPU, upload the RGB.

64 frames of 1920x1080 at quality 85 - the synthetic scene of tools/mjpeg_bench.py - as two kinds of file:
  export   as this project's encoder writes them: 4:2:0, one restart interval per MCU row, 68 intervals per frame (4352 per batch);
  pillow   as Pillow writes them by default: 4:2:0, no restart markers, one interval per frame (64 per batch).
Per kind:
  stages   HIP-event time of each stage of one vbt_mjpeg_decode of the batch (VBT_MJPEG_DECODE_STAMPS=1): H2D copy of the compressed
           bytes, memsets, marker scan, entropy decode, IDCT, upsampling + colour;
  gpu      frames/s from compressed bytes in host memory to RGB24 frames in device memory: Decoder.decode + one synchronisation;
  cpu      the same frames through Pillow (libjpeg-turbo) on --threads CPU threads into pinned memory, then one upload of the RGB:
           frames/s of the decode alone and of decode + upload - in the same process, alternating with `gpu`.
Median, minimum and maximum of --reps after --warmup rounds each; every GPU frame is compared with Pillow's.

  python tools/mjpeg_decode_bench.py [--frames 64] [--reps 7] [--warmup 2] [--quality 85] [--threads 16] [--out FILE.json]

Prints one JSON line."""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["VBT_MJPEG_DECODE_STAMPS"] = "1"

from mjpeg_bench import H, W, scene, spread  # noqa: E402

STAGES = ("h2d_copy", "memsets", "marker_scan", "entropy_decode", "idct", "upsample_colour")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ctypes
    import numpy as np
    from PIL import Image
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer, pinned_empty
    from vbt_amd.mjpeg import Decoder, Encoder
    L = _lib.lib()
    if L.vbt_device_count() < 1:
        raise SystemExit("mjpeg_decode_bench: no GPU - a timing taken anywhere else says nothing")
    B = args.frames
    clip = scene(B, "rgb24")
    enc = Encoder(H, W, "rgb24", quality=args.quality, max_batch=B)
    src = DeviceBuffer.from_host(clip)
    enc.encode(src.ptr, B)
    kinds = {"export": enc.read()}
    del src, enc

    def pil_bytes(f):
        b = io.BytesIO()
        Image.fromarray(f).save(b, "JPEG", quality=args.quality)
        return b.getvalue()
    kinds["pillow"] = [pil_bytes(f) for f in clip]
    res = {"frames": B, "H": H, "W": W, "quality": args.quality, "reps": args.reps, "threads": args.threads, "rgb_bytes": int(clip.nbytes)}
    dec = Decoder(H, W, max_batch=B)
    out = DeviceBuffer(B * H * W * 3)
    host = pinned_empty((B, H, W, 3))
    up = DeviceBuffer(B * H * W * 3)
    pool = ThreadPoolExecutor(args.threads)

    def cpu_one(k, jpegs):
        host[k] = np.asarray(Image.open(io.BytesIO(jpegs[k])).convert("RGB"))

    for kind, jpegs in kinds.items():
        t = {"gpu_s": [], "cpu_decode_s": [], "cpu_total_s": []}
        stages = {k: [] for k in STAGES}
        for r in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            dec.decode(jpegs, out.ptr)
            status = dec.status()
            t_gpu = time.perf_counter() - t0
            ms = (ctypes.c_float * 6)()
            _lib.check(L.vbt_mjpeg_decode_stage_ms(dec._h, ms))
            t0 = time.perf_counter()
            list(pool.map(lambda k: cpu_one(k, jpegs), range(B)))
            t_dec = time.perf_counter() - t0
            _lib.check(L.vbt_memcpy(up.ptr, host.ctypes.data, host.nbytes, 0))
            _lib.check(L.vbt_device_synchronize(0))
            t_tot = time.perf_counter() - t0
            if r >= args.warmup:
                t["gpu_s"].append(t_gpu)
                t["cpu_decode_s"].append(t_dec)
                t["cpu_total_s"].append(t_tot)
                for k, v in zip(STAGES, ms):
                    stages[k].append(float(v) * 1e3)
        got = out.to_host((B, H, W, 3), np.uint8)
        nbytes = sum(len(j) for j in jpegs)
        res[kind] = {"compressed_bytes": nbytes, "ratio": clip.nbytes / nbytes, "intervals_per_frame": 68 if kind == "export" else 1,
                     "status_all_zero": bool(not status.any()), "equals_pillow": bool(np.array_equal(got, host)),
                     "stage_us": {k: spread(v) for k, v in stages.items()},
                     "kernels_us_median": sum(statistics.median(stages[k]) for k in STAGES[2:]),
                     "gpu_fps": spread([B / v for v in t["gpu_s"]]), "cpu_decode_fps": spread([B / v for v in t["cpu_decode_s"]]),
                     "cpu_decode_upload_fps": spread([B / v for v in t["cpu_total_s"]]),
                     "gpu_over_cpu": statistics.median(t["cpu_total_s"]) / statistics.median(t["gpu_s"])}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
