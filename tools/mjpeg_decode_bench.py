#!/usr/bin/env python3
"""Cost of the MJPEG import (vbt_mjpeg_decode) against the route a caller had before it: decode on the CPU, upload the RGB.

64 frames of 1920x1080 at quality 85 - the synthetic scene of tools/mjpeg_bench.py - as two kinds of file:
  export   as this project's encoder writes them: 4:2:0, one restart interval per MCU row, 68 intervals per frame (4352 per batch);
  pillow   as Pillow writes them by default: 4:2:0, no restart markers, one interval per frame (64 per batch).
Per kind, for each entropy mode asked for (--entropy interval|sync|both; sync once per --subseq size), the modes alternating inside one
process, round by round:
  stages   HIP-event time of each stage of one vbt_mjpeg_decode of the batch (VBT_MJPEG_DECODE_STAMPS=1): H2D copy of the compressed
           bytes, memsets, marker scan, entropy decode, IDCT, upsampling + colour;
  gpu      frames/s from compressed bytes in host memory to RGB24 frames in device memory: Decoder.decode + one synchronisation;
  rounds   vbt_mjpeg_decode_entropy_info: the most rounds any chunk of subsequences took, and the intervals one lane had to finish;
  cpu      the same frames through Pillow (libjpeg-turbo) on --threads CPU threads into pinned memory, then one upload of the RGB:
           frames/s of the decode alone and of decode + upload - in the same process, alternating with `gpu`.
--sweep: the same frames written by Pillow with restart markers every N MCUs / MCU rows (restart_marker_blocks / _rows), from about
1 KB per interval to the whole frame; per spacing the entropy stage of `interval` and of `sync` at every --subseq, alternating.  From
it: the smallest mean interval length at which sync's range lies wholly below interval's, per subsequence size.
Median, minimum and maximum of --reps after --warmup rounds each; every GPU frame is compared with Pillow's.

  python tools/mjpeg_decode_bench.py [--frames 64] [--reps 7] [--warmup 2] [--quality 85] [--threads 16] [--entropy both]
                                     [--subseq 128,256,512,1024] [--sweep] [--out FILE.json]

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
SWEEP = (("blocks", 15), ("blocks", 30), ("blocks", 60), ("rows", 1), ("rows", 2), ("rows", 4), ("rows", 8), ("rows", 17), ("rows", 34), ("none", 0))


def variants(args):
    """[(label, mode, subseq_bytes)]"""
    out = [("interval", "interval", 0)] if args.entropy in ("interval", "both") else []
    if args.entropy in ("sync", "both"):
        out += [(f"sync-{S}", "sync", S) for S in args.subseq]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--entropy", choices=("interval", "sync", "both"), default="both")
    ap.add_argument("--subseq", type=lambda v: [int(x) for x in v.split(",")], default=[128, 256, 512, 1024],
                    help="subsequence sizes of the sync mode, comma-separated; 0 = the library's default")
    ap.add_argument("--sweep", action="store_true", help="also sweep the restart spacing (entropy stage only)")
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

    def pil_bytes(f, **kw):
        b = io.BytesIO()
        Image.fromarray(f).save(b, "JPEG", quality=args.quality, **kw)
        return b.getvalue()
    kinds["pillow"] = [pil_bytes(f) for f in clip]
    res = {"frames": B, "H": H, "W": W, "quality": args.quality, "reps": args.reps, "threads": args.threads, "rgb_bytes": int(clip.nbytes)}
    dec = Decoder(H, W, max_batch=B)
    res["entropy_defaults"] = dict(zip(("mode", "subseq_bytes", "auto_min_interval_bytes"), dec.entropy))
    out = DeviceBuffer(B * H * W * 3)
    host = pinned_empty((B, H, W, 3))
    up = DeviceBuffer(B * H * W * 3)
    pool = ThreadPoolExecutor(args.threads)
    todo = variants(args)

    def cpu_one(k, jpegs):
        host[k] = np.asarray(Image.open(io.BytesIO(jpegs[k])).convert("RGB"))

    def gpu_once(jpegs, mode, S):
        """-> (seconds, status, the six stage times in us, entropy info)"""
        dec.set_entropy(mode, S)
        t0 = time.perf_counter()
        dec.decode(jpegs, out.ptr)
        status = dec.status()
        t = time.perf_counter() - t0
        ms = (ctypes.c_float * 6)()
        _lib.check(L.vbt_mjpeg_decode_stage_ms(dec._h, ms))
        return t, status, [float(v) * 1e3 for v in ms], dec.entropy_info()

    def intervals_of(jpegs):
        return sum(j.count(b"\xff\xd0") + j.count(b"\xff\xd1") + j.count(b"\xff\xd2") + j.count(b"\xff\xd3") + j.count(b"\xff\xd4") +
                   j.count(b"\xff\xd5") + j.count(b"\xff\xd6") + j.count(b"\xff\xd7") + 1 for j in jpegs) / len(jpegs)

    for kind, jpegs in kinds.items():
        t = {"cpu_decode_s": [], "cpu_total_s": []}
        per = {label: {"gpu_s": [], "stages": {k: [] for k in STAGES}, "info": None, "ok": True} for label, _, _ in todo}
        list(pool.map(lambda k: cpu_one(k, jpegs), range(B)))
        want = host.copy()
        for r in range(args.warmup + args.reps):
            for label, mode, S in todo:
                t_gpu, status, us, info = gpu_once(jpegs, mode, S)
                p = per[label]
                p["info"] = info
                p["ok"] = p["ok"] and not status.any()
                if r == 0:
                    p["ok"] = p["ok"] and bool(np.array_equal(out.to_host((B, H, W, 3), np.uint8), want))
                if r >= args.warmup:
                    p["gpu_s"].append(t_gpu)
                    for k, v in zip(STAGES, us):
                        p["stages"][k].append(v)
            t0 = time.perf_counter()
            list(pool.map(lambda k: cpu_one(k, jpegs), range(B)))
            t_dec = time.perf_counter() - t0
            _lib.check(L.vbt_memcpy(up.ptr, host.ctypes.data, host.nbytes, 0))
            _lib.check(L.vbt_device_synchronize(0))
            t_tot = time.perf_counter() - t0
            if r >= args.warmup:
                t["cpu_decode_s"].append(t_dec)
                t["cpu_total_s"].append(t_tot)
        nbytes = sum(len(j) for j in jpegs)
        res[kind] = {"compressed_bytes": nbytes, "ratio": clip.nbytes / nbytes, "intervals_per_frame": intervals_of(jpegs),
                     "cpu_decode_fps": spread([B / v for v in t["cpu_decode_s"]]), "cpu_decode_upload_fps": spread([B / v for v in t["cpu_total_s"]]),
                     "modes": {label: {"status_all_zero_and_equals_pillow": p["ok"], "entropy_info": p["info"],
                                       "stage_us": {k: spread(v) for k, v in p["stages"].items()},
                                       "kernels_us_median": sum(statistics.median(p["stages"][k]) for k in STAGES[2:]),
                                       "gpu_fps": spread([B / v for v in p["gpu_s"]]),
                                       "gpu_over_cpu": spread([c / g for c, g in zip(t["cpu_total_s"], p["gpu_s"])])}      # per round: the two alternate
                               for label, p in per.items()}}
    if args.sweep:
        res["sweep"] = []
        for what, n in SWEEP:
            kw = {"restart_marker_blocks": n} if what == "blocks" else {"restart_marker_rows": n} if what == "rows" else {}
            jpegs = [pil_bytes(f, **kw) for f in clip]
            per = {label: {"us": [], "info": None, "ok": True} for label, _, _ in todo}
            for r in range(args.warmup + args.reps):
                for label, mode, S in todo:
                    _, status, us, info = gpu_once(jpegs, mode, S)
                    per[label]["info"] = info
                    per[label]["ok"] = per[label]["ok"] and not status.any()
                    if r >= args.warmup:
                        per[label]["us"].append(us[3])
            n_int = intervals_of(jpegs)
            res["sweep"].append({"restart": f"{what}-{n}", "intervals_per_frame": n_int, "mean_interval_bytes": sum(len(j) for j in jpegs) / len(jpegs) / n_int,
                                 "entropy_us": {label: dict(spread(p["us"]), rounds=p["info"]["rounds"], single=p["info"]["single"], status_all_zero=p["ok"])
                                                for label, p in per.items()}})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
