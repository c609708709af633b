#!/usr/bin/env python3
"""Cost of the validation figure (vbt_validation: include/vbt_hip.h, "Validation figure") on the 37 golden pairs (32 Kinovea, 5
Qualisys: tests/golden/validation.npz, dfs_ocsort_main.npz) at the default size, and the wall time of the batched numbers against the
loop over validate.validate_pair that gave them before - in one process, alternating rounds, after --warmup rounds, median with min
and max of --reps.

HIP-event times in microseconds (all 37 pairs go in ONE set: the kind is per pair):
  set     vbt_validation_set: host validation, ONE upload, the prepare launch (a workgroup per pair) and the synchronisation;
  render  vbt_validation_render of the 37 frames (one launch), and of 10 back to back divided by 10;
  encode  vbt_mjpeg_encode of the rendered frames at quality 90 (the read-back is not in it);
  copy    a device-to-device hipMemcpyAsync of the same frames: the per-byte yardstick of the render.
Wall times in milliseconds (time.perf_counter around the whole call, synchronised):
  batched   Validation.set + Validation.stats on an existing handle: the numbers of all 37 pairs;
  loop      validate.validate_pair per pair: one vbt_window_means round trip each, the rest in numpy.
Also the merged points per pair and which path the render's tiles take.

  python tools/validation_bench.py [--reps 20] [--warmup 5] [--out FILE.json]

Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden_pairs():
    """[(ref, rows, source)] of the 37 pairs"""
    import numpy as np
    gold = np.load(os.path.join(GOLDEN, "validation.npz"))
    main = np.load(os.path.join(GOLDEN, "dfs_ocsort_main.npz"))
    out = []
    for k in sorted(k[:-6] for k in gold.files if k.endswith("_stats")):
        if k.startswith("q_"):
            out.append((gold[k + "_ref"], gold[k + "_rows"], "qualisys"))
        else:
            c = "c" + k[1:]
            out.append((gold[k + "_ref"], np.stack([main[f"{c}_{n}"] for n in ("time", "x", "y", "norm_plate_height", "norm_plate_width")], axis=1), "kinovea"))
    return out


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from vbt_amd import validate as V
    from vbt_amd.mjpeg import Encoder
    if not torch.cuda.is_available():
        raise SystemExit("validation_bench: no GPU - a timing taken anywhere else says nothing")
    so = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = ctypes.CDLL(so if os.path.exists(so) else "libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    stream = torch.cuda.current_stream().cuda_stream
    items = golden_pairs()
    n = len(items)
    pairs, kinds = [(f, r) for f, r, _ in items], [s for _, _, s in items]
    v = V.Validation(max_pairs=n, max_rows=max(len(r) for _, r in pairs), max_ref_rows=max(len(f) for f, _ in pairs),
                     max_grid=max(V.grid_size(f, r) for f, r in pairs))
    W, H = v.W, v.H
    frames = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(frames)
    enc = Encoder(H, W, "rgb24", 90, n)
    res = {"pairs": n, "W": W, "H": H, "scale": v.params["scale"], "reps": args.reps, "frame_bytes": frames.numel(),
           "rows": [len(r) for _, r in pairs], "ref_rows": [len(f) for f, _ in pairs], "grid": [V.grid_size(f, r) for f, r in pairs],
           "device": torch.cuda.get_device_name(0)}

    def timed(fn, k=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k                      # microseconds

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out              # milliseconds

    def fset():
        v.set(pairs, kinds, 0.45, 30.0, stream)

    def render():
        v.render(frames.data_ptr(), 0, n, stream)

    def encode():
        enc.encode(frames.data_ptr(), n, stream)

    def copy():
        rc = hip.hipMemcpyAsync(dst.data_ptr(), frames.data_ptr(), frames.numel(), 3, stream)      # hipMemcpyDeviceToDevice
        assert rc == 0, rc

    def batched():
        v.set(pairs, kinds, 0.45, 30.0, stream)
        return v.stats()

    def loop():
        return [V.validate_pair(f, r, 0.45, s) for f, r, s in items]
    t = {"set": [], "render": [], "render10": [], "encode": [], "copy": [], "batched_ms": [], "loop_ms": []}
    jpeg_bytes, stats, ref = 0, None, None
    for r in range(args.warmup + args.reps):
        one = {"set": timed(fset), "render": timed(render), "copy": timed(copy), "render10": timed(render, 10), "encode": timed(encode)}
        jpeg_bytes = sum(len(j) for j in enc.read())                # releases the encoder for the next round
        order = (batched, loop) if r % 2 == 0 else (loop, batched)  # alternating which goes first
        for fn in order:
            ms, out = wall(fn)
            one[fn.__name__ + "_ms"] = ms
            if fn is batched:
                stats = out
            else:
                ref = out
        if r >= args.warmup:
            for k, val in one.items():
                t[k].append(val)
    want = np.array([[q["mse_x"], q["mse_y"], q["r_x"], q["r_y"]] for q in ref])
    res["max_rel_diff_to_loop"] = float(np.max(np.abs(stats[:, :4] - want) / np.abs(want)))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import validation_ref as VR
    merged, paths = [], []
    for i in range(n):
        _, _, _, counts, pts, recs = v.table(i)
        merged.append(int(counts.sum()))
        st = VR.staged(counts.astype(np.int64), pts.astype(np.int64), recs.astype(np.int64), width=W, height=H, scale=v.params["scale"],
                       thickness=v.params["thickness"])
        paths.append("lds" if all(st) else "global")
    med = {k: statistics.median(val) for k, val in t.items()}
    nbytes = frames.numel()
    res.update({(k if k.endswith("_ms") else k + "_us"): spread(val) for k, val in t.items()})
    res.update({"render_over_copy": med["render"] / med["copy"], "copy_GBps": 2 * nbytes / med["copy"] / 1e3,
                "render_write_GBps": nbytes / med["render"] / 1e3, "render_ns_per_pixel": med["render"] * 1e3 / (nbytes // 3),
                "loop_over_batched": med["loop_ms"] / med["batched_ms"], "jpeg_bytes": jpeg_bytes, "merged_points_per_pair": merged, "pair_paths": paths})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
