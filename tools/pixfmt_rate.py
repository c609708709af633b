"""Host-fed 1920 x 1080 frames in every source format, one process, one GPU: frames/s and bytes uploaded per frame.

The shape of tools/yuv_bench.py: 64 frames per step from pinned host memory, 24 steps per pass, uploaded on the copy stream (only the
rows the resize reads: the compact layouts of include/vbt_hip.h, vbt_pipeline_set_pixel_format), converted and resized on the device,
detect + NMS + track, clip close at the end.  One leg per format - nv12 (the path that existed before the other formats), yuyv422,
uyvy422, p010le, rgb24 - alternating `--rounds` times after one warm-up pass each.  The path is bound by the upload, so the expectation
the table is read against is: rates in the inverse ratio of the uploaded bytes.  Prints one JSON line and, with --md, the table.

  python tools/pixfmt_rate.py [--rounds 4] [--steps 24] [--md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODEL = os.path.join(ROOT, "models", "efficientdet_lite0_synth.vbtm")
LEGS = ("nv12", "yuyv422", "uyvy422", "p010le", "rgb24")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--md", action="store_true", help="also print the table as markdown")
    args = ap.parse_args()
    import torch
    from vbt_amd.rawvideo import frame_dtype, frame_shape
    from vbt_amd.track import Pipeline
    nb, T, H, W = 64, args.steps, 1080, 1920
    rng = np.random.default_rng(5)
    src = {}
    for name in LEGS:
        dt = frame_dtype(name)
        a = rng.integers(0, 1 << (8 * dt.itemsize), (2, nb) + frame_shape(name, H, W), dtype=dt)
        src[name] = torch.from_numpy(a.view(np.int16) if dt.itemsize == 2 else a).pin_memory()
    pipe = Pipeline(MODEL, nb, max_frames=T + 4, fps=30.0)
    stream = torch.cuda.current_stream().cuda_stream
    h2d = {}

    def leg(name):
        pipe.reset()
        pipe.set_pixel_format(name)
        up0 = pipe.info().h2d_bytes
        for t in range(T):
            pipe.step(src[name][t % 2], stream, src_hw=(H, W))
        pipe.close(cap=64)
        pipe.rows_all()
        total = int(pipe.info().h2d_bytes - up0)
        assert total % (T * nb) == 0, (name, total)
        h2d[name] = total // (T * nb)

    def timed(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        leg(name)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for name in LEGS:                                # first touch of the pinned pages / staging buffers, code objects, clocks
        timed(name)
    times = {name: [] for name in LEGS}
    for _ in range(args.rounds):
        for name in LEGS:
            times[name].append(timed(name))
    fps = {name: [nb * T / x for x in v] for name, v in times.items()}
    med = {name: float(np.median(v)) for name, v in fps.items()}
    out = {"metric": "host_fed_1080p_by_pixel_format", "gpu": torch.cuda.get_device_name(0), "batch": nb, "steps": T, "source_hw": [H, W],
           "rounds": args.rounds}
    for name in LEGS:
        out[name] = {"frames_per_s": med[name], "runs": [round(x, 1) for x in fps[name]], "h2d_bytes_per_frame": h2d[name],
                     "frame_bytes": int(src[name][0, 0].numel() * src[name].element_size()),
                     "h2d_GBps": h2d[name] * med[name] / 1e9,
                     "bytes_over_nv12": h2d[name] / h2d["nv12"], "rate_over_nv12": med[name] / med["nv12"],
                     "rate_expected_from_bytes": h2d["nv12"] / h2d[name]}
    print(json.dumps(out))
    if args.md:
        print("| format | uploaded bytes / frame | bytes / nv12 | frames/s (median) | min .. max | rate / nv12 | expected from bytes | upload GB/s |")
        print("|---|---|---|---|---|---|---|---|")
        for name in LEGS:
            o = out[name]
            print(f"| {name} | {o['h2d_bytes_per_frame']} | {o['bytes_over_nv12']:.3f} | {o['frames_per_s']:.0f} | "
                  f"{min(o['runs']):.0f} .. {max(o['runs']):.0f} | {o['rate_over_nv12']:.3f} | {o['rate_expected_from_bytes']:.3f} | {o['h2d_GBps']:.2f} |")


if __name__ == "__main__":
    main()
