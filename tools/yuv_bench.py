"""Host-fed source-resolution frames as packed RGB and as NV12, one process, one GPU.

The shape of bench.py's `configs.n2_1080x1920`: 64 frames of 1920 x 1080 per step from pinned host memory, 24 steps per pass,
uploaded on the copy stream, resized on the device, detect + NMS + track, clip close at the end.  Leg "rgb" is that configuration as
it is (BGR frames, row-pair upload); leg "nv12" feeds NV12 frames of the same size through the same pipeline
(vbt_pipeline_set_pixel_format): luma row pairs + chroma planes up, conversion fused into the resize.  The legs alternate `--reps`
times after one warm-up pass each.  Prints one JSON line: frames/s of each leg (median and every pass) and the bytes uploaded per step.

  python tools/yuv_bench.py [--reps 5] [--steps 24]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=24)
    args = ap.parse_args()
    import torch
    from vbt_amd.track import Pipeline
    nb, T, H, W = 64, args.steps, 1920, 1080
    rng = np.random.default_rng(5)
    src = {"rgb": torch.from_numpy(rng.integers(0, 256, (2, nb, H, W, 3), dtype=np.uint8)).pin_memory(),
           "nv12": torch.from_numpy(rng.integers(0, 256, (2, nb, H * 3 // 2, W), dtype=np.uint8)).pin_memory()}
    pipe = Pipeline(MODEL, nb, max_frames=T + 4, fps=30.0)
    stream = torch.cuda.current_stream().cuda_stream
    h2d = {}

    def leg(name):
        pipe.reset()
        pipe.set_pixel_format("rgb24" if name == "rgb" else name)
        up0 = pipe.info().h2d_bytes
        for t in range(T):
            pipe.step(src[name][t % 2], stream, src_hw=(H, W), swap_rb=name == "rgb")
        pipe.close(cap=64)
        pipe.rows_all()
        total = int(pipe.info().h2d_bytes - up0)
        assert total % T == 0, (name, total)
        h2d[name] = total // T

    def timed(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        leg(name)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for name in src:                                 # first touch of the pinned pages / staging buffers, code objects, clocks
        timed(name)
    times = {name: [] for name in src}
    for _ in range(args.reps):
        for name in src:
            times[name].append(timed(name))
    fps = {name: [nb * T / x for x in v] for name, v in times.items()}
    print(json.dumps({
        "metric": "host_fed_1080x1920_rgb_vs_nv12", "gpu": torch.cuda.get_device_name(0), "batch": nb, "steps": T, "source_hw": [H, W],
        "rgb_frames_per_s": float(np.median(fps["rgb"])), "nv12_frames_per_s": float(np.median(fps["nv12"])),
        "rgb_runs": [round(x, 1) for x in fps["rgb"]], "nv12_runs": [round(x, 1) for x in fps["nv12"]],
        "rgb_h2d_bytes_per_step": h2d["rgb"], "nv12_h2d_bytes_per_step": h2d["nv12"],
        # derived: RGB row pairs 2 h W 3; NV12 luma pairs 0..h-2, then luma row p(h-1) = 1916 to the end of the frame with the chroma plane
        "rgb_h2d_bytes_expected": nb * 2 * 320 * W * 3, "nv12_h2d_bytes_expected": nb * (2 * 319 * W + (H - 1916) * W + H * W // 2),
        "nv12_over_rgb_bytes": h2d["nv12"] / h2d["rgb"], "nv12_over_rgb_frames_per_s": float(np.median(fps["nv12"]) / np.median(fps["rgb"])),
        "rgb_h2d_GBps": h2d["rgb"] * T / float(np.median(times["rgb"])) / 1e9, "nv12_h2d_GBps": h2d["nv12"] * T / float(np.median(times["nv12"])) / 1e9,
    }))


if __name__ == "__main__":
    main()
