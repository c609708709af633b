#!/usr/bin/env python3
"""Cost of the tracking overlay (vbt_overlay_draw) against the least any copy-then-draw or whole-frame design would pay.

64 frames of 1920x1080 on the device, RGB24 and NV12, 4 rows per frame, every row with a full 120-point bar path.  Per format:
  draw   HIP-event time of one vbt_overlay_draw of the batch (one launch), and of 10 back to back divided by 10;
  copy   HIP-event time of a device-to-device hipMemcpyAsync of the same 64 frames, in the same process, alternating with the draws;
  median of --reps after --warmup rounds each.  The draw writes well under 1 % of the bytes the copy moves.
set_rows is timed on the host clock (it synchronises): validation, index, upload and the prepare kernel, for the benchmark's rows and
for a 10-minute clip's worth (4 ids x 18000 frames).

--hud: a second handle with the same rows and a rep panel (vbt_overlay_set_hud: default 156 x 150 panel, 24 phases) is timed in the same
rounds, alternating with the first: per format "hud" = its draw time and the increment over the panel-off draw, next to the copy of
the batch.  --size WxH (default 1920x1080): the same at another frame size - the increment must not grow with H * W.

--hud_follow: the rep panel that follows the live analysis (vbt_overlay_hud_follow) against the route it replaces, and nothing else.
A tracker replays reference clip 029 (tests/golden) up to the launch after which its leader holds the most phases.  Per format, in
one process, alternating: "follow" = HIP-event time of hud_follow_update + the panel draw of the batch (two launches, nothing
synchronised); "poll" = host-clock time of live poll + set_hud + the same draw + the synchronisation that ends it (the poll and
set_hud synchronise on their own), and of the poll + set_hud part alone.  Medians with min and max.  Then `track --one_pass
--video_format mjpeg` on a synthetic clip with and without --live_hud, alternating, frames per second of the whole command.

  python tools/overlay_bench.py [--frames 64] [--reps 20] [--warmup 5] [--hud | --hud_follow] [--size 1920x1080] [--out FILE.json]

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

H, W, FPS, TRAIL, IDS = 1080, 1920, 30.0, 120, 4


def make_rows(n_frames):
    """IDS plates on Lissajous paths, one row per plate and frame 1..n_frames (a step of about 15 pixels per frame at 1080p)"""
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


def make_phases(n_frames):
    """24 phases of equal length over frames 1..n_frames: eccentric and concentric in turn, 12 reps (the bar window is full)"""
    step = n_frames / 24.0
    return [((1 + i * step) / FPS, (1 + (i + 1) * step) / FPS, 0.3, 0.6, 0.4 + 0.01 * i, 1 - i % 2) for i in range(24)]


def replay_029(upto=None, chunk=64):
    """a tracker with live analysis that replayed clip 029 `chunk` frames per launch - all of it, or its first `upto` launches; returns
    (tracker, phases of the leader after every launch)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_tracker import _pack
    from test_oracle_ocsort import frames_from_rows
    from test_oracle_ocsort_corpus import load_all
    from vbt_amd.ocsort import MultiClipTracker
    fr, tm = frames_from_rows(load_all()["029"][0])
    dets, counts, times = _pack([fr], [tm])
    mc = MultiClipTracker(1, 8192, max_age=30, asso_func="diou", iou_threshold=0.1)
    mc.enable_live(path_cap=4096, phase_cap=128)
    seen = []
    for k, f0 in enumerate(range(0, len(fr), chunk)):
        if upto is not None and k >= upto:
            break
        mc.update_frames(dets[f0:f0 + chunk], counts[f0:f0 + chunk], times[f0:f0 + chunk])
        seen.append(len(mc.live()[0].phases))
    return mc, seen


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def hud_follow_bench(args, res):
    import tempfile
    import numpy as np
    import torch
    from click.testing import CliRunner
    from vbt_amd import synth
    from vbt_amd.cli import main as cli
    from vbt_amd.overlay import Overlay
    from vbt_amd.rawvideo import frame_shape
    B = args.frames
    _, seen = replay_029()
    best = max(range(len(seen)), key=lambda k: seen[k])
    mc, seen = replay_029(upto=best + 1)
    frame0 = (best + 1) * 64
    res["clip"] = {"name": "029", "launches_replayed": best + 1, "leader_phases": seen[-1], "frame0": frame0}
    prm = dict(x=16, y=16, scale=3)
    for fmt in ("rgb24", "nv12"):
        src = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B,) + frame_shape(fmt, H, W), dtype=np.uint8)).cuda()
        fol, sta = Overlay(H, W, fmt), Overlay(H, W, fmt)
        fol.hud_follow(mc, 0, FPS, **prm)
        t = {"follow": [], "poll_route": [], "poll_set_hud": []}
        for r in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fol.hud_follow_update(False, None)
            fol.draw(src.data_ptr(), B, frame0, 1, None)
            e1.record()
            e1.synchronize()
            a = e0.elapsed_time(e1) * 1e3
            t0 = time.perf_counter()
            rec = mc.live()[0]
            sta.set_hud(rec.phases, FPS, None, **prm)
            t1 = time.perf_counter()
            sta.draw(src.data_ptr(), B, frame0, 1, None)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if r >= args.warmup:
                t["follow"].append(a)
                t["poll_route"].append((t2 - t0) * 1e6)
                t["poll_set_hud"].append((t1 - t0) * 1e6)
        assert np.array_equal(fol.hud_table(), sta.hud_table()) and fol.hud_follow_status()[2] == 0
        res[fmt] = {"panel": [52 * prm["scale"], 50 * prm["scale"]], "phases": len(rec.phases),
                    "follow_update_plus_draw_us_events": spread(t["follow"]), "poll_set_hud_draw_sync_us_host": spread(t["poll_route"]),
                    "poll_set_hud_us_host": spread(t["poll_set_hud"])}
    T, S = 256, 416
    model = os.path.join(ROOT, "models", "efficientdet_lite0_synth.vbtm")
    fps_of = {"plain": [], "live_hud": []}
    with tempfile.TemporaryDirectory() as d:
        clip = os.path.join(d, "clip.npy")
        np.save(clip, synth.clip_frames(12, 0, T, size=S))
        for r in range(1 + 3):                                     # one warm-up round
            for name, extra in (("plain", []), ("live_hud", ["--live_hud"])):
                t0 = time.perf_counter()
                out = CliRunner().invoke(cli, ["track", clip, "--model", model, "--detection_treshold", "0.3", "--fps", "60", "--video_dir",
                                               os.path.join(d, name), "--video_format", "mjpeg", "--one_pass"] + extra)
                dt = time.perf_counter() - t0
                assert out.exit_code == 0, out.output
                if r:
                    fps_of[name].append(T / dt)
    res["track_one_pass_mjpeg"] = {"frames": T, "size": S, "frames_per_s": {k: spread(v) for k, v in fps_of.items()},
                                   "note": "whole command: model load, pipeline set-up and export included"}


def main():
    global H, W
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hud", action="store_true", help="also time the draw with a rep panel set")
    ap.add_argument("--hud_follow", action="store_true", help="time the panel that follows the live analysis against poll + set_hud, and nothing else")
    ap.add_argument("--size", default=f"{W}x{H}", help="frame size WIDTHxHEIGHT")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.lower().split("x"))
    import numpy as np
    import torch
    from vbt_amd.overlay import Overlay
    from vbt_amd.rawvideo import frame_shape
    if not torch.cuda.is_available():
        raise SystemExit("overlay_bench: no GPU - a timing taken anywhere else says nothing")
    so = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = ctypes.CDLL(so if os.path.exists(so) else "libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    B = args.frames
    frame0 = TRAIL + 1                                            # every row of the batch has a full trail
    rows = make_rows(TRAIL + B)
    stream = torch.cuda.current_stream().cuda_stream
    res = {"frames": B, "H": H, "W": W, "rows_per_frame": IDS, "trail": TRAIL, "reps": args.reps, "device": torch.cuda.get_device_name(0)}

    def finish():
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")

    if args.hud_follow:
        hud_follow_bench(args, res)
        return finish()

    def timed(fn, k=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k                      # microseconds

    for fmt in ("rgb24", "nv12"):
        shape = (B,) + frame_shape(fmt, H, W)
        src = torch.from_numpy(np.random.default_rng(0).integers(0, 256, shape, dtype=np.uint8)).cuda()
        dst = torch.empty_like(src)
        nbytes = src.numel()
        ov = Overlay(H, W, fmt)
        t0 = time.perf_counter()
        ov.set_rows(rows, FPS, stream)
        set_rows_us = (time.perf_counter() - t0) * 1e6

        ovh = None
        if args.hud:
            ovh = Overlay(H, W, fmt)
            ovh.set_rows(rows, FPS, stream)
            ovh.set_hud(make_phases(TRAIL + B), FPS, stream)

        def draw():
            ov.draw(src.data_ptr(), B, frame0, 1, stream)

        def draw_hud():
            ovh.draw(src.data_ptr(), B, frame0, 1, stream)

        def copy():
            rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream)      # hipMemcpyDeviceToDevice
            assert rc == 0, rc
        before = src.clone()
        draw()
        torch.cuda.synchronize()
        written = int((src != before).sum().item())               # bytes the draw changed on noise (a lower bound of what it writes)
        del before
        t = {"draw": [], "draw10": [], "copy": [], "hud": [], "hud10": []}
        for r in range(args.warmup + args.reps):
            one = {"draw": timed(draw), "copy": timed(copy), "draw10": timed(draw, 10)}
            if ovh is not None:
                one.update({"hud": timed(draw_hud), "hud10": timed(draw_hud, 10)})
            if r >= args.warmup:
                for k, v in one.items():
                    t[k].append(v)
        med = {k: statistics.median(v) for k, v in t.items() if v}
        res[fmt] = {"batch_bytes": nbytes, "bytes_changed_by_draw": written, "changed_share": written / nbytes,
                    "draw_us": med["draw"], "draw_us_min": min(t["draw"]), "draw_us_max": max(t["draw"]), "draw_back_to_back_us": med["draw10"],
                    "draw_back_to_back_us_min": min(t["draw10"]), "draw_back_to_back_us_max": max(t["draw10"]), "copy_us": med["copy"],
                    "copy_us_min": min(t["copy"]), "copy_GBps": 2 * nbytes / med["copy"] / 1e3, "draw_over_copy": med["draw"] / med["copy"],
                    "set_rows_us": set_rows_us, "rows": len(rows["id"])}
        if ovh is not None:
            prm = dict(x=16, y=16, scale=3)
            res[fmt]["hud"] = {"panel": [52 * prm["scale"], 50 * prm["scale"]], "phases": 24,
                               "draw_us": med["hud"], "draw_us_min": min(t["hud"]), "draw_us_max": max(t["hud"]),
                               "draw_back_to_back_us": med["hud10"], "draw_back_to_back_us_min": min(t["hud10"]),
                               "draw_back_to_back_us_max": max(t["hud10"]), "increment_us": med["hud"] - med["draw"],
                               "increment_back_to_back_us": med["hud10"] - med["draw10"], "copy_us": med["copy"]}
    long_rows = make_rows(18000)
    ov = Overlay(H, W, "rgb24")
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        ov.set_rows(long_rows, FPS, stream)
        ts.append((time.perf_counter() - t0) * 1e6)
    res["set_rows_long"] = {"rows": len(long_rows["id"]), "us_median": statistics.median(ts), "note": "includes the numpy sort of the Python wrapper"}
    finish()


if __name__ == "__main__":
    main()
