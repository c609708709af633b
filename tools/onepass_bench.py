#!/usr/bin/env python3
"""One-pass export (track_frames(one_pass=True): upload or decode once, detect, track, draw from the tracker's device row log, encode)
against the two-pass export it stands beside (track, read the rows back, then overlay.render over the clip again).

Fixed setup: 64-frame batches of 1920x1080 (--batches of them), the synthetic scene of tools/mjpeg_bench.py, a Motion-JPEG sink at
quality 85; --warmup rounds, then median and range of --reps; one-pass and two-pass alternate inside one process, round by round.
  a  a .npy source (memory-mapped, as `track` opens it)
  b  an .avi source with restart markers (this project's own export of the clip)
  c  an .avi source without restart markers (the clip as Pillow writes it)
Per case and arm: frames/s of the whole call, host to file, and the bytes that went host -> device (the pipeline's own uploads, the
copies of vbt_memcpy and the compressed bytes handed to the decoder).  The rows and the .avi of both arms are compared.
draw: HIP-event time of follow_update + draw of one 64-frame batch - 4 rows per frame with full 120-point bar paths, the rows of
tools/mjpeg_bench.py, as a device log - against the draw of the same rows in sorted mode: follow mode's grid has 25 row slots per frame
whatever the frame holds, and that is on record here.

  python tools/onepass_bench.py [--batches 2] [--reps 7] [--warmup 2] [--cases abc] [--out FILE.json]

Prints one JSON line."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mjpeg_bench import FPS, H, TRAIL, W, make_rows, scene, spread  # noqa: E402

B, QUALITY = 64, 85
MODEL = os.path.join(ROOT, "models", "efficientdet_lite0_synth.vbtm")


class H2D:
    """bytes that cross the bus host -> device during one track_frames call"""

    def __init__(self):
        from vbt_amd import _lib, mjpeg, track
        self.L, self.track, self.mjpeg = _lib.lib(), track, mjpeg
        self.copied = self.compressed = 0
        self.pipes = []

    def __enter__(self):
        memcpy, Pipeline, decode, me = self.L.vbt_memcpy, self.track.Pipeline, self.mjpeg.Decoder.decode, self

        def counting_memcpy(dst, src, n, kind):
            if kind == 0:
                me.copied += int(n)
            return memcpy(dst, src, n, kind)

        class CountedPipeline(Pipeline):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                me.pipes.append(self)

        def counting_decode(dec, jpegs, *a, **kw):
            me.compressed += sum(len(j) for j in jpegs)
            return decode(dec, jpegs, *a, **kw)
        self._undo = (memcpy, Pipeline, decode)
        self.L.vbt_memcpy, self.track.Pipeline, self.mjpeg.Decoder.decode = counting_memcpy, CountedPipeline, counting_decode
        return self

    def __exit__(self, *exc):
        self.L.vbt_memcpy, self.track.Pipeline, self.mjpeg.Decoder.decode = self._undo

    def total(self):
        return self.copied + self.compressed + sum(int(p.info().h2d_bytes) for p in self.pipes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from vbt_amd import _lib
    from vbt_amd.cli import _open_source
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.mjpeg import AviWriter, Encoder, frame_rate
    from vbt_amd.ocsort import ROW_DTYPE
    from vbt_amd.overlay import Overlay, render
    from vbt_amd.track import track_frames
    if not torch.cuda.is_available():
        raise SystemExit("onepass_bench: no GPU - a timing taken anywhere else says nothing")
    tmp = args.dir or tempfile.mkdtemp(prefix="onepass_bench_")
    os.makedirs(tmp, exist_ok=True)
    T = B * args.batches
    clip = np.concatenate([scene(B, "rgb24")] * args.batches)
    res = {"frames": T, "batch": B, "H": H, "W": W, "quality": QUALITY, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "clip_bytes": int(clip.nbytes)}
    paths = {}
    if "a" in args.cases:
        paths["a_npy"] = os.path.join(tmp, "src.npy")
        np.save(paths["a_npy"], clip)
    if "b" in args.cases:
        paths["b_avi_restart"] = os.path.join(tmp, "src_rst.avi")
        with AviWriter(paths["b_avi_restart"], W, H, *frame_rate(FPS)) as sink:
            render(clip, make_rows(0), FPS, batch=B, sink=sink, quality=QUALITY)
    if "c" in args.cases:
        paths["c_avi_no_restart"] = os.path.join(tmp, "src_norst.avi")
        with AviWriter(paths["c_avi_no_restart"], W, H, *frame_rate(FPS)) as sink:
            for f in clip:
                b = io.BytesIO()
                Image.fromarray(f).save(b, "JPEG", quality=QUALITY)
                sink.write(b.getvalue())
    del clip
    for name, path in paths.items():
        frames = _open_source(path, "rgb24", None)
        t = {"one_pass": [], "two_pass": []}
        h2d, rows, out_bytes = {}, {}, {}
        for r in range(args.warmup + args.reps):
            for arm in ("one_pass", "two_pass"):
                out = os.path.join(tmp, f"out_{arm}.avi")
                with H2D() as count:
                    t0 = time.perf_counter()
                    with AviWriter(out, W, H, *frame_rate(FPS)) as sink:
                        rows[arm] = track_frames(frames, MODEL, fps=FPS, time_batch=B, video_sink=sink, video_quality=QUALITY, one_pass=arm == "one_pass")
                    dt = time.perf_counter() - t0
                    h2d[arm] = count.total()
                if r >= args.warmup:
                    t[arm].append(dt)
                with open(out, "rb") as fh:
                    out_bytes[arm] = fh.read()
        res[name] = {"source_bytes": os.path.getsize(path), "rows": len(rows["one_pass"]["id"]),
                     "same_rows": rows["one_pass"] == rows["two_pass"], "same_avi": out_bytes["one_pass"] == out_bytes["two_pass"],
                     "one_pass_fps": spread([T / v for v in t["one_pass"]]), "two_pass_fps": spread([T / v for v in t["two_pass"]]),
                     "speedup": float(np.median(t["two_pass"]) / np.median(t["one_pass"])),
                     "h2d_bytes": h2d}
        del frames
    # the draw itself: one batch of frames TRAIL + 1 .. TRAIL + B, every row with a full bar path
    data = make_rows(TRAIL + B)
    log = np.zeros(len(data["id"]), ROW_DTYPE)
    for k in log.dtype.names:
        log[k] = data[k]
    log = log[np.lexsort((log["id"], log["time"]))]
    old = int((log["time"] * FPS < TRAIL + 0.5).sum())
    stream = torch.cuda.current_stream().cuda_stream
    src = DeviceBuffer(B * H * W * 3)
    rows_dev = DeviceBuffer.from_host(log)
    count_dev = DeviceBuffer.from_host(np.array([old], np.int32))
    L = _lib.lib()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                          # microseconds
    sorted_ov = Overlay(H, W)
    sorted_ov.set_rows(data, FPS, stream)
    fol = Overlay(H, W)
    d = {"follow_update_draw_us": [], "follow_update_us": [], "follow_draw_us": [], "sorted_draw_us": []}
    for r in range(args.warmup + args.reps):
        def set_count(n):
            c = np.array([n], np.int32)
            _lib.check(L.vbt_memcpy(count_dev.ptr, c.ctypes.data, 4, 0))
        set_count(old)                                            # the rows before the batch are consumed ahead of the clock,
        fol.follow(rows_dev.ptr, count_dev.ptr, len(log), TRAIL + B, 25, FPS)
        fol.follow_update(stream)
        torch.cuda.synchronize()
        set_count(len(log))                                       # the batch's rows (4 x 64) inside it

        def both():
            fol.follow_update(stream)
            fol.draw(src.ptr, B, TRAIL + 1, 1, stream)
        one = {"follow_update_draw_us": timed(both)}
        assert fol.follow_status(stream) == (len(log), 0)
        one["follow_draw_us"] = timed(lambda: fol.draw(src.ptr, B, TRAIL + 1, 1, stream))
        one["sorted_draw_us"] = timed(lambda: sorted_ov.draw(src.ptr, B, TRAIL + 1, 1, stream))
        fol.follow(rows_dev.ptr, count_dev.ptr, len(log), TRAIL + B, 25, FPS)
        one["follow_update_us"] = timed(lambda: fol.follow_update(stream))          # the whole log, 736 rows, in one update
        if r >= args.warmup:
            for k, v in one.items():
                d[k].append(v)
    res["draw"] = dict({k: spread(v) for k, v in d.items()}, rows_per_frame=4, batch_rows=len(log) - old, log_rows=len(log), row_slots_per_frame=25)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
