#!/usr/bin/env python3
"""Cost of `eval` over a directory of .jpg files: decoded with Pillow on the host and uploaded as frames (--jpeg_decode host, the route
before the GPU decoder) against decoded on the GPU straight to the network input (--jpeg_decode auto).

The directory is the reference test set's mix: 59 images of 416 x 416 at 4:2:0 and 5 of 1080 x 1920 at 4:4:4, written with Pillow at
--quality from the smooth-gradients-under-noise pattern of tests/mjpeg_dec_ref.py, the large ones spread through the list.
  eval     evaluate.detections_table over the directory, the two arms alternating round by round in one process: images/s (the whole
           call: pipeline creation, file reads, decode, detector, matcher, table read-back) and host -> device bytes of the images;
           the two tables must be equal.  `..._without_create`: the same less `create_s`, the median of three timings of what every call
           spends making the pipeline and the matcher, the same in both arms.  Host -> device bytes: the decoded frames (host arm), the
           decoder's packed buffers (GPU arm).
  stages   the decoder's stage times on the batches `eval` cuts the directory into, from a handle of this tool's own, HIP events
           (VBT_MJPEG_DECODE_STAMPS=1), summed over the batches of a round: H2D copy, memsets, marker scan, entropy decode, IDCT,
           upsampling + colour + resize.
  fused    the 1080 x 1920 frames alone, --fused_frames of them: vbt_jpeg_stills_decode_resized against vbt_jpeg_stills_decode followed by
           vbt_resize_frames on the device, alternating - the last stage's event time of each (fused: colour + resize in one kernel;
           unfused: the colour kernel), the resize kernel's time from the wall clock of --resize_launches back-to-back launches, and the
           wall time of each whole path with one synchronisation.  The outputs must be equal.
Median, minimum and maximum of --reps rounds after --warmup.

  python tools/eval_jpeg_bench.py [--reps 7] [--warmup 2] [--quality 85] [--fused_frames 5] [--out FILE.json]

Prints one JSON line."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["VBT_MJPEG_DECODE_STAMPS"] = "1"

from mjpeg_bench import spread  # noqa: E402

STAGES = ("h2d_copy", "memsets", "marker_scan", "entropy_decode", "idct", "last_stage")
VOC = ("<annotation><filename>{name}</filename><size><width>{w}</width><height>{h}</height><depth>3</depth></size><object><name>barbell</name>"
       "<bndbox><xmin>{x0}</xmin><xmax>{x1}</xmax><ymin>{y0}</ymin><ymax>{y1}</ymax></bndbox></object></annotation>")


def write_dataset(d, quality):
    """-> (names in order, total file bytes, total decoded bytes)"""
    import mjpeg_dec_ref as D
    kinds = [((416, 416), 2)] * 59
    for at in (6, 19, 32, 45, 58):                                                  # the five large files, spread through the list
        kinds.insert(at, ((1080, 1920), 0))
    names, nbytes, raw = [], 0, 0
    for k, ((h, w), sub) in enumerate(kinds):
        name = f"img_{k:03d}.jpg"
        data = D.pil_jpeg(D.smooth(h, w, k), quality=quality, subsampling=sub)
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
        with open(os.path.join(d, f"img_{k:03d}.xml"), "w") as f:
            f.write(VOC.format(name=name, h=h, w=w, x0=w // 4, x1=3 * w // 4, y0=h // 4, y1=3 * h // 4))
        names.append(name)
        nbytes += len(data)
        raw += h * w * 3
    return names, nbytes, raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--fused_frames", type=int, default=5)
    ap.add_argument("--resize_launches", type=int, default=20)
    ap.add_argument("--model", default=os.path.join(ROOT, "models", "efficientdet_lite0_synth.vbtm"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from vbt_amd import _lib, evaluate
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.stills import JpegStills, blocks, plan
    from vbt_amd.track import Pipeline
    L = _lib.lib()
    if L.vbt_device_count() < 1:
        raise SystemExit("eval_jpeg_bench: no GPU - a timing taken anywhere else says nothing")
    d = tempfile.mkdtemp(prefix="eval_jpeg_bench_")
    try:
        names, file_bytes, raw_bytes = write_dataset(d, args.quality)
        ann = evaluate.read_annotations(d)
        images = [(n, os.path.join(d, n)) for n in names]
        n = len(images)
        res = {"images": n, "quality": args.quality, "reps": args.reps, "file_bytes": file_bytes, "decoded_bytes": raw_bytes}
        created = []
        for _ in range(3):
            t0 = time.perf_counter()
            pipe = Pipeline(args.model, evaluate.BATCH, max_frames=1, detection_treshold=0.0)
            ev = evaluate.Evaluator(n * evaluate.MAX_DETECTIONS, evaluate.BATCH)
            L.vbt_device_synchronize(0)
            created.append(time.perf_counter() - t0)
            size = pipe._size
            del pipe, ev
        create_s = res["create_s"] = sorted(created)[1]
        srt = evaluate.SortedImages(images)
        batches = plan([srt.heads[k][2] for k in srt.stills], evaluate.BATCH, evaluate.STILLS_MAX_BLOCK_BUDGET)
        own = JpegStills(evaluate.BATCH, max(sum(srt.heads[k][2] for k in srt.stills[i0:i1]) for i0, i1 in batches))
        net = DeviceBuffer(evaluate.BATCH * size * size * 3)
        uploaded, stage_rounds = 0, []
        for r in range(args.warmup + args.reps):
            ms, uploaded = [0.0] * 6, 0
            for i0, i1 in batches:
                own.decode_resized([srt.data[k] for k in srt.stills[i0:i1]], net.ptr, size, size, swap_rb=True)
                if own.status().any():
                    raise SystemExit("eval_jpeg_bench: a scan status is not 0")
                ms = [a + b for a, b in zip(ms, own.stage_ms())]
                uploaded += own.uploaded_bytes()
            if r >= args.warmup:
                stage_rounds.append([v * 1e3 for v in ms])
        del own, net
        arms = {a: {"s": [], "work_s": [], "h2d": h2d} for a, h2d in (("host", raw_bytes), ("auto", uploaded))}
        tables = {}
        for r in range(args.warmup + args.reps):
            for arm, p in arms.items():
                t0 = time.perf_counter()
                table, order = evaluate.detections_table(args.model, images, ann, jpeg_decode=arm)
                t = time.perf_counter() - t0
                first = np.searchsorted(table["image"], np.arange(len(order) + 1))
                tables[arm] = {k: (table["score"][first[i]:first[i + 1]].tobytes(), table["iou"][first[i]:first[i + 1]].tobytes()) for i, k in enumerate(order)}
                if r >= args.warmup:
                    p["s"].append(t)
                    p["work_s"].append(t - create_s)
        res["tables_equal"] = tables["host"] == tables["auto"]
        for arm, p in arms.items():
            res[arm] = {"images_per_s": spread([n / v for v in p["s"]]), "seconds": spread(p["s"]), "h2d_bytes": p["h2d"],
                        "images_per_s_without_create": spread([n / v for v in p["work_s"]]), "seconds_without_create": spread(p["work_s"])}
        res["auto"]["stage_us"] = {k: spread([s[i] for s in stage_rounds]) for i, k in enumerate(STAGES)}
        res["auto_over_host"] = spread([h / a for h, a in zip(arms["host"]["s"], arms["auto"]["s"])])       # per round: the two alternate
        res["auto_over_host_without_create"] = spread([h / a for h, a in zip(arms["host"]["work_s"], arms["auto"]["work_s"])])

        # ---- fused colour + resize against colour, then resize
        big = [open(os.path.join(d, k), "rb").read() for k in names if evaluate.jpeg_header(os.path.join(d, k))[0] == 1080]
        big = (big * (args.fused_frames // len(big) + 1))[:args.fused_frames]
        B, H, W = len(big), 1080, 1920
        dec = JpegStills(B, sum(blocks(j) for j in big))
        full, small_f, small_u = DeviceBuffer(B * H * W * 3), DeviceBuffer(B * size * size * 3), DeviceBuffer(B * size * size * 3)
        offs = np.arange(B + 1, dtype=np.uint64) * (H * W * 3)

        def resize():
            _lib.check(L.vbt_resize_frames(full.ptr, B, H, W, 1, small_u.ptr, size, size, 1, 0, 0, None))

        t = {k: [] for k in ("fused_last_stage_us", "unfused_colour_us", "resize_us", "fused_path_s", "unfused_path_s", "fused_kernels_us", "unfused_kernels_us")}
        for r in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            dec.decode_resized(big, small_f.ptr, size, size)
            ok = not dec.status().any()
            tf = time.perf_counter() - t0
            msf = dec.stage_ms()
            t0 = time.perf_counter()
            dec.decode(big, full.ptr, offs)
            resize()
            ok = ok and not dec.status().any()
            tu = time.perf_counter() - t0
            msu = dec.stage_ms()
            t0 = time.perf_counter()
            for _ in range(args.resize_launches):
                resize()
            _lib.check(L.vbt_device_synchronize(0))
            tr = (time.perf_counter() - t0) / args.resize_launches
            if r >= args.warmup:
                for k, v in (("fused_last_stage_us", msf[5] * 1e3), ("unfused_colour_us", msu[5] * 1e3), ("resize_us", tr * 1e6), ("fused_path_s", tf), ("unfused_path_s", tu),
                             ("fused_kernels_us", sum(msf[2:]) * 1e3), ("unfused_kernels_us", sum(msu[2:]) * 1e3 + tr * 1e6)):
                    t[k].append(v)
        res["fused"] = dict({k: spread(v) for k, v in t.items()}, frames=B, target=size, status_all_zero=bool(ok),
                            outputs_equal=bool(np.array_equal(small_f.to_host((B, size, size, 3), np.uint8), small_u.to_host((B, size, size, 3), np.uint8))),
                            full_frame_bytes=B * H * W * 3)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
