"""Streamed clips vs clips known up front, one process, one GPU (profiles/r06_stream.md).

The 34-clip corpus (tests/golden/corpus_meta.json frame counts and frame rates, synthetic frames as in bench.py's corpus leg) runs
  (a) all known up front: 34 tracker clips, shard.run_schedule over 64 detector slots, one vbt_pipeline_close + rows_all at the end
      (bench.py --full's corpus_1gpu);
  (b) streamed: 16 tracker slots, shard.stream_schedule, a slot closed with vbt_pipeline_close_clips when its clip ends and the next
      clip opened in it; every result read back (vbt_pipeline_closed_clip, rows included) as soon as it is ready.
The legs alternate three times after one warm-up each.  Prints one JSON line: frames/s of each leg (median over the repeats), the host
time inside vbt_pipeline_close_clips (median / max over all closes of the timed repeats) and the time from a close to its result being
ready, as seen by a poll after every step (so its resolution is one step, whose time is also reported), and the host time of the reads.
A result is read when a poll finds it ready, or - waiting - when its slot is about to be closed again.

  python tools/stream_bench.py [--reps 3] [--slots 64] [--concurrent 16] [--legs ab|a|b]
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
CORPUS_META = os.path.join(ROOT, "tests", "golden", "corpus_meta.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--concurrent", type=int, default=16)
    ap.add_argument("--legs", choices=("ab", "a", "b"), default="ab")
    args = ap.parse_args()
    import torch
    from vbt_amd import _lib, shard, synth
    from vbt_amd.track import Pipeline
    dev = torch.device("cuda:0")
    meta = json.load(open(CORPUS_META))
    keys = sorted(meta)
    lengths = np.array([meta[k][0] for k in keys])
    fps_c = np.array([meta[k][1] for k in keys], np.float64)
    U, slots, conc = 8, args.slots, args.concurrent
    base = np.stack([np.stack([synth.render(synth.background(int(k), 320), 11 * u) for u in range(U)]) for k in keys])
    reps_needed = -(-(U + slots) // U)
    fr = torch.from_numpy(np.concatenate([base] * reps_needed, axis=1)).to(dev)    # [clip][U * reps]: any run of <= slots frames fits

    def src(c, f0, nf):
        s = (f0 - 1) % U
        return fr[c, s:s + nf]

    L = _lib.lib()
    # (a) all known up front
    steps_a = shard.run_schedule(lengths, slots)
    pipe_a = Pipeline(MODEL, slots, max_frames=int(lengths.max()), fps=fps_c, tracker_clips=len(keys))
    out_a = {}

    def leg_a():
        pipe_a.reset()
        for step in steps_a:
            pipe_a.step_runs([src(c, f0, nf) for c, _, nf, f0 in step], step)
        b, r, _, o, _ = pipe_a.close(cap=512)
        pipe_a.rows_all()
        out_a.update(best=b.copy(), rows=r.copy(), overflow=o.copy())

    # (b) streamed through `conc` tracker slots
    steps_b = shard.stream_schedule(lengths, conc, slots)
    nxt = {}
    for t, (_, _, closes) in enumerate(steps_b):
        for s in closes:
            nxt[(t, s)] = next((c for opens, _, _ in steps_b[t + 1:] for sl, c in opens if sl == s), None)
    first = {sl: c for opens, _, _ in steps_b[:1] for sl, c in opens}
    pipe_b = Pipeline(MODEL, slots, max_frames=int(lengths.max()), fps=[fps_c[first.get(s, 0)] for s in range(conc)], tracker_clips=conc,
                      slot_close=True)
    close_us, ready_us, read_us, waits = [], [], [], [0]
    out_b = {}

    def leg_b(record):
        pipe_b.reset()
        pipe_b.fps[:] = [fps_c[first.get(s, 0)] for s in range(conc)]
        clip_of, unread = {}, {}

        def read(s, wait):
            r0 = time.perf_counter()
            got = pipe_b.closed(s, wait=wait)
            if got is None:
                return False
            c, t0 = unread.pop(s)
            if record:
                now = time.perf_counter()
                ready_us.append((now - t0) * 1e6)
                read_us.append((now - r0) * 1e6)
                waits[0] += int(wait)
            out_b[c] = (got[0], len(got[1]["id"]), got[3])
            return True

        for t, (opens, runs, closes) in enumerate(steps_b):
            for s, c in opens:
                clip_of[s] = c
            pipe_b.step_runs([src(clip_of[s], f0, nf) for s, _, nf, f0 in runs], runs)
            for s in list(unread):                   # finished results only: never waits
                read(s, False)
            if closes:
                for s in closes:                     # a result still unread when its slot closes again: the only wait
                    if s in unread:
                        read(s, True)
                cl = np.asarray(closes, np.int32)
                nf = np.asarray([fps_c[nxt[(t, s)]] if nxt[(t, s)] is not None else pipe_b.fps[s] for s in closes], np.float64)
                t0 = time.perf_counter()
                _lib.check(L.vbt_pipeline_close_clips(pipe_b._h, cl.ctypes.data, len(cl), nf.ctypes.data))
                t1 = time.perf_counter()
                if record:
                    close_us.append((t1 - t0) * 1e6)
                pipe_b.fps[cl] = nf
                for s in closes:
                    unread[s] = (clip_of.pop(s), t1)
        for s in list(unread):
            read(s, True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    total = int(lengths.sum())
    if args.legs != "b":
        timed(leg_a)
    if args.legs != "a":
        timed(lambda: leg_b(False))
    ta, tb = [], []
    for _ in range(args.reps):
        if args.legs != "b":
            ta.append(timed(leg_a))
        if args.legs != "a":
            tb.append(timed(lambda: leg_b(True)))
    if args.legs != "ab":                            # (one leg: for a kernel trace of that leg alone)
        print(json.dumps({"legs": args.legs, "frames_per_s": [total / x for x in ta + tb]}))
        return
    fa, fb = [total / x for x in ta], [total / x for x in tb]
    equal = all(out_b[c] == (int(out_a["best"][c]), int(out_a["rows"][c]), int(out_a["overflow"][c])) for c in range(len(keys)))
    res = {
        "metric": "stream_vs_upfront_corpus",
        "frames": total, "clips": len(keys), "detector_slots": slots, "tracker_slots_streamed": conc,
        "upfront_frames_per_s": float(np.median(fa)), "streamed_frames_per_s": float(np.median(fb)),
        "upfront_runs": [round(x, 1) for x in fa], "streamed_runs": [round(x, 1) for x in fb],
        "streamed_over_upfront": float(np.median(fb) / np.median(fa)),
        "close_clips_host_us_median": float(np.median(close_us)), "close_clips_host_us_max": float(np.max(close_us)),
        "closes_timed": len(close_us),
        "close_to_ready_us_median": float(np.median(ready_us)),
        "read_host_us_median": float(np.median(read_us)), "read_host_ms_per_rep": float(np.sum(read_us) / args.reps / 1e3),
        "reads_that_waited": waits[0],
        "streamed_us_per_step": float(np.median(tb) / len(steps_b) * 1e6),
        "steps_upfront": len(steps_a), "steps_streamed": len(steps_b),
        "results_equal": bool(equal),
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
