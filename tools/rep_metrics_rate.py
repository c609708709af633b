"""What the rep metrics (vbt_tracker_rep_metrics_enable) cost, on one GPU at the benchmark's 64-clip shape.

64 tracker clips replay the boxes of the golden corpus (tests/golden/dfs_ocsort_all.npz), one frame of every clip per launch, as the
pipeline steps them.  Measured per leg:
  close_us       vbt_tracker_finish -> vbt_tracker_summary(_ex) returned: export id + rep analysis of 64 clips + the packed copy
  live_step_us   time per step of a tracker with live analysis on minus that of one without: live_analyze_kernel, per launch
Legs: `parent` (a library built from the parent commit, --parent_lib), `disabled` (this tree, metrics not enabled), `enabled`.
Every leg runs in a fresh child process (a library is loaded once per process); the driver alternates the legs --rounds times, each
child warming up once before it measures, and prints a markdown table of min / median / max per leg.

  python tools/rep_metrics_rate.py --parent_lib /path/to/parent/libvbt_hip.so [--rounds 5] [--frames 600]
  python tools/rep_metrics_rate.py --leg enabled          (one leg, one JSON line)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CLIPS = 64


def _boxes(frames):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_tracker import _pack
    from test_oracle_ocsort import frames_from_rows
    from test_oracle_ocsort_corpus import load_all
    corpus = load_all()
    names = sorted(corpus)
    data = [frames_from_rows(corpus[names[i % len(names)]][0]) for i in range(N_CLIPS)]
    dets, counts, times = _pack([d[0][:frames] for d in data], [d[1][:frames] for d in data])
    return np.ascontiguousarray(dets), np.ascontiguousarray(counts), np.ascontiguousarray(times)


def leg(name, frames):
    sys.path.insert(0, ROOT)
    from vbt_amd import _lib
    from vbt_amd.ocsort import MultiClipTracker
    if name == "parent":                                                             # the parent's library does not export the new entries
        for k in [k for k in _lib._SIGS if k.endswith("_ex") or "rep_metrics" in k or k in ("vbt_analyze_metrics", "vbt_set_summary")]:
            del _lib._SIGS[k]
    dets, counts, times = _boxes(frames)
    F = counts.shape[0]
    kw = dict(max_age=30, asso_func="diou", iou_threshold=0.1)
    live, bare = MultiClipTracker(N_CLIPS, 8192, **kw), MultiClipTracker(N_CLIPS, 8192, **kw)
    live.enable_live(path_cap=4096, phase_cap=128)
    if name == "enabled":
        live.enable_rep_metrics()
    sync = lambda: _lib.check(_lib.lib().vbt_device_synchronize(0))                  # noqa: E731

    def steps(mc):
        sync()
        t0 = time.perf_counter()
        for f in range(F):
            mc.update_frames(dets[f:f + 1], counts[f:f + 1], times[f:f + 1])
        sync()
        return (time.perf_counter() - t0) / F * 1e6

    def close(mc):
        t0 = time.perf_counter()
        mc.finish(0.45)
        out = mc.summary_ex(cap=64) if name == "enabled" else mc.summary(cap=64)
        return (time.perf_counter() - t0) * 1e6, int(out[2].sum())

    res = None
    for rnd in range(2):                                                             # round 0 warms up
        live.reset()
        bare.reset()
        with_live, without = steps(live), steps(bare)
        close_us, phases = close(live)
        res = dict(leg=name, frames=F, phases=phases, step_live_us=with_live, step_bare_us=without, live_step_us=with_live - without, close_us=close_us)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["parent", "disabled", "enabled"])
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=600)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.frames)
    legs = (["parent"] if a.parent_lib else []) + ["disabled", "enabled"]
    runs = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k in legs:
            env = dict(os.environ)
            if k == "parent":
                env["VBT_LIB_PATH"] = a.parent_lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", k, "--frames", str(a.frames)],
                                 env=env, check=True, capture_output=True, text=True, timeout=300).stdout
            runs[k].append(json.loads(out.strip().splitlines()[-1]))
            print(k, runs[k][-1], file=sys.stderr, flush=True)
    print("| leg | close_us min / median / max | live_step_us min / median / max | step with live, us (median) | phases |")
    print("|---|---|---|---|---|")
    for k in legs:
        c, s = [r["close_us"] for r in runs[k]], [r["live_step_us"] for r in runs[k]]
        print(f"| {k} | {min(c):.1f} / {statistics.median(c):.1f} / {max(c):.1f} | {min(s):.2f} / {statistics.median(s):.2f} / {max(s):.2f} | "
              f"{statistics.median(r['step_live_us'] for r in runs[k]):.2f} | {runs[k][0]['phases']} |")


if __name__ == "__main__":
    main()
