#!/usr/bin/env python3
"""tests/golden/dfs_sort.npz: the reference's SORT result set (reference dfs/*.pkl.gz, made with sort.tracker.SortTracker, the
commented-out alternative of track.py:16,156) as far as the numpy restatement tests/sort_ref.py can be held against it.
Run in the build container only (the reference never travels to the GPU box).  DATA ONLY: columns of the DataFrames.

The detections are not stored again: they are rebuilt from tests/golden/dfs_ocsort_all.npz (every emitted row of the OC-SORT
result set carries the detector's box: x -+ w/2, y -+ h/2 in float64), replayed through tests/sort_ref.py (max_age = 30) and compared
with dfs/ by the key (id - id offset, time); the id offset of a clip is its smallest id - 1 (the package's id counter is shared by
all trackers of a process, so the file ids run 1, 3, 7, ..., 94).  A clip whose key set matches completely is stored in full; of the
others (OC-SORT's min_hits hid detections from the fixture) the export id's rows are stored if the file stays within the size limit of
a committed file.  The table this prints is kept in profiles/sort_tracker.md."""
import glob
import os
import re
import sys

import numpy as np
import pandas as pd

REF = "/root/reference"
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import sort_ref  # noqa: E402

FN = re.compile(r"(\S*)_id(\d+)_(\S*)\.pkl\.gz")
COLS = ["time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width"]
SIZE_LIMIT = 1 << 20          # no committed file above 1 MiB
EARLY = 20                    # rows of a track in which the 1e-6 of OC-SORT's convert_bbox_to_z is still visible in w, h


def detections(a, clip):
    """per-frame [x1,y1,x2,y2,score,cls] from the OC-SORT rows (tests/test_oracle_ocsort.py:frames_from_rows)"""
    g = {k: a[f"c{clip}_{k}"] for k in COLS}
    times = np.unique(g["time"])
    frames = []
    for t in times:
        m = g["time"] == t
        x, y, w, h = g["x"][m], g["y"][m], g["norm_plate_width"][m], g["norm_plate_height"][m]
        frames.append(np.stack([x - w / 2, y - h / 2, x + w / 2, y + h / 2, np.full(len(x), 0.9), np.zeros(len(x))], 1))
    return frames, times


def compare(df, offset, rep):
    """per column: exact rows and the largest difference over the common keys (w, h split at row EARLY of each track)"""
    ref = {(int(i) - offset, t): j for j, (i, t) in enumerate(zip(df["id"].to_numpy(), df["time"].to_numpy()))}
    got = {(int(i), t): j for j, (i, t) in enumerate(zip(rep["id"], rep["time"]))}
    common = sorted(set(ref) & set(got))
    ri, gi = np.array([ref[k] for k in common], int), np.array([got[k] for k in common], int)
    rank = df.groupby("id").cumcount().to_numpy()[ri] if len(ri) else np.zeros(0, int)
    res = {"common": len(common), "same_keys": set(ref) == set(got)}
    for c in COLS:
        r, g = df[c].to_numpy()[ri], np.asarray(rep[c])[gi]
        d = np.abs(r - g)
        res[c] = (int((r == g).sum()), float(d.max()) if len(d) else 0.0)
        if c.startswith("norm_"):
            res[c + "_early"] = float(d[rank < EARLY].max()) if (rank < EARLY).any() else 0.0
            res[c + "_late"] = float(d[rank >= EARLY].max()) if (rank >= EARLY).any() else 0.0
    return res


def main():
    a = np.load(os.path.join(OUT, "dfs_ocsort_all.npz"))
    full, extra, table = {}, {}, []
    tot = {"rows": 0, "common": 0, "dx": 0, "dy": 0, "full_rows": 0}
    worst = {"x": 0.0, "y": 0.0, "h_early": 0.0, "w_early": 0.0, "h_late": 0.0, "w_late": 0.0}
    for f in sorted(glob.glob(os.path.join(REF, "dfs", "*.pkl.gz"))):
        m = FN.match(os.path.basename(f))
        if not m:
            continue
        video, tid, _ = m.groups()
        clip = video[:3]
        df = pd.read_pickle(f)                                     # sorted by (id, time), track.py:105
        offset = int(df["id"].min()) - 1
        frames, times = detections(a, clip)
        rep, stats = sort_ref.track_boxes(frames, times)
        r = compare(df, offset, rep)
        table.append((clip, len(df), len(rep["id"]), r, stats, offset))
        tot["rows"] += len(df)
        tot["common"] += r["common"]
        tot["dx"] += min(r["dx"][0], r["dy"][0])
        dst = full if r["same_keys"] else extra
        sel = df if r["same_keys"] else df[df["id"] == int(tid)]
        dst[f"c{clip}_id"] = sel["id"].to_numpy(np.int16)
        for c in COLS:
            dst[f"c{clip}_{c}"] = sel[c].to_numpy(np.float64)
        dst[f"c{clip}_offset"] = np.int16(offset)
        dst[f"c{clip}_export_id"] = np.int16(tid)
        dst[f"c{clip}_full"] = np.bool_(r["same_keys"])
        if r["same_keys"]:
            tot["full_rows"] += len(df)
            worst["x"], worst["y"] = max(worst["x"], r["x"][1]), max(worst["y"], r["y"][1])
            for k, c in (("h", "norm_plate_height"), ("w", "norm_plate_width")):
                worst[k + "_early"] = max(worst[k + "_early"], r[c + "_early"])
                worst[k + "_late"] = max(worst[k + "_late"], r[c + "_late"])
    print("| clip | id offset | rows dfs/ | rows replay | common keys | keys equal | time == | x == | y == | dx == | dy == | h == | w == | max abs x | max abs y |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for clip, n, nr, r, stats, offset in table:
        print(f"| {clip} | {offset} | {n} | {nr} | {r['common']} | {'yes' if r['same_keys'] else 'no'} | " +
              " | ".join(str(r[c][0]) for c in COLS) + f" | {r['x'][1]:.2e} | {r['y'][1]:.2e} |")
    n_full = sum(1 for t in table if t[3]["same_keys"])
    print(f"\nclips {len(table)}, fully matching {n_full} ({' '.join(t[0] for t in table if t[3]['same_keys'])}), rows in them {tot['full_rows']}")
    print(f"all clips: rows {tot['rows']}, common keys {tot['common']}, of them dx and dy exact {tot['dx']}")
    print("fully matching clips, largest differences: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f" (early = a track's first {EARLY} rows)")
    path = os.path.join(OUT, "dfs_sort.npz")
    np.savez_compressed(path, **full, **extra)
    kept = "kept"
    if os.path.getsize(path) > SIZE_LIMIT:
        np.savez_compressed(path, **full)
        kept = f"dropped (with them the file exceeds {SIZE_LIMIT} bytes)"
    print(f"dfs_sort.npz {os.path.getsize(path)} bytes; export-id rows of the {len(table) - n_full} other clips: {kept}")


if __name__ == "__main__":
    main()
