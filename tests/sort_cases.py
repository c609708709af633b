"""Inputs the SORT tests share (tests/test_sort_ref_host.py on the CPU, tests/test_gpu_sort.py on the device): the reference's SORT
frames (tests/golden/dfs_sort.npz, tools/make_golden_sort.py), the detections rebuilt from the OC-SORT fixture, the seeded random
scenes, and the numpy reference's replays of both - computed once per process and never modified."""
import functools
import os

import numpy as np

import sort_ref
from conftest import GOLDEN

COLS = ["time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width"]
# the clips on which the replay's (id - id offset, time) key set IS the reference's (tools/make_golden_sort.py prints the table)
FULL_CLIPS = ("005", "007", "010", "014", "018", "021", "023", "024", "026", "030", "031", "033")
EARLY = 20                       # rows of a track in which the 1e-6 of OC-SORT's convert_bbox_to_z (the fixture's first box) is visible
# Tolerances against dfs/.  x, y: the centre of a posterior box that was itself recomputed from the filter state - the tool measured
# 1.11e-16 (half an ulp of 0.5..1), held with one decade of margin.  w, h: 2e-6 in a track's first EARLY rows (measured 9.8e-7: the first
# OC-SORT row of a track carries the 1e-6 of its convert_bbox_to_z, so the recovered first detection is off by that much), 1e-8 after
# (measured 8.8e-10).
TOL_XY, TOL_WH_EARLY, TOL_WH_LATE = 1.2e-15, 2e-6, 1e-8
SCENE_SEEDS = tuple(range(24))
SCENE_THRESHOLDS = (0.3, 0.1)


@functools.lru_cache(maxsize=None)
def fixture():
    """{clip: (columns dict incl. "id", id offset, export id)} of the clips stored in full"""
    a = np.load(os.path.join(GOLDEN, "dfs_sort.npz"))
    clips = sorted(k[1:4] for k in a.files if k.endswith("_full") and bool(a[k]))
    return {c: ({k: a[f"c{c}_{k}"] for k in ["id"] + COLS}, int(a[f"c{c}_offset"]), int(a[f"c{c}_export_id"])) for c in clips}


@functools.lru_cache(maxsize=None)
def clip_detections(clip):
    """(frames, times): per-frame float64 [x1,y1,x2,y2,score,cls] rebuilt from the OC-SORT rows of tests/golden/dfs_ocsort_all.npz -
    x -+ w/2, y -+ h/2 in float64, NOT rounded to float32 (tools/make_golden_sort.py: rounding loses the fit)"""
    a = np.load(os.path.join(GOLDEN, "dfs_ocsort_all.npz"))
    g = {k: a[f"c{clip}_{k}"] for k in COLS}
    times = np.unique(g["time"])
    frames = []
    for t in times:
        m = g["time"] == t
        x, y, w, h = g["x"][m], g["y"][m], g["norm_plate_width"][m], g["norm_plate_height"][m]
        frames.append(np.stack([x - w / 2, y - h / 2, x + w / 2, y + h / 2, np.full(len(x), 0.9), np.zeros(len(x))], 1))
    return frames, times


@functools.lru_cache(maxsize=None)
def clip_replay(clip):
    """(rows as arrays, counters) of the numpy reference on the clip, SortTracker(max_age=30) as in track.py:156"""
    rows, stats = sort_ref.track_boxes(*clip_detections(clip))
    return {k: np.asarray(v) for k, v in rows.items()}, stats


def check_against_dfs(clip, rows):
    """`rows` (columns as arrays, ids starting at 1) against the reference's frame of a fully matching clip, in the terms of
    tests/test_sort_ref_host.py.  Returns the number of rows compared."""
    g, offset, _ = fixture()[clip]
    ref = {(int(i) - offset, t): j for j, (i, t) in enumerate(zip(g["id"], g["time"]))}
    got = {(int(i), t): j for j, (i, t) in enumerate(zip(rows["id"], rows["time"]))}
    assert len(ref) == len(g["id"]) and len(got) == len(rows["id"]), clip              # keys are unique on both sides
    assert set(ref) == set(got), (clip, len(ref), len(got))                            # time and id - offset: exact on every row
    keys = sorted(ref)
    ri, gi = np.array([ref[k] for k in keys]), np.array([got[k] for k in keys])
    for c in ("dx", "dy"):
        assert np.array_equal(g[c][ri], rows[c][gi]), (clip, c)
    for c in ("x", "y"):
        err = np.abs(g[c][ri] - rows[c][gi]).max()
        assert err <= TOL_XY, (clip, c, err)
    first = {}
    rank = np.empty(len(g["id"]), int)
    for j, i in enumerate(g["id"]):                                                    # stored sorted by (id, time): row number inside the track
        rank[j] = first.setdefault(int(i), j)
    rank = np.arange(len(rank)) - rank
    for c in ("norm_plate_height", "norm_plate_width"):
        d = np.abs(g[c][ri] - rows[c][gi])
        early = rank[ri] < EARLY
        assert d[early].max() <= TOL_WH_EARLY and (not (~early).any() or d[~early].max() <= TOL_WH_LATE), (clip, c, d[early].max(), d[~early].max())
    return len(keys)


def random_scene(seed, n_frames=160):
    """Crossing / appearing / disappearing / flickering boxes with clutter (the recipe of tests/test_gpu_tracker.py:_random_scene):
    assignment-path frames, births, deaths, misses."""
    rng = np.random.default_rng(seed)
    nobj = int(rng.integers(2, 7))
    pos = rng.uniform(0.15, 0.85, (nobj, 2))
    vel = rng.normal(0, 0.006, (nobj, 2))
    size = rng.uniform(0.06, 0.2, (nobj, 2))
    life = [(int(rng.integers(0, 40)), int(rng.integers(80, n_frames))) for _ in range(nobj)]
    frames, times = [], []
    for f in range(n_frames):
        d = []
        for o in range(nobj):
            pos[o] += vel[o] + rng.normal(0, 0.002, 2)
            if not (life[o][0] <= f < life[o][1]) or rng.random() < 0.15:
                continue
            c, s = pos[o], size[o] * (1 + rng.normal(0, 0.02, 2))
            d.append([c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2, rng.uniform(0.5, 0.99), 0.0])
        if rng.random() < 0.2:
            c, s = rng.uniform(0.1, 0.9, 2), rng.uniform(0.05, 0.15, 2)
            d.append([c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2, rng.uniform(0.5, 0.99), 0.0])
        frames.append(np.asarray(d, np.float64).reshape(-1, 6))
        times.append((f + 1) / 30.0)
    return frames, np.asarray(times)


@functools.lru_cache(maxsize=None)
def scenes():
    return [random_scene(s) for s in SCENE_SEEDS]


@functools.lru_cache(maxsize=None)
def scene_replays(iou_threshold):
    """[(rows as arrays, counters)] of the numpy reference on every scene, SortTracker(max_age=10, iou_threshold)"""
    out = []
    for frames, tm in scenes():
        rows, stats = sort_ref.track_boxes(frames, tm, max_age=SCENE_MAX_AGE, iou_threshold=iou_threshold)
        out.append(({k: np.asarray(v) for k, v in rows.items()}, stats))
    return out


SCENE_MAX_AGE = 10               # objects leave between frames 80 and 160: with 10 every one of them dies inside the scene


def pack(frames_list, times_list):
    """list over clips of (frames, times) -> dets [F,n,25,6], counts [F,n], times [F,n] (padded with empty frames)"""
    n = len(frames_list)
    F = max(len(f) for f in frames_list)
    dets = np.zeros((F, n, 25, 6))
    counts = np.zeros((F, n), np.int32)
    times = np.zeros((F, n))
    for c, (fr, tm) in enumerate(zip(frames_list, times_list)):
        for f, d in enumerate(fr):
            counts[f, c] = len(d)
            dets[f, c, :len(d)] = d
            times[f, c] = tm[f]
    return dets, counts, times
