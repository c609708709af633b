"""Crowd-size inputs of the tracker tests (tests/test_crowd_cases_host.py on the CPU, tests/test_gpu_tracker_crowd.py on the device):
seeded, deterministic scenes with up to 25 detections per frame and up to 64 live tracks, and the numpy oracles' replays of them
(oracle/ocsort_np.py, tests/sort_ref.py) with `linear_assignment` and `associate` wrapped, so that every cost matrix the solver saw is
on record together with the call site it came from.  Every builder returns (frames, times) in the format of
tests/test_gpu_tracker.py:_random_scene: at most 25 detections [x1,y1,x2,y2,score,cls] per frame, at most 80 frames.  Replays are
computed once per process and never modified.

  A  full house: 64 objects on an 8 x 8 grid (pitch 0.11) born in three disjoint groups of 25 / 25 / 14 that cycle through frames 0-8
     with 0.06 boxes; then the boxes grow by 0.01 a frame to 0.15, neighbours overlap above the 0.1 threshold and every frame goes to
     the solver with 25 detections against 64 tracks.  From frame 9 on a frame holds 12 "runners" (the same objects for 8 frames, so
     that their hit streaks reach min_hits and rows are emitted) and the 13 objects that have waited longest.
  B  scene A's schedule (every object is seen at least every fourth frame, so it holds under max_age = 3) with a closing part: a
     group of 8 objects - list positions 0, 1, 2, 30, 31, 40, 41, 63 - leaves after frame 32 and dies in one frame; 8 new objects
     are then born in a ninth row.  Object 0 zig-zags while it is a runner: its id has the longest path when it dies.
  C  more detections than tracks: 30 overlapping objects, half of them missed in any frame; under max_age = 0 a missed track dies
     at once, so the track count follows the previous frame's detection count.
  D  recovery en masse: two groups of 8 fast objects vanish for four frames each and come back next to their last observations, far
     from where the filter has taken them; the first return meets three never-observed tracks besides (fewer unmatched detections
     than tracks), the second comes with 5 extra detections (more).
  E  exact ties: a cluster of 10 overlapping objects in which every other frame repeats one detection byte for byte; one-shot
     detections leave tracks that are never observed, and a recovery as in D meets them in the second association.
"""
import collections
import contextlib
import functools

import numpy as np

import sort_ref
from oracle import ocsort_np as oc

MAXD, MAXT = 25, 64
COLS = ["time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width"]
PITCH, ORIGIN = 0.11, 0.08
LEAVERS = (0, 1, 2, 30, 31, 40, 41, 63)          # scene B: the objects (= list positions) that leave together
B_LEAVE, B_ARRIVE = 33, 37                        # first frame without them (they die in frame 36); first frame of the 8 new objects


def _det(cx, cy, w, h, score):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, score, 0.0]


def _times(n):
    return (np.arange(n) + 1) / 30.0


def _finish(frames):
    assert len(frames) <= 80 and all(len(f) <= MAXD for f in frames)
    return [np.asarray(f, np.float64).reshape(-1, 6) for f in frames], _times(len(frames))


def _grid_centre(o):
    """objects 0..63 on the 8 x 8 grid, 64..71 in a ninth row far below it: so far that DIoU with any box
    of the grid stays under the 0.1 threshold and the second association leaves a detection there alone"""
    return ORIGIN + PITCH * (o % 8), ORIGIN + PITCH * (o // 8) + (1.8 if o >= 64 else 0.0)


def _house(seed, n_frames, runners, gone=lambda f: (), arrivals=lambda f: (), wanderer=None):
    """The schedule of scenes A and B.  runners(f): the 12 objects seen in every frame of a block; gone(f): objects no longer
    seen; arrivals(f): objects of the ninth row that exist from frame f on."""
    rng = np.random.default_rng(seed)
    groups = [list(range(0, 25)), list(range(25, 50)), list(range(50, 64))]
    stale = np.zeros(72, int)
    frames = []
    for f in range(n_frames):
        present = [o for o in range(64) if o not in gone(f)] + list(arrivals(f))
        if f < 9:
            seen = groups[f % 3]
        else:
            run = [o for o in runners(f) if o in present]
            rest = sorted((o for o in present if o not in run), key=lambda o: (-stale[o], o))
            seen = run + rest[:MAXD - len(run)]
            seen = [seen[i] for i in rng.permutation(len(seen))]          # detection order is not list order
        size = 0.06 if f < 9 else min(0.15, 0.06 + 0.01 * (f - 8))
        d = []
        for o in seen:
            cx, cy = _grid_centre(o)
            jx, jy = rng.normal(0, 0.0015, 2)
            if o == wanderer:
                jx += 0.012 * (1 if f % 2 else -1)
            w, h = size * (1 + rng.normal(0, 0.01, 2))
            d.append(_det(cx + jx, cy + jy, w, h, rng.uniform(0.5, 0.99)))
        stale += 1
        stale[seen] = 0
        frames.append(d)
    return _finish(frames)


def _runners_a(f):
    """blocks of 8 frames; object 63 (list position 63) runs in blocks 1 and 5 and waits its turn in the others"""
    first = (0, 52, 20, 36, 8, 52, 24, 40)[((f - 9) // 8) % 8]
    return list(range(first, first + 12))


def scene_a(n_frames=70):
    return _house(101, n_frames, _runners_a)


def _runners_b(f):
    if f < B_LEAVE:
        return list(LEAVERS) + [10, 20, 35, 45]
    return list(range(64, 72)) + [10, 20, 35, 45]


def scene_b(n_frames=52):
    return _house(202, n_frames, _runners_b, gone=lambda f: LEAVERS if f >= B_LEAVE else (),
                  arrivals=lambda f: range(64, 72) if f >= B_ARRIVE else (), wanderer=0)


def free_place_births(frames, times, k, seed=303):
    """scene A with one more frame: k detections in the ninth row, where no track is, and the runners of the last block"""
    rng = np.random.default_rng(seed)
    f = len(frames)
    d = [_det(*_grid_centre(64 + j), 0.06, 0.06, rng.uniform(0.5, 0.99)) for j in range(k)]
    for o in _runners_a(f - 1):
        cx, cy = _grid_centre(o)
        d.append(_det(cx, cy, 0.15, 0.15, rng.uniform(0.5, 0.99)))
    return _finish([list(map(list, fr)) for fr in frames] + [d])


def scene_c(seed=404, n_frames=60):
    rng = np.random.default_rng(seed)
    frames = []
    for f in range(n_frames):
        d = []
        for o in range(30):
            if rng.random() < 0.5:
                continue
            cx, cy = 0.15 + 0.12 * (o % 6) + rng.normal(0, 0.004), 0.2 + 0.12 * (o // 6) + rng.normal(0, 0.004)
            w, h = 0.16 * (1 + rng.normal(0, 0.02, 2))
            d.append(_det(cx, cy, w, h, rng.uniform(0.5, 0.99)))
        frames.append(d[:MAXD])
    return _finish(frames)


def _movers(rng, f, n, lane0, t0, hidden, x0=0.1, pitch=0.06, w=0.08, h=0.05):
    """n fast objects in lanes of their own, there from frame t0 on: 0.03 a frame to the right, not seen during `hidden`, back next to
    their last observations (not on them) and then to the left"""
    a, b = hidden
    if f < t0 or a <= f < b:
        return []
    x = x0 + 0.03 * (min(f, a - 1) - t0)
    if f >= b:
        x -= 0.004 + 0.03 * (f - b)
    return [_det(x + 0.002 * o + rng.normal(0, 0.0005), lane0 + pitch * o + rng.normal(0, 0.0005), w, h, rng.uniform(0.5, 0.99)) for o in range(n)]


def scene_d(seed=505, n_frames=44):
    rng = np.random.default_rng(seed)
    frames = []
    for f in range(n_frames):
        d = _movers(rng, f, 8, 0.04, 0, (10, 14)) + _movers(rng, f, 8, 0.52, 16, (26, 30))
        d += [_det(0.93, 0.2 + 0.3 * s + rng.normal(0, 0.001), 0.07, 0.1, rng.uniform(0.5, 0.99)) for s in range(3)]      # always seen
        if f == 5:                                  # seen once: three tracks that never get an observation
            d += [_det(0.6 + 0.08 * j, 0.1 + 0.25 * j, 0.05, 0.05, rng.uniform(0.5, 0.99)) for j in range(3)]
        if f == 30:                                 # extra detections on the frame of the second return
            d += [_det(0.62 + 0.07 * j, 0.9 - 0.22 * j, 0.05, 0.05, rng.uniform(0.5, 0.99)) for j in range(5)]
        frames.append([d[i] for i in rng.permutation(len(d))])
    return _finish(frames)


def scene_e(seed=606, n_frames=46):
    rng = np.random.default_rng(seed)
    frames = []
    for f in range(n_frames):
        d = []
        for o in range(10):
            cx, cy = 0.55 + 0.1 * (o % 5) + rng.normal(0, 0.002), 0.3 + 0.1 * (o // 5) + rng.normal(0, 0.002)
            d.append(_det(cx, cy, 0.14, 0.14, rng.uniform(0.5, 0.99)))
        if f % 2 == 0:
            d.insert(int(rng.integers(0, 10)), list(d[(f // 2) % 10]))      # the same box and score twice
        d += _movers(rng, f, 6, 0.55, 0, (16, 20), x0=0.05, pitch=0.09, h=0.07)
        if f in (12, 26):                           # seen once: three tracks without an observation
            d += [_det(0.1 + 0.12 * j, 0.08 + 0.1 * (f == 26), 0.05, 0.05, rng.uniform(0.5, 0.99)) for j in range(3)]
        frames.append(d)
    return _finish(frames)


def random_scene(seed, n_frames=80):
    """an ordinary clip (2-6 objects): the first frames of tests/sort_cases.py's recipe"""
    import sort_cases
    frames, times = sort_cases.random_scene(seed)
    return frames[:n_frames], times[:n_frames]


# name -> (builder, the max_age its conditions are stated under); every replay runs at iou_threshold 0.1
SCENES = {"A": (scene_a, 30), "B": (scene_b, 3), "C": (scene_c, 0), "D": (scene_d, 30), "E": (scene_e, 30)}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name][0]()


# ---- instrumented replays ----

Call = collections.namedtuple("Call", "site frame cost pairs")          # site: "first" / "second" association; frame: stepped frame
Step = collections.namedtuple("Step", "out ids kfx before")             # update()'s rows; track ids and kf.x in list order; ids before
Replay = collections.namedtuple("Replay", "rows steps calls stats")


@contextlib.contextmanager
def _recording(calls, frame):
    """oc.linear_assignment and oc.associate wrapped for the duration: every cost matrix with its call site"""
    solve, assoc = oc.linear_assignment, oc.associate
    site = ["second"]

    def linear_assignment(cost):
        pairs = solve(cost)
        calls.append(Call(site[0], frame[0], np.array(cost), np.array(pairs)))
        return pairs

    def associate(*a, **k):
        site[0] = "first"
        try:
            return assoc(*a, **k)
        finally:
            site[0] = "second"

    oc.linear_assignment, oc.associate = linear_assignment, associate
    try:
        yield
    finally:
        oc.linear_assignment, oc.associate = solve, assoc


def _replay(trk, frames, times, sort):
    rows = {k: [] for k in ["id"] + COLS}
    steps, calls, frame = [], [], [0]
    with _recording(calls, frame):
        for f, (d, t) in enumerate(zip(frames, times)):
            if len(d) == 0:
                continue
            frame[0] = f
            before = [k.id for k in trk.trackers]
            if sort:
                calls_before = len(calls)
                out = trk.update(d)
                for i in range(calls_before, len(calls)):
                    calls[i] = calls[i]._replace(site="first")           # SORT has one association
            else:
                out = trk.update(np.asarray(d, np.float64), [])
            kfx = {k.id: k.kf.x.flatten().copy() for k in trk.trackers}
            for xmin, ymin, xmax, ymax, tid, _, _ in out:
                tid = int(tid)
                dx, dy = kfx[tid - 1][4:6]
                for k, v in zip(["id"] + COLS, (tid, t, (xmin + xmax) / 2, (ymin + ymax) / 2, dx, dy, abs(ymax - ymin), abs(xmax - xmin))):
                    rows[k].append(v)
            steps.append(Step(np.array(out), [k.id for k in trk.trackers], np.array([kfx[k.id] for k in trk.trackers]).reshape(-1, 7), before))
    stats = dict(getattr(trk, "stats", {}), frame_count=trk.frame_count)
    return Replay({k: np.asarray(v) for k, v in rows.items()}, steps, calls, stats)


def replay_ocsort_on(frames, times, **kw):
    """the oracle of oracle/ocsort_np.py:track_boxes, stepped frame by frame and recorded"""
    kw.setdefault("max_age", 30)
    kw.setdefault("asso_func", "diou")
    kw.setdefault("iou_threshold", 0.1)
    return _replay(oc.OCSort(**kw), frames, times, False)


def replay_sort_on(frames, times, **kw):
    kw.setdefault("max_age", 30)
    return _replay(sort_ref.SortTracker(**kw), frames, times, True)


@functools.lru_cache(maxsize=None)
def replay(tracker, item, max_age):
    """tracker: "diou" / "iou" (OC-SORT with that second-association function) or "sort"; item: a scene's name, or the seed of an
    ordinary clip that sits between crowd clips under their parameters"""
    fr, tm = random_scene(item) if isinstance(item, int) else scene(item)
    if tracker == "sort":
        return replay_sort_on(fr, tm, max_age=max_age, iou_threshold=0.1)
    return replay_ocsort_on(fr, tm, max_age=max_age, iou_threshold=0.1, asso_func=tracker)


def replay_ocsort(name, asso="diou"):
    return replay(asso, name, SCENES[name][1])


def replay_sort(name):
    return replay("sort", name, SCENES[name][1])


# ---- what the conditions are stated in ----

def live_counts(rep):
    return [len(s.ids) for s in rep.steps]


def rows_per_step(rep):
    return [len(s.out) for s in rep.steps]


def emitted_ids(step):
    """0-based ids of the tracks that emitted a row in this step"""
    return [int(r[4]) - 1 for r in step.out]


def deaths(rep):
    """[(step index, live tracks at the deletion, [list positions deleted])] of every step that deleted a track"""
    out = []
    for i, s in enumerate(rep.steps):
        gone = [p for p, tid in enumerate(s.before) if tid not in s.ids]
        if gone:
            out.append((i, len(s.before) + len([t for t in s.ids if t not in s.before]), gone))
    return out


def has_twin_lines(cost):
    """two identical rows or two identical columns"""
    c = np.asarray(cost)
    return len(np.unique(c, axis=0)) < c.shape[0] or len(np.unique(c, axis=1)) < c.shape[1]


def export_rule(rows):
    """the id the reference's export picks (track.py:107-115): largest cumulative path among the ids with a step, as
    tests/test_gpu_tracker.py:test_finish_selects_id_and_phases_for_reference_clip states it; also the path lengths"""
    cum = {}
    for tid in np.unique(rows["id"]):
        m = rows["id"] == tid
        d = np.sqrt(np.diff(rows["x"][m]) ** 2 + np.diff(rows["y"][m]) ** 2)
        if len(d):
            cum[int(tid)] = d.sum()
    return (max(cum, key=cum.get) if cum else -1), cum


def pack(clips):
    """[(frames, times)] -> dets [F,n,25,6], counts [F,n], times [F,n] (padded with empty frames)"""
    n, F = len(clips), max(len(f) for f, _ in clips)
    dets, counts, times = np.zeros((F, n, MAXD, 6)), np.zeros((F, n), np.int32), np.zeros((F, n))
    for c, (fr, tm) in enumerate(clips):
        for f, d in enumerate(fr):
            counts[f, c] = len(d)
            dets[f, c, :len(d)] = d
            times[f, c] = tm[f]
    return dets, counts, times


def as_detector_output(frames):
    """a scene as the detector writes it - float32 boxes (ymin,xmin,ymax,xmax) [F,25,4], scores [F,25], counts [F] - and the float64
    detections the tracker makes of them (tests/test_gpu_sort.py:f32_scene)"""
    n = len(frames)
    boxes, scores, counts = np.zeros((n, MAXD, 4), np.float32), np.zeros((n, MAXD), np.float32), np.zeros(n, np.int32)
    dets = []
    for f, d in enumerate(frames):
        counts[f] = len(d)
        boxes[f, :len(d)] = d[:, [1, 0, 3, 2]]
        scores[f, :len(d)] = d[:, 4]
        b, s = boxes[f, :len(d)].astype(np.float64), scores[f, :len(d)].astype(np.float64)
        dets.append(np.stack([b[:, 1], b[:, 0], b[:, 3], b[:, 2], s, np.zeros(len(d))], 1).reshape(-1, 6))
    return boxes, scores, counts, dets


# ---- the detector-format paths (device; also run from a child process, which imports this module) ----

UNEVEN_RUNS = (1, 7, 2, 13, 5, 6, 9, 3)          # run lengths, cycled: below and above the 6 frames from which a run keeps the state in LDS


def run_lengths(n, plan):
    out, i = [], 0
    while sum(out) < n:
        out.append(min(plan[i % len(plan)], n - sum(out)))
        i += 1
    return out


def detector_path_logs(tracker, max_age, boxes, scores, counts, forms):
    """{form: (row log of MultiClipTracker.rows, status)} of one clip stepped from float32 detector outputs on the device.  forms:
    "fused" - vbt_tracker_update_from_detections, one frame per call; "seq" - vbt_tracker_update_from_detections_seq as ONE run;
    "runs" - the same in runs of UNEVEN_RUNS frames.  Frame f carries the time (f + 1) / 30."""
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.ocsort import MultiClipTracker
    from vbt_amd.sort import MultiClipSortTracker
    L = _lib.lib()
    n = len(counts)
    b, s, c = (DeviceBuffer.from_host(np.ascontiguousarray(x)) for x in (boxes, scores, counts))
    logs = {}
    for form in forms:
        if tracker == "sort":
            mc = MultiClipSortTracker(1, 4096, max_age=max_age, iou_threshold=0.1)
        else:
            mc = MultiClipTracker(1, 4096, max_age=max_age, iou_threshold=0.1, asso_func=tracker)
        if form == "fused":
            for f in range(n):
                t = np.array([(f + 1) / 30.0], np.float64)
                _lib.check(L.vbt_tracker_update_from_detections(mc.handle, b.ptr + f * MAXD * 16, s.ptr + f * MAXD * 4, c.ptr + f * 4, t.ctypes.data, 0.25, None))
        else:
            f0 = 0
            for length in ([n] if form == "seq" else run_lengths(n, UNEVEN_RUNS)):
                ra = (_lib.Run * 1)(_lib.Run(0, f0, 1, length, f0 + 1, 1, 30.0))
                _lib.check(L.vbt_tracker_update_from_detections_seq(mc.handle, b.ptr, s.ptr, c.ptr, n, ra, 1, 0.25, None))
                f0 += length
        logs[form] = (mc.rows(0), mc.status(0))
    return logs
