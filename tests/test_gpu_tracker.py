"""GPU parity of the on-device tracker + rep analysis (through the C ABI):
  * against the reference's committed DataFrames (bit-exact Kalman velocities, phases)
  * against the numpy / python oracles on seeded random scenes (every row, bit-exact)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
COLS = ["time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width"]


def _clip_frames(clip):
    from test_oracle_ocsort import frames_from_rows, load_clip
    g = load_clip(clip)
    frames, times = frames_from_rows(g)
    return g, frames, times


def _pack(frames_list, times_list):
    """list over clips of (frames, times) -> dets [F,n,25,6], counts [F,n], times [F,n] (padded with empty frames)."""
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


def test_replay_reference_clips_bit_exact_vs_golden_and_oracle():
    """5 reference clips tracked in ONE launch (one wavefront per clip)."""
    from oracle import ocsort_np as oc
    from test_oracle_ocsort import SEGMENTS
    from vbt_amd.ocsort import MultiClipTracker
    clips = ["001", "002", "005", "008", "030"]
    data = [_clip_frames(c) for c in clips]
    dets, counts, times = _pack([d[1] for d in data], [d[2] for d in data])
    mc = MultiClipTracker(len(clips), 8192, max_age=30, asso_func="diou", iou_threshold=0.1)
    mc.update_frames(dets, counts, times)
    for ci, clip in enumerate(clips):
        g, frames, tm = data[ci]
        got = {k: np.asarray(v) for k, v in mc.rows(ci).items()}
        want = {k: np.asarray(v) for k, v in oc.track_boxes(frames, tm).items()}
        assert mc.status(ci)["overflow"] == 0
        for k in ["id"] + COLS:                      # the whole row log equals the oracle's, bit for bit
            assert np.array_equal(got[k], want[k]), (clip, k)
        for c2, tid, n in SEGMENTS:                  # and the reference's stored velocities where they are pinned
            if c2 != clip:
                continue
            rm, om = g["id"] == tid, got["id"] == tid
            for col in ("time", "dx", "dy", "x", "y"):
                assert np.array_equal(g[col][rm][:n], got[col][om][:n]), (clip, tid, col)


def _random_scene(seed, n_frames=160):
    """Crossing / appearing / disappearing / flickering boxes: exercises LAP, OCR, ORU, births, deaths."""
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
                continue                               # missed detection -> freeze / re-update paths
            c, s = pos[o], size[o] * (1 + rng.normal(0, 0.02, 2))
            d.append([c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2, rng.uniform(0.5, 0.99), 0.0])
        if rng.random() < 0.2:                          # clutter
            c, s = rng.uniform(0.1, 0.9, 2), rng.uniform(0.05, 0.15, 2)
            d.append([c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2, rng.uniform(0.5, 0.99), 0.0])
        frames.append(np.asarray(d, np.float64).reshape(-1, 6))
        times.append((f + 1) / 30.0)
    return frames, np.asarray(times)


@pytest.mark.parametrize("asso", ["diou", "iou"])
def test_random_scenes_equal_numpy_oracle(asso):
    from oracle import ocsort_np as oc
    from vbt_amd.ocsort import MultiClipTracker
    scenes = [_random_scene(s) for s in range(24)]
    dets, counts, times = _pack([s[0] for s in scenes], [s[1] for s in scenes])
    mc = MultiClipTracker(len(scenes), 4096, max_age=30, asso_func=asso, iou_threshold=0.1)
    mc.update_frames(dets, counts, times)
    nrows = 0
    for ci, (frames, tm) in enumerate(scenes):
        want = oc.track_boxes(frames, tm, asso_func=asso)
        got = mc.rows(ci)
        assert got["id"] == want["id"], ci
        for k in COLS:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (ci, k)
        nrows += len(got["id"])
    assert nrows > 5000


def test_ocsort_dropin_call_shape():
    """OCSort().update(dets, []) rows + tracker.trackers[i].id / .kf.x (reference track.py:186-199)."""
    from oracle import ocsort_np as oc
    from vbt_amd.ocsort import OCSort
    frames, tm = _random_scene(99, 120)
    a = OCSort(max_age=30, asso_func="diou", iou_threshold=0.1)
    b = oc.OCSort(max_age=30, asso_func="diou", iou_threshold=0.1)
    for d in frames:
        if len(d) == 0:
            continue
        ra, rb = a.update(d, []), b.update(d, [])
        assert np.array_equal(ra, rb)
        ta, tb = a.trackers, b.trackers
        assert [t.id for t in ta] == [t.id for t in tb]
        for x, y in zip(ta, tb):
            assert np.array_equal(x.kf.x, y.kf.x)


def test_the_two_read_back_paths_agree_frame_by_frame():
    """last_output / trackers after every frame, read two ways: handle A (one clip, one frame per call) is the one-frame kernel, whose
    packed block comes back with the call; handle B (two clips, the scene in clip 1) is the multi-clip kernel, read through a copy of the
    clip's state.  Both equal each other and the numpy oracle, bit for bit.  Seed 0's first 40 frames (picked with the oracle): two
    tracks die, up to 4 rows per frame, 7 frames without a detection (on those A is not stepped and reads through the state copy too)."""
    from oracle import ocsort_np as oc
    from vbt_amd.ocsort import MultiClipTracker
    frames, tm = _random_scene(0)
    frames, tm = frames[:40], tm[:40]
    kw = dict(max_age=30, asso_func="diou", iou_threshold=0.1)
    a, b, o = MultiClipTracker(1, 512, **kw), MultiClipTracker(2, 512, **kw), oc.OCSort(**kw)
    want, most, deaths, alive = np.empty((0, 7)), 0, 0, set()
    for d, t in zip(frames, tm):
        da, ca, ta = _pack([[d]], [[t]])
        db, cb, tb = _pack([[d[:0]], [d]], [[t], [t]])
        a.update_frames(da, ca, ta)
        b.update_frames(db, cb, tb)
        if len(d):                                    # (an empty frame steps nothing: track.py:180-181)
            want = o.update(d, [])
        (oa, va), (ob, vb) = a.last_output(0), b.last_output(1)
        assert np.array_equal(oa, ob) and np.array_equal(va, vb)
        assert np.array_equal(oa, want)
        kx = {k.id: k.kf.x.flatten() for k in o.trackers}
        assert np.array_equal(va, np.array([kx[int(r[4]) - 1][4:6] for r in want]).reshape(-1, 2))
        tka, tkb = a.trackers(0), b.trackers(1)
        assert [k.id for k in tka] == [k.id for k in tkb] == [k.id for k in o.trackers]
        for x, y, z in zip(tka, tkb, o.trackers):
            assert np.array_equal(x.kf.x, y.kf.x) and np.array_equal(x.kf.x, z.kf.x)
        most = max(most, len(oa))
        deaths += len(alive - set(kx))
        alive = set(kx)
    assert most >= 2 and deaths >= 1                  # not a degenerate scene
    assert b.status(0)["frame_count"] == 0 and b.rows(1) == a.rows(0)


def test_host_detection_filter_at_the_gate():
    """dets = dets[confs > det_thresh] of the host-provided detections, with confidences exactly at, one ulp below and one ulp above the
    gate, through the one-frame kernel (F == 1) and the multi-frame kernel (F > 1).  Frame 4 has detections but none passes: the tracker is
    still stepped, on no detections (frame_count counts it), as the reference's update() is."""
    from oracle import ocsort_np as oc
    from vbt_amd.ocsort import MultiClipTracker
    g = 0.2
    at, below, above = g, np.nextafter(g, 0.0), np.nextafter(g, 1.0)

    def box(cx, cy, conf):
        return [cx - 0.05, cy - 0.04, cx + 0.05, cy + 0.04, conf, 0.0]

    confs = [(above, 0.9, at), (above, below, above), (0.9, above, below), (at, below, at), (above, above, 0.9), (above, at, above)]
    frames = [np.array([box(0.2 + 0.01 * f, 0.3, c0), box(0.5, 0.5 + 0.01 * f, c1), box(0.8 - 0.01 * f, 0.7, c2)]) for f, (c0, c1, c2) in enumerate(confs)]
    tm = (np.arange(6) + 1) / 30.0
    kw = dict(det_thresh=g, max_age=30, min_hits=1, asso_func="diou", iou_threshold=0.1)       # min_hits 1: every matched track emits a row
    want = oc.track_boxes(frames, tm, **kw)
    one, many = MultiClipTracker(1, 512, **kw), MultiClipTracker(1, 512, **kw)
    for d, t in zip(frames, tm):
        one.update_frames(*_pack([[d]], [[t]]))
    many.update_frames(*_pack([frames], [tm]))
    ra, rb = one.rows(0), many.rows(0)
    assert ra == rb
    assert ra["id"] == want["id"] and len(ra["id"]) >= 6
    for k in COLS:
        assert np.array_equal(np.asarray(ra[k]), np.asarray(want[k])), k
    assert one.status(0)["frame_count"] == many.status(0)["frame_count"] == 6
    assert max(ra["id"]) == 3 and 4.0 / 30.0 not in ra["time"]      # a fourth track is never born: nothing at or below the gate gets through


def test_velocity_tracker_all_34_reference_clips():
    from vbt_amd.velocity import analyze_rows
    main = np.load(os.path.join(GOLDEN, "dfs_ocsort_main.npz"))
    with open(os.path.join(GOLDEN, "phases_ocsort.json")) as f:
        phases = json.load(f)
    for clip in sorted(k for k in phases if len(k) == 3):
        rows = np.stack([main[f"c{clip}_{c}"] for c in COLS], axis=1)
        got = analyze_rows(rows, 0.45, preprocess=True)
        want = phases[clip]["phases"]
        assert len(got) == len(want), clip
        for p, w in zip(got, want):
            assert [p.time_start, p.time_end, p.y_start, p.y_end, p.rom] == [float.fromhex(v) for v in w[:5]], clip
            assert p.type == w[5]


def test_velocity_tracker_class_streaming_and_edges():
    from oracle import velocity as ov
    from vbt_amd.velocity import VelocityTracker
    pre = np.load(os.path.join(GOLDEN, "pre_ocsort.npz"))
    rows = np.stack([pre[f"c001_{c}"] for c in COLS], axis=1)
    vt, ref = VelocityTracker(0.45), ov.VelocityTracker(0.45)
    assert vt.phases == []
    for i, r in enumerate(rows[:1500]):
        vt.process_measurements(*r)
        ref.process_measurements(*r)
        if i in (0, 1, 700, 1400):                    # mid-stream reads (no flush)
            assert [p.rom for p in vt.phases] == [p.rom for p in ref.phases]
    vt.end_processing()
    ref.end_processing()
    assert [(p.time_start, p.time_end, p.rom, p.type) for p in vt.phases] == [(p.time_start, p.time_end, p.rom, p.type) for p in ref.phases]
    assert abs(vt.phases[1].duration - (vt.phases[1].time_end - vt.phases[1].time_start)) == 0


def test_finish_selects_id_and_phases_for_reference_clip():
    """End-to-end tail of the hot path on reference data: row log -> export id (track.py:107-115) ->
    preprocessing + VelocityTracker on device -> the SURVEY 4.3 ACV table."""
    from vbt_amd.ocsort import MultiClipTracker
    g, frames, tm = _clip_frames("001")
    dets, counts, times = _pack([frames], [tm])
    mc = MultiClipTracker(1, 8192, max_age=30, asso_func="diou", iou_threshold=0.1)
    mc.update_frames(dets, counts, times)
    mc.finish(0.45)
    best, ph = mc.phases(0)
    # oracle for the same tail: numpy tracker rows -> max cumulative path id -> python rep analysis
    from oracle import ocsort_np as oc
    from oracle import velocity as ov
    rows = {k: np.asarray(v) for k, v in oc.track_boxes(frames, tm).items()}
    cum = {}
    for tid in np.unique(rows["id"]):
        m = rows["id"] == tid
        d = np.sqrt(np.diff(rows["x"][m]) ** 2 + np.diff(rows["y"][m]) ** 2)
        if len(d):
            cum[int(tid)] = d.sum()
    want_id = max(cum, key=cum.get)
    assert best == want_id == 1
    m = rows["id"] == want_id
    want = ov.analyze_track(*[rows[c][m].tolist() for c in COLS], plate_diameter=0.45)
    assert len(ph) == len(want) == 12
    for r, w in zip(ph, want):
        assert list(r) == w.as_row()
    conc = ph[ph[:, 5] == 0]
    acv = conc[:, 4] / (conc[:, 1] - conc[:, 0])
    # the replay lacks the ~20 observations the reference's min_hits rule hid after lost periods, so the ACVs
    # sit within 2e-3 m/s of the SURVEY 4.3 table rather than on it
    assert np.allclose(acv, [0.437798, 0.481084, 0.455869, 0.445342, 0.391556, 0.400236], atol=2e-3)


def test_whole_reference_corpus_replayed_on_the_device():
    """All 34 reference DataFrames (every id) replayed through the HIP tracker in ONE launch, one wavefront per clip:
    the row log equals the numpy oracle's bit for bit on every clip, and on the 22 single-track clips it IS the reference
    DataFrame (ids, emission order, time/x/y/dx/dy bit for bit) - see tests/test_oracle_ocsort_corpus.py for what the
    other 12 clips can and cannot pin."""
    from oracle import ocsort_np as oc
    from test_oracle_ocsort import frames_from_rows
    from test_oracle_ocsort_corpus import load_all, single_track_clips
    from vbt_amd.ocsort import MultiClipTracker
    corpus = load_all()
    clips = sorted(corpus)
    data = [frames_from_rows(corpus[c][0]) for c in clips]
    dets, counts, times = _pack([d[0] for d in data], [d[1] for d in data])
    mc = MultiClipTracker(len(clips), 8192, max_age=30, asso_func="diou", iou_threshold=0.1)
    mc.update_frames(dets, counts, times)
    clean = set(single_track_clips(corpus))
    assert len(clean) == 22
    for ci, clip in enumerate(clips):
        got = {k: np.asarray(v) for k, v in mc.rows(ci).items()}
        want = {k: np.asarray(v) for k, v in oc.track_boxes(*data[ci]).items()}
        assert mc.status(ci)["overflow"] == 0 and mc.status(ci)["rows_overflow"] == 0
        for k in ["id"] + COLS:
            assert np.array_equal(got[k], want[k]), (clip, k)
        if clip in clean:
            g = corpus[clip][0]
            order = np.argsort(g["index"])
            assert np.array_equal(got["id"], g["id"][order])
            for k in ("time", "x", "y", "dx", "dy"):
                assert np.array_equal(got[k], g[k][order]), (clip, k)
    # export id (reference track.py:107-115: the file name carries it) of every clip, selected on the device
    mc.finish(0.45)
    for ci, clip in enumerate(clips):
        assert mc.phases(ci)[0] == corpus[clip][1], clip
