"""The trackers on the device at crowd size - 25 detections against 64 live tracks, deaths and slot reuse in a full list, mass
recovery, exact ties, the 65th birth and a full row log - against the numpy oracles (oracle/ocsort_np.py, tests/sort_ref.py), bit for
bit.  The scenes and the oracles' replays are tests/crowd_cases.py; tests/test_crowd_cases_host.py asserts, without a device, that the
scenes reach the code these tests are about."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import crowd_cases as cc
from conftest import ROOT

pytestmark = pytest.mark.gpu
COLS = cc.COLS
TRACKERS = ("diou", "iou", "sort")
# clips of one launch (they share the tracker's parameters): crowd scenes side by side and an ordinary clip between two of them
GROUPS = {30: ("A", 3, "D", "E"), 3: ("B", 5, "A"), 0: ("C", 7, "E")}


def _tracker(kind, n_clips, rows_cap, max_age):
    from vbt_amd.ocsort import MultiClipTracker
    from vbt_amd.sort import MultiClipSortTracker
    if kind == "sort":
        return MultiClipSortTracker(n_clips, rows_cap, max_age=max_age, iou_threshold=0.1)
    return MultiClipTracker(n_clips, rows_cap, max_age=max_age, iou_threshold=0.1, asso_func=kind)


def _clip(item):
    return cc.random_scene(item) if isinstance(item, int) else cc.scene(item)


def _assert_rows(got, want, what):
    """a row log as MultiClipTracker.rows returns it against a replay's rows"""
    assert np.array_equal(np.asarray(got["id"]), want["id"]), what
    for k in COLS:
        assert np.array_equal(np.asarray(got[k], np.float64), want[k], equal_nan=True), (what, k)


def _assert_state(mc, clip, rep, what):
    """status() and the track list (ids in list order, every kf.x) against the replay's last step"""
    st = mc.status(clip)
    last = rep.steps[-1]
    assert (st["rows"], st["trackers"], st["frame_count"]) == (len(rep.rows["id"]), len(last.ids), rep.stats["frame_count"]), (what, st)
    assert st["overflow"] == 0 and st["rows_overflow"] == 0, (what, st)
    tk = mc.trackers(clip)
    assert [k.id for k in tk] == last.ids, what
    assert np.array_equal(np.array([k.kf.x.flatten() for k in tk]).reshape(-1, 7), last.kfx, equal_nan=True), what


# ---- 1. host detections, all frames of all clips in one launch ----

@pytest.mark.parametrize("max_age", sorted(GROUPS))
@pytest.mark.parametrize("kind", TRACKERS)
def test_crowd_clips_in_one_launch_equal_the_oracle(kind, max_age):
    items = GROUPS[max_age]
    reps = [cc.replay(kind, it, max_age) for it in items]
    assert all(max(cc.live_counts(r)) <= cc.MAXT for r in reps)                    # the oracle knows no capacity: stay within the device's
    mc = _tracker(kind, len(items), 1024, max_age)
    mc.update_frames(*cc.pack([_clip(it) for it in items]))
    for ci, (it, rep) in enumerate(zip(items, reps)):
        _assert_rows(mc.rows(ci), rep.rows, (kind, max_age, it))
        _assert_state(mc, ci, rep, (kind, max_age, it))


# ---- 2. the one-frame kernel: the full-size view ----

def test_one_frame_kernel_at_64_tracks():
    """OCSort.update, one frame per call: update()'s rows, the ids in list order and every kf.x after every frame of scene A (68
    frames with 64 tracks, up to 25 rows: the whole 2 + 25 * 9 + 64 * 8 doubles of the view are in use)"""
    from vbt_amd.ocsort import OCSort
    frames, tm = cc.scene("A")
    rep = cc.replay("diou", "A", 30)
    a = OCSort(max_age=30, asso_func="diou", iou_threshold=0.1, rows_cap=1024)
    for f, (d, t, want) in enumerate(zip(frames, tm, rep.steps)):
        out = a.update(d, [], time=t)
        assert np.array_equal(out, want.out), f
        tk = a.trackers
        assert [k.id for k in tk] == want.ids, f
        assert np.array_equal(np.array([k.kf.x.flatten() for k in tk]), want.kfx), f
    assert len(a.trackers) == cc.MAXT
    _assert_rows(a.multi.rows(0), rep.rows, "one frame per call")


# ---- 3. the detector-format paths ----

CHILD = (
    "import pickle, sys\n"
    "sys.path.insert(0, sys.argv[3])\n"
    "import crowd_cases as cc\n"
    "jobs = pickle.load(open(sys.argv[1], 'rb'))\n"
    "pickle.dump([cc.detector_path_logs(*j) for j in jobs], open(sys.argv[2], 'wb'))\n")


@pytest.fixture(scope="module")
def detector_scenes():
    """scenes A and B as float32 detector outputs, and the oracle on the float64 detections the tracker makes of them"""
    out = {}
    for name in ("A", "B"):
        frames, tm = cc.scene(name)
        boxes, scores, counts, dets = cc.as_detector_output(frames)
        rep = cc.replay_ocsort_on(dets, tm, max_age=cc.SCENES[name][1], iou_threshold=0.1, asso_func="diou")
        assert max(cc.live_counts(rep)) == cc.MAXT and cc.live_counts(rep).count(cc.MAXT) >= 30      # rounding to float32 keeps the house full
        out[name] = (boxes, scores, counts, rep)
    return out


def _check_detector_logs(logs, rep, what):
    for form, (rows, st) in logs.items():
        _assert_rows(rows, rep.rows, (what, form))
        assert (st["rows"], st["trackers"], st["overflow"], st["rows_overflow"], st["frame_count"]) == \
            (len(rep.rows["id"]), len(rep.steps[-1].ids), 0, 0, rep.stats["frame_count"]), (what, form, st)


@pytest.mark.parametrize("name", ["A", "B"])
def test_detector_format_paths(detector_scenes, name):
    """one frame per call, one run of all frames, runs of uneven lengths (state in LDS from 6 frames on)"""
    boxes, scores, counts, rep = detector_scenes[name]
    logs = cc.detector_path_logs("diou", cc.SCENES[name][1], boxes, scores, counts, ("fused", "seq", "runs"))
    _check_detector_logs(logs, rep, name)


def test_detector_format_paths_with_the_state_in_global_memory(detector_scenes, tmp_path):
    """VBT_SEQ_NO_LDS is read once per process: the time-batched walks of both scenes again in a child process that sets it"""
    src, dst = str(tmp_path / "in.pkl"), str(tmp_path / "out.pkl")
    jobs = [("diou", cc.SCENES[n][1], *detector_scenes[n][:3], ("seq", "runs")) for n in ("A", "B")]
    with open(src, "wb") as f:
        pickle.dump(jobs, f)
    subprocess.run([sys.executable, "-c", CHILD, src, dst, os.path.dirname(os.path.abspath(__file__))], check=True, cwd=ROOT,
                   env={**os.environ, "VBT_SEQ_NO_LDS": "1"}, timeout=120)
    for n, logs in zip(("A", "B"), pickle.load(open(dst, "rb"))):
        _check_detector_logs(logs, detector_scenes[n][3], (n, "no LDS"))


# ---- 4. clip close ----

@pytest.mark.parametrize("asso", ["diou", "iou"])
def test_finish_exports_a_dead_id_after_scene_b(asso):
    """the export id (reference track.py:107-115) is one of the eight tracks that died together: it comes out of best_id / best_cum, not
    out of the 64 live tracks; its phases are oracle/velocity.py's on its rows"""
    from oracle import velocity as ov
    rep = cc.replay(asso, "B", 3)
    mc = _tracker(asso, 2, 1024, 3)
    mc.update_frames(*cc.pack([cc.scene("B"), cc.random_scene(5)]))
    assert mc.status(0)["trackers"] == cc.MAXT
    mc.finish(0.45)
    best, ph = mc.phases(0)
    want_id, cum = cc.export_rule(rep.rows)
    assert best == want_id and want_id - 1 not in rep.steps[-1].ids              # dead at the close
    m = rep.rows["id"] == want_id
    want = ov.analyze_track(*[rep.rows[c][m].tolist() for c in COLS], plate_diameter=0.45)
    assert len(ph) == len(want)
    for r, w in zip(ph, want):
        assert list(r) == w.as_row()
    other = cc.replay(asso, 5, 3)
    assert mc.phases(1)[0] == cc.export_rule(other.rows)[0]
    best_ids, n_rows, _, ovf, _ = mc.summary()
    assert list(best_ids) == [want_id, cc.export_rule(other.rows)[0]] and list(n_rows) == [len(rep.rows["id"]), len(other.rows["id"])]
    assert list(ovf) == [0, 0]


# ---- 5. capacity: the 65th track ----

def test_65th_track_is_counted_not_stored():
    """scene A, then a frame with births in free places: the births beyond 64 are counted in `overflow`, the clip's read-backs refuse
    with the capacity error, the clips next to it never notice, and a reset gives the slot a fresh clip"""
    from oracle import ocsort_np as oc
    from vbt_amd import _lib
    frames, tm = cc.free_place_births(*cc.scene("A"), 5)
    o = oc.OCSort(max_age=30, asso_func="diou", iou_threshold=0.1)
    for d in frames[:-1]:
        o.update(d, [])
    before = [k.id for k in o.trackers]
    o.update(frames[-1], [])
    assert len(before) == cc.MAXT and [k.id for k in o.trackers][:cc.MAXT] == before       # no track dies in that frame
    k = len(o.trackers) - cc.MAXT
    assert k == 5
    left, right = cc.replay("diou", 3, 30), cc.replay("diou", "D", 30)
    mc = _tracker("diou", 3, 1024, 30)
    mc.update_frames(*cc.pack([cc.random_scene(3), (frames, tm), cc.scene("D")]))
    st = mc.status(1)
    assert st["overflow"] == k and st["trackers"] == cc.MAXT and st["frame_count"] == len(frames)
    assert [t.id for t in mc.trackers(1)] == before
    msg = f"clip 1: more than 64 live tracks \\({k} births dropped\\)"
    with pytest.raises(_lib.VbtError, match=msg):
        mc.rows(1)
    mc.finish(0.45)
    with pytest.raises(_lib.VbtError, match=msg):
        mc.phases(1)
    ovf = mc.summary()[3]
    assert ovf[1] != 0 and ovf[0] == 0 and ovf[2] == 0
    for ci, rep in ((0, left), (2, right)):
        _assert_rows(mc.rows(ci), rep.rows, ("neighbour", ci))
        _assert_state(mc, ci, rep, ("neighbour", ci))
    # the same slot again, from scratch
    mc.reset_clips([1])
    assert mc.status(1) == dict(rows=0, trackers=0, overflow=0, rows_overflow=0, frame_count=0)
    c_frames, c_tm = cc.scene("C")
    empty = ([f[:0] for f in c_frames], c_tm)
    mc.update_frames(*cc.pack([empty, (c_frames, c_tm), empty]))
    again = cc.replay("diou", "C", 30)
    _assert_rows(mc.rows(1), again.rows, "after reset_clips")
    _assert_state(mc, 1, again, "after reset_clips")
    _assert_rows(mc.rows(0), left.rows, "neighbour after the reset")


# ---- 6. capacity: a full row log ----

def test_full_row_log_keeps_tracking_and_spares_the_next_clip():
    from vbt_amd import _lib
    from vbt_amd.ocsort import LIVE_ROWS_LOST, ROW_DTYPE
    rep, other = cc.replay("diou", "A", 30), cc.replay("diou", 3, 30)
    per_step = cc.rows_per_step(rep)
    cum = np.cumsum(per_step)
    s = next(i for i in range(1, len(per_step)) if cum[i - 1] >= 300 and per_step[i] >= 5)
    cap = int(cum[s - 1]) + 3                                                     # the log fills inside step s, which emits 5 rows or more
    total = len(rep.rows["id"])
    assert cap >= len(other.rows["id"]) and total - cap >= 100
    mc = _tracker("diou", 2, cap, 30)
    mc.enable_live()
    mc.update_frames(*cc.pack([cc.scene("A"), cc.random_scene(3)]))
    st = mc.status(0)
    assert st["rows"] == cap and st["rows_overflow"] == total - cap and st["overflow"] == 0
    assert st["frame_count"] == rep.stats["frame_count"]
    tk = mc.trackers(0)                                                           # tracking went on after the log was full
    assert [k.id for k in tk] == rep.steps[-1].ids
    assert np.array_equal(np.array([k.kf.x.flatten() for k in tk]), rep.steps[-1].kfx)
    ptr, nptr, dev_cap = mc.rows_dev(0)
    assert dev_cap == cap
    log, n = np.zeros(cap, ROW_DTYPE), np.zeros(1, np.int32)
    _lib.check(_lib.lib().vbt_memcpy(log.ctypes.data, ptr, log.nbytes, 1))
    _lib.check(_lib.lib().vbt_memcpy(n.ctypes.data, nptr, 4, 1))
    assert n[0] == cap
    assert np.array_equal(log["id"], rep.rows["id"][:cap])
    for k in COLS:
        assert np.array_equal(log[k], rep.rows[k][:cap]), k
    _assert_rows(mc.rows(1), other.rows, "the clip behind the full log")
    _assert_state(mc, 1, other, "the clip behind the full log")
    with pytest.raises(_lib.VbtError, match=f"clip 0: row capacity {cap} exceeded by {total - cap}"):
        mc.rows(0)
    live = mc.live(flush_view=True)
    assert live[0].overflow & LIVE_ROWS_LOST and live[0].phases == []
    assert live[1].overflow == 0 and live[1].rows == len(other.rows["id"])
    mc.finish(0.45)
    ovf = mc.summary()[3]
    assert ovf[0] != 0 and ovf[1] == 0


# ---- 7. a count above 25 ----

def test_a_count_above_25_is_clamped():
    """counts = 30 where a frame holds 25 detections: the step sees the 25 there are (one-frame kernel: clamped on the host; the
    multi-frame kernel, one and two clips: min(n, 25) on the device)"""
    frames, tm = cc.scene("A")
    frames, tm = frames[:14], tm[:14]
    rep = cc.replay_ocsort_on(frames, tm, max_age=30, iou_threshold=0.1, asso_func="diou")
    dets, counts, times = cc.pack([(frames, tm)])
    assert (counts == 25).sum() >= 10
    counts[counts == 25] = 30
    one, many, two = _tracker("diou", 1, 1024, 30), _tracker("diou", 1, 1024, 30), _tracker("diou", 2, 1024, 30)
    for f in range(len(frames)):
        one.update_frames(dets[f:f + 1], counts[f:f + 1], times[f:f + 1])
    many.update_frames(dets, counts, times)
    two.update_frames(np.repeat(dets, 2, axis=1), np.repeat(counts, 2, axis=1), np.repeat(times, 2, axis=1))
    for what, mc, ci in (("one frame per call", one, 0), ("all frames", many, 0), ("two clips", two, 0), ("two clips", two, 1)):
        _assert_rows(mc.rows(ci), rep.rows, what)
        _assert_state(mc, ci, rep, what)


# ---- 8. a track whose predicted box is NaN ----

def test_zero_height_detection_is_born_and_removed_by_ocsort():
    """tests/test_gpu_sort.py's scene under OC-SORT: s = w * h = 0 at the birth, so the predicted box of the next frame is NaN (h = s / w
    = 0 / 0) and the track leaves the list in the predict phase, twice in ten frames.  Host detections in one launch, and the
    time-batched walk as one run with the state in LDS, where a slot is freed mid-walk and the write-back has to skip it."""
    from test_gpu_sort import zero_height_scene
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer
    frames, tm = zero_height_scene()
    assert len(frames) == 10 and all(list(frames[f][1]) == [0.4, 0.5, 0.5, 0.5, 0.8, 0.0] for f in (1, 5))
    boxes, scores, counts, dets32 = cc.as_detector_output(frames)
    reps = {}
    for what, fr in (("host", frames), ("walk", dets32)):        # the walk's oracle: on the float64 detections the tracker makes of float32
        with np.errstate(invalid="ignore"):
            rep = reps[what] = cc.replay_ocsort_on(fr, tm, max_age=30, asso_func="diou", iou_threshold=0.1)
        assert len(rep.rows["id"]) == 21 and set(rep.rows["id"]) == {1, 2, 3} and not np.isnan(rep.rows["x"]).any(), what
        assert [(len(s.before), len(s.ids)) for s in rep.steps][2::4] == [(3, 2), (3, 2)], what     # the list after frames 3 and 7
        assert [(i, gone) for i, _, gone in cc.deaths(rep)] == [(2, [2]), (6, [2])], what                    # two removals, none by age
    host = _tracker("diou", 1, 512, 30)
    host.update_frames(*cc.pack([(frames, tm)]))
    walk = _tracker("diou", 1, 512, 30)
    b, s, c = (DeviceBuffer.from_host(np.ascontiguousarray(x)) for x in (boxes, scores, counts))
    run = (_lib.Run * 1)(_lib.Run(0, 0, 1, len(frames), 1, 1, 30.0))         # 10 frames: above the 6 from which a run keeps the state in LDS
    _lib.check(_lib.lib().vbt_tracker_update_from_detections_seq(walk.handle, b.ptr, s.ptr, c.ptr, len(frames), run, 1, 0.25, None))
    for what, mc in (("host", host), ("walk", walk)):
        rep = reps[what]
        _assert_rows(mc.rows(0), rep.rows, what)
        _assert_state(mc, 0, rep, what)
        assert mc.status(0)["trackers"] == 2, what
        mc.finish(0.45)
        assert mc.phases(0)[0] == cc.export_rule(rep.rows)[0] == 1, what
