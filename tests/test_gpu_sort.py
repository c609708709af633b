"""The SORT tracker on the device (vbt_tracker_create_sort, vbt_amd/csrc/sort_step.h + step_phases.h) against the numpy restatement
(tests/sort_ref.py) bit for bit, and against the reference's committed SORT frames (tests/golden/dfs_sort.npz) in the terms of
tests/test_sort_ref_host.py; then every path that steps it (host detections, the one-frame kernel, the fused per-frame kernel, the
time-batched walk with its two state homes), the pipeline and the CLI.  Inputs and reference replays: tests/sort_cases.py."""
import ctypes
import os

import numpy as np
import pytest

import sort_cases as sc
import sort_ref

pytestmark = pytest.mark.gpu
COLS = sc.COLS


def _rows(mc, clip=0):
    return {k: np.asarray(v) for k, v in mc.rows(clip).items()}


def _assert_rows_equal(got, want, what):
    assert np.array_equal(got["id"], np.asarray(want["id"])), what
    for k in COLS:
        assert np.array_equal(got[k], np.asarray(want[k], np.float64), equal_nan=True), (what, k)


def _ref(frames, times, **kw):
    rows, stats = sort_ref.track_boxes(frames, times, **kw)
    return rows, stats


def _scene(seed, n):
    """the first n frames of a random scene"""
    frames, tm = sc.random_scene(seed)
    return frames[:n], tm[:n]


def _run_host(frames, times, n_clips=1, clip=0, rows_cap=4096, **kw):
    """the scene through vbt_tracker_update (host detections, all frames in one launch) in `clip` of an n_clips tracker"""
    from vbt_amd.sort import MultiClipSortTracker
    mc = MultiClipSortTracker(n_clips, rows_cap, **kw)
    empty = ([f[:0] for f in frames], times)
    mc.update_frames(*sc.pack([frames if c == clip else empty[0] for c in range(n_clips)], [times] * n_clips))
    return mc


# ---- 1. the reference's clips ----

def test_reference_clips_in_one_launch():
    """The 12 fully matching clips, one wavefront per clip, longest 3 243 frames: the whole row log equals the numpy reference bit
    for bit, ids included, and the reference's dfs/ frames under the CPU test's terms."""
    from vbt_amd.sort import MultiClipSortTracker
    data = [sc.clip_detections(c) for c in sc.FULL_CLIPS]
    assert max(len(d[0]) for d in data) == 3243
    mc = MultiClipSortTracker(len(data), 8192, max_age=30)
    mc.update_frames(*sc.pack([d[0] for d in data], [d[1] for d in data]))
    rows = 0
    for ci, clip in enumerate(sc.FULL_CLIPS):
        st = mc.status(ci)
        assert st["overflow"] == 0 and st["rows_overflow"] == 0, clip
        got = _rows(mc, ci)
        _assert_rows_equal(got, sc.clip_replay(clip)[0], clip)
        rows += sc.check_against_dfs(clip, got)
    assert rows >= 19000
    mc.finish(0.45)                                     # the clip close works on a SORT log: the export id is the file's, less the offset
    for ci, clip in enumerate(sc.FULL_CLIPS):
        _, offset, export_id = sc.fixture()[clip]
        assert mc.phases(ci)[0] == export_id - offset, clip


# ---- 2. random scenes ----

@pytest.mark.parametrize("thr", sc.SCENE_THRESHOLDS)
def test_random_scenes_equal_numpy_reference(thr):
    from vbt_amd.sort import MultiClipSortTracker
    scenes, reps = sc.scenes(), sc.scene_replays(thr)
    assert len(scenes) == 24 and all(len(f) == 160 for f, _ in scenes)
    # conditions on the scenes, through the reference's counters
    assert sum(len(r["id"]) for r, _ in reps) > 5000
    assert sum(s["assignment_frames"] for _, s in reps) >= 50
    assert all(s["deaths"] >= 1 and s["late_births"] >= 1 for _, s in reps)
    mc = MultiClipSortTracker(len(scenes), 4096, max_age=sc.SCENE_MAX_AGE, iou_threshold=thr)
    mc.update_frames(*sc.pack([s[0] for s in scenes], [s[1] for s in scenes]))
    for ci, (want, _) in enumerate(reps):
        assert mc.status(ci)["overflow"] == 0
        _assert_rows_equal(_rows(mc, ci), want, (thr, ci))


# ---- 3. edges ----

def _box(cx, cy, w=0.06, h=0.06, score=0.9):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, score, 0.0]


def _times(n):
    return (np.arange(n) + 1) / 30.0


def zero_height_scene():
    """two plates moving slowly; in frame 2 (emitted whatever its hits) and in frame 6 (hidden) a detection of zero height between them"""
    frames = []
    for f in range(10):
        d = [_box(0.2 + 0.004 * f, 0.3), _box(0.7, 0.6 - 0.003 * f, 0.1, 0.08)]
        if f in (1, 5):
            d.insert(1, [0.4, 0.5, 0.5, 0.5, 0.8, 0.0])
        frames.append(np.asarray(d))
    return frames, _times(10)


def test_zero_height_detection_is_born_and_removed():
    frames, tm = zero_height_scene()
    want, stats = _ref(frames, tm, max_age=30)
    assert stats["nan_removals"] == 2 and np.isnan(np.asarray(want["x"])).sum() == 1          # frame 2's birth row is the NaN box
    mc = _run_host(frames, tm, max_age=30)
    got = _rows(mc)
    _assert_rows_equal(got, want, "zero height")
    assert mc.status()["trackers"] == 2 and [k.id for k in mc.trackers()] == [0, 1]           # the neighbours are all that is left
    clean, _ = _ref([f[f[:, 3] > f[:, 1]] for f in frames], tm, max_age=30)                   # ... and they never noticed
    for tid in (1, 2):
        m, c = got["id"] == tid, np.asarray(clean["id"]) == tid
        for k in COLS:
            assert np.array_equal(got[k][m], np.asarray(clean[k])[c]), (tid, k)


def grid_boxes(cells):
    """one 0.06 box in each listed cell of a 9 x 9 grid of the unit square: no two overlap"""
    return np.asarray([_box(0.1 * (c % 9) + 0.1, 0.1 * (c // 9) + 0.1) for c in cells])


def test_25_births_at_once():
    frames, tm = [grid_boxes(range(25))] * 4, _times(4)
    want, stats = _ref(frames, tm, max_age=30)
    assert len(want["id"]) == 100 and sorted(want["id"][:25]) == list(range(1, 26))
    mc = _run_host(frames, tm, max_age=30)
    _assert_rows_equal(_rows(mc), want, "25 births")
    assert mc.status()["trackers"] == 25


def test_65th_track_sets_the_overflow_flag_and_writes_nothing():
    """25 + 25 + 25 detections in disjoint places: 64 tracks live, 11 births counted in `overflow` and not stored (as on the OC-SORT
    path); the clip next to it in memory is untouched and the read-backs report the capacity error."""
    from vbt_amd import _lib
    from vbt_amd.sort import MultiClipSortTracker
    frames = [grid_boxes(range(25 * f, 25 * f + 25)) for f in range(3)]
    other, otm = _scene(5, 40)
    want_other, _ = _ref(other, otm, max_age=30)
    mc = MultiClipSortTracker(2, 4096, max_age=30)
    mc.update_frames(*sc.pack([frames + [f[:0] for f in other[3:]], other], [otm, otm]))
    st = mc.status(0)
    assert st["trackers"] == 64 and st["overflow"] == 11 and st["frame_count"] == 3
    assert [k.id for k in mc.trackers(0)] == list(range(64))
    with pytest.raises(_lib.VbtError, match="more than 64 live tracks"):
        mc.rows(0)
    assert mc.status(1)["overflow"] == 0
    _assert_rows_equal(_rows(mc, 1), want_other, "neighbour clip")


def leaving_scene(n=40, last=5):
    """plate A in every frame; plate B in frames 1..last only"""
    return [np.asarray([_box(0.3, 0.3 + 0.002 * f)] + ([_box(0.7, 0.7)] if f < last else [])) for f in range(n)], _times(n)


@pytest.mark.parametrize("max_age,dies_on", [(0, 6), (30, 36)])
def test_death_on_the_exact_frame(max_age, dies_on):
    """one frame per call (the one-frame kernel): the track list after every frame is the reference's; B dies when its misses exceed max_age"""
    from vbt_amd.sort import SortTracker
    frames, tm = leaving_scene()
    a, b = SortTracker(max_age=max_age), sort_ref.SortTracker(max_age=max_age)
    alive = []
    for d, t in zip(frames, tm):
        ra, rb = a.update(d, [], time=t), b.update(d, [])
        assert np.array_equal(ra, rb)
        ta, tb = a.trackers, b.trackers
        assert [k.id for k in ta] == [k.id for k in tb]
        for x, y in zip(ta, tb):
            assert np.array_equal(x.kf.x, y.kf.x)
        alive.append(len(ta))
    assert alive[dies_on - 2] == 2 and alive[dies_on - 1] == 1 and b.stats["deaths"] == 1


def test_min_hits_zero():
    frames, tm = _scene(7, 60)
    want, _ = _ref(frames, tm, max_age=5, min_hits=0)
    hidden, _ = _ref(frames, tm, max_age=5, min_hits=3)
    assert len(want["id"]) > len(hidden["id"])                     # every track is emitted from its birth frame on
    _assert_rows_equal(_rows(_run_host(frames, tm, max_age=5, min_hits=0)), want, "min_hits 0")


def shrinking_scene():
    """plate B shrinks fast and is then missed: its predicted area runs into the `s + vs <= 0` clamp while plate A keeps the frames coming"""
    sizes = [0.30, 0.24, 0.18, 0.12, 0.06, 0.02]
    frames = [np.asarray([_box(0.2, 0.2)] + ([_box(0.65, 0.65, sizes[f], sizes[f])] if f < len(sizes) else [])) for f in range(16)]
    return frames, _times(16)


def test_negative_area_velocity_is_clamped():
    frames, tm = shrinking_scene()
    want, stats = _ref(frames, tm, max_age=30, min_hits=0)
    assert stats["vs_clamps"] >= 1 and stats["nan_removals"] == 0
    mc = _run_host(frames, tm, max_age=30, min_hits=0)
    _assert_rows_equal(_rows(mc), want, "clamp")
    b = sort_ref.SortTracker(max_age=30, min_hits=0)
    for d in frames:
        b.update(d)
    for x, y in zip(mc.trackers(), b.trackers):                    # the clamped state itself, not only the rows it emitted before
        assert x.id == y.id and np.array_equal(x.kf.x, y.kf.x)


def test_empty_frame_is_not_stepped_and_id_base():
    frames, tm = _scene(11, 30)
    frames = [f if i not in (4, 9, 10) else f[:0] for i, f in enumerate(frames)]
    stepped = sum(len(f) > 0 for f in frames)
    want, _ = _ref(frames, tm, max_age=30, id_base=93)
    mc = _run_host(frames, tm, max_age=30, id_base=93)
    assert mc.status()["frame_count"] == stepped < 30                   # `count = 0`: frame_count does not move (track.py:180-181)
    got = _rows(mc)
    _assert_rows_equal(got, want, "id_base")
    assert got["id"].min() == 94 and mc.trackers()[0].id >= 93


# ---- 4. paths ----

def f32_scene(seed=29, n=47):
    """a random scene as the detector would write it: float32 boxes (ymin,xmin,ymax,xmax) and scores, and the float64 detections
    [x1,y1,x2,y2,score,cls] the tracker makes of them; a few frames carry no detection"""
    frames, tm = _scene(seed, n)
    boxes, scores, counts = np.zeros((n, 25, 4), np.float32), np.zeros((n, 25), np.float32), np.zeros(n, np.int32)
    dets = []
    for f, d in enumerate(frames):
        if f in (12, 13, 30):
            d = d[:0]
        counts[f] = len(d)
        boxes[f, :len(d)] = d[:, [1, 0, 3, 2]]
        scores[f, :len(d)] = d[:, 4]
        b, s = boxes[f, :len(d)].astype(np.float64), scores[f, :len(d)].astype(np.float64)
        dets.append(np.stack([b[:, 1], b[:, 0], b[:, 3], b[:, 2], s, np.zeros(len(d))], 1))
    return boxes, scores, counts, dets, tm


def test_every_path_gives_the_same_row_log():
    """vbt_tracker_update (host detections), the one-frame kernel (SortTracker.update), vbt_tracker_update_from_detections and the
    time-batched kernel with runs of 5 frames (state in global memory) and of 7 (state in LDS): five row logs, all equal, and equal to
    the numpy reference."""
    import torch
    from vbt_amd import _lib
    from vbt_amd.sort import MultiClipSortTracker, SortTracker
    L = _lib.lib()
    boxes, scores, counts, dets, tm = f32_scene()
    n = len(dets)
    kw = dict(max_age=8, iou_threshold=0.3)
    want, stats = _ref(dets, tm, **kw)
    assert stats["assignment_frames"] > 0 and stats["deaths"] > 0 and len(want["id"]) > 60
    logs = {"host": _rows(_run_host(dets, tm, **kw))}
    one = SortTracker(**kw)
    for d, t in zip(dets, tm):
        one.update(d, [], time=t)
    logs["one"] = _rows(one.multi)
    b, s, c = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(counts).cuda()
    fused = MultiClipSortTracker(1, 4096, **kw)
    for f in range(n):
        t = np.array([tm[f]], np.float64)
        _lib.check(L.vbt_tracker_update_from_detections(fused.handle, b[f].data_ptr(), s[f].data_ptr(), c[f:f + 1].data_ptr(), t.ctypes.data, 0.25, None))
    torch.cuda.synchronize()
    logs["fused"] = _rows(fused)
    for run in (5, 7):                                              # SEQ_LDS_MIN = 6 frames: below it the walk works on global memory
        seq = MultiClipSortTracker(1, 4096, **kw)
        for f0 in range(0, n, run):
            ra = (_lib.Run * 1)(_lib.Run(0, f0, 1, min(run, n - f0), f0 + 1, 1, 30.0))
            _lib.check(L.vbt_tracker_update_from_detections_seq(seq.handle, b.data_ptr(), s.data_ptr(), c.data_ptr(), n, ra, 1, 0.25, None))
        torch.cuda.synchronize()
        logs[f"seq{run}"] = _rows(seq)
        assert seq.status()["frame_count"] == int((counts > 0).sum())
    for name, got in logs.items():
        _assert_rows_equal(got, want, name)


def test_reset_clips_restarts_one_clip_at_id_base():
    from vbt_amd.sort import MultiClipSortTracker
    frames, tm = _scene(2, 50)
    want, _ = _ref(frames, tm, max_age=30, id_base=7)
    mc = MultiClipSortTracker(2, 2048, max_age=30, id_base=7)
    both = sc.pack([frames, frames], [tm, tm])
    mc.update_frames(*both)
    before = mc.rows(1)
    mc.reset_clips([0])
    assert mc.status(0)["rows"] == 0 and mc.status(0)["frame_count"] == 0 and mc.rows(1) == before
    mc.update_frames(*sc.pack([frames, [f[:0] for f in frames]], [tm, tm]))
    got = _rows(mc, 0)
    _assert_rows_equal(got, want, "after reset_clips")
    assert got["id"].min() == 8 and mc.rows(1) == before
    mc.reset()
    assert mc.status(1)["rows"] == 0
    mc.update_frames(*both)
    _assert_rows_equal(_rows(mc, 1), want, "after reset")


# ---- 5. pipeline and CLI ----

T_CLIP, THR = 14, 0.45         # at 0.45 the synthetic detector leaves 1..8 boxes per frame: about 40 SORT tracks, one with 8 rows


def _clip():
    from vbt_amd import synth
    return synth.clip_frames(12, 0, T_CLIP)


def _replayed(steps, fps, thr):
    """the detector's read-back outputs of every step, thresholded and reordered as the fused path does (odt.py:70-75,102-118)"""
    dets = []
    for b, s, cnt in steps:
        keep = [i for i in range(int(cnt)) if s[i] >= np.float32(thr)]
        dets.append(np.asarray([[b[i, 1], b[i, 0], b[i, 3], b[i, 2], s[i], 0.0] for i in keep], np.float64).reshape(-1, 6))
    return dets, [(t + 1) / fps for t in range(len(steps))]


def test_pipeline_sort_rows_equal_the_replayed_detections(model_path):
    import torch
    from vbt_amd import _lib
    from vbt_amd.sort import sort_params
    from vbt_amd.track import Pipeline
    fd = torch.from_numpy(_clip()).cuda()
    pipe = Pipeline(model_path, 1, max_frames=T_CLIP, fps=60.0, detection_treshold=THR, rows_per_frame=25, tracker="sort")
    steps = []
    for t in range(T_CLIP):
        pipe.step(fd[t:t + 1])
        b, s, _, cnt = pipe.detections()
        steps.append((b[0].copy(), s[0].copy(), cnt[0]))
    p = sort_params(max_age=30)
    assert _lib.lib().vbt_pipeline_use_sort(pipe._h, ctypes.byref(p)) == -5          # VBT_ERR_STATE: steps were enqueued
    pipe.finish()
    got = {k: np.asarray(v) for k, v in pipe.rows(0).items()}
    dets, tm = _replayed(steps, 60.0, THR)
    assert len(got["id"]) > 0
    _assert_rows_equal(got, _rows(_run_host(dets, np.asarray(tm), max_age=30)), "pipeline vs host path")
    _assert_rows_equal(got, _ref(dets, tm, max_age=30)[0], "pipeline vs numpy reference")
    pipe.reset()
    assert _lib.lib().vbt_pipeline_use_sort(pipe._h, ctypes.byref(p)) == -5          # ... and a reset does not reopen the choice


def test_pipeline_sort_live_leader_is_the_clip_close(model_path):
    """live analysis on a SORT pipeline: after the last batch the leader and its flush view are the close's export id and phases"""
    from vbt_amd.track import Pipeline
    frames = _clip()
    pipe = Pipeline(model_path, 8, max_frames=T_CLIP, fps=60.0, detection_treshold=THR, rows_per_frame=25, tracker_clips=1, tracker="sort")
    pipe.enable_live()
    for t0 in range(0, T_CLIP, 8):
        nf = min(8, T_CLIP - t0)
        pipe.step_runs(np.ascontiguousarray(frames[t0:t0 + nf]), [(0, 0, nf, t0 + 1)])
    live = pipe.live(flush_view=True)[0]
    best, rows, nph, ovf, ph = pipe.close(cap=32)
    assert live.overflow == 0 and ovf[0] == 0 and live.leader == best[0] >= 1 and live.rows == rows[0]
    assert [(p.time_start, p.time_end, p.y_start, p.y_end, p.rom, p.type) for p in live.phases] == [tuple(r[:5]) + (int(r[5]),) for r in ph[0, :nph[0]]]


def test_cli_tracker_flag(tmp_path, model_path):
    """`cli track --tracker sort` writes {video}_id{N}_{model}.pkl.gz with the rows of track_frames(tracker="sort"); its phases come out
    of the clip close on the device and equal the CPU analysis of the exported id; without the flag the rows are today's OC-SORT rows."""
    import pandas as pd
    from click.testing import CliRunner
    from oracle import velocity as ov
    from vbt_amd.cli import main
    from vbt_amd.track import COLUMNS, Pipeline, track_frames
    frames = _clip()
    src = tmp_path / "sort_clip.npy"
    np.save(str(src), frames)
    common = ["track", str(src), "--model", model_path, "--fps", "60", "--detection_treshold", str(THR), "--time_batch", "8"]
    dfs = {}
    for name, extra in (("sort", ["--tracker", "sort"]), ("ocsort", [])):
        out = tmp_path / name
        res = CliRunner().invoke(main, common + ["--df_dir", str(out)] + extra)
        assert res.exit_code == 0, res.output
        files = os.listdir(out)
        assert len(files) == 1 and files[0].startswith("sort_clip_id") and files[0].endswith("_efficientdet_lite0_synth.pkl.gz")
        dfs[name] = (files[0], pd.read_pickle(os.path.join(out, files[0])))
        want = track_frames(frames, model_path, fps=60.0, detection_treshold=THR, time_batch=8, **({"tracker": "sort"} if extra else {}))
        wdf = pd.DataFrame.from_dict(want).sort_values(by=["id", "time"])
        assert len(wdf) == len(dfs[name][1]) > 0
        for c in COLUMNS:
            assert np.array_equal(dfs[name][1][c].to_numpy(), wdf[c].to_numpy()), (name, c)
    a, b = dfs["sort"][1], dfs["ocsort"][1]
    assert not (len(a) == len(b) and np.array_equal(a["x"].to_numpy(), b["x"].to_numpy()))      # posterior boxes, not the observations
    # phases of the SORT clip: vbt_tracker_finish on the device against the CPU analysis of the exported id's rows
    pipe = Pipeline(model_path, 8, max_frames=T_CLIP, fps=60.0, detection_treshold=THR, rows_per_frame=25, tracker_clips=1, tracker="sort")
    for t0 in range(0, T_CLIP, 8):
        nf = min(8, T_CLIP - t0)
        pipe.step_runs(np.ascontiguousarray(frames[t0:t0 + nf]), [(0, 0, nf, t0 + 1)])
    best, _, nph, _, ph = pipe.close(cap=32)
    assert f"_id{best[0]}_" in dfs["sort"][0]
    sel = a[a["id"] == best[0]]
    want_ph = ov.analyze_track(*[sel[c].tolist() for c in COLUMNS[1:]], plate_diameter=0.45)
    assert nph[0] == len(want_ph)
    for r, w in zip(ph[0, :nph[0]], want_ph):
        assert list(r) == w.as_row()
    # the flag goes through --live, --concurrent and the one-pass export, which all read the row log
    res = CliRunner().invoke(main, common + ["--tracker", "sort", "--live"])
    assert res.exit_code == 0 and f"{len(a)} rows" in res.output, res.output
    res = CliRunner().invoke(main, ["track", str(src), str(src)] + common[2:] + ["--tracker", "sort", "--concurrent", "2"])
    assert res.exit_code == 0 and res.output.count(f"{len(a)} rows") == 2, res.output
    res = CliRunner().invoke(main, common + ["--tracker", "sort", "--video_dir", str(tmp_path / "vid"), "--one_pass", "--live_hud", "--hud_scale", "1"])
    assert res.exit_code == 0 and f"{len(a)} rows" in res.output and os.path.exists(tmp_path / "vid" / "sort_clip.npy"), res.output
