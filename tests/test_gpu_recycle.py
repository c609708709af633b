"""Slot close and reopen on the device (vbt_tracker_reset_clips, vbt_pipeline_close_clips / _closed_clip): a clip closed in its slot
gives what vbt_pipeline_close gives for it, bit for bit; the clip that reopens in the slot gives what it gives tracked alone in a fresh
one-clip pipeline; the other slots never notice - on all three tracker-launch paths (own stream, inline, depth 1) and with plain,
deferred, `active` and run steps."""
import ctypes
import os

import numpy as np
import pytest

from conftest import MODEL_LITE0

pytestmark = pytest.mark.gpu
COLS = ["time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width"]
ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -4, -5


def _rows_equal(got, want, what):
    assert got["id"] == want["id"], what
    for k in COLS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)


def _phase_rows(phases):
    return np.asarray([[p.time_start, p.time_end, p.y_start, p.y_end, p.rom, float(p.type)] for p in phases], np.float64).reshape(-1, 6)


_ALONE = {}


def _alone(key, frames, fps):
    """The clip tracked alone: vbt_track_clip on a fresh one-clip pipeline, then vbt_pipeline_close -> (rows, best_id, overflow, phases)."""
    if key not in _ALONE:
        from vbt_amd.track import Pipeline
        p = Pipeline(MODEL_LITE0, 16, max_frames=len(frames), fps=fps, rows_per_frame=25, tracker_clips=1)
        rows = p.track_clip(np.ascontiguousarray(frames))
        best, _, nph, ovf, ph = p.close(cap=512)
        _ALONE[key] = (rows, int(best[0]), int(ovf[0]), ph[0, :nph[0]].copy())
    return _ALONE[key]


def _check_alone(result, key, frames, fps):
    best, rows, phases, ovf = result
    want_rows, want_best, want_ovf, want_ph = _alone(key, frames, fps)
    _rows_equal(rows, want_rows, key)
    assert best == want_best and ovf == want_ovf, key
    assert np.array_equal(_phase_rows(phases), want_ph), key


# ---- 1. tracker level, against the oracle ----
def test_tracker_reset_clips_equals_oracle_and_leaves_other_clips_alone():
    from oracle import ocsort_np as oc
    from test_gpu_tracker import _pack, _random_scene
    from vbt_amd.ocsort import MultiClipTracker
    scenes = [_random_scene(s) for s in (3, 4, 5)]
    fresh = _random_scene(11)
    fresh = (fresh[0][:80], fresh[1][:80])         # a new scene for clip 1's last 80 frames, its times from 1 / fps
    dets, counts, times = _pack([s[0] for s in scenes], [s[1] for s in scenes])
    plain = MultiClipTracker(3, 4096, max_age=30, asso_func="diou", iou_threshold=0.1)
    plain.update_frames(dets, counts, times)
    mc = MultiClipTracker(3, 4096, max_age=30, asso_func="diou", iou_threshold=0.1)
    mc.update_frames(dets[:80], counts[:80], times[:80])
    mc.reset_clips([1])
    d2, c2, t2 = dets[80:].copy(), counts[80:].copy(), times[80:].copy()
    fd, fc, ft = _pack([fresh[0]], [fresh[1]])
    d2[:, 1], c2[:, 1], t2[:, 1] = fd[:, 0], fc[:, 0], ft[:, 0]
    mc.update_frames(d2, c2, t2)
    _rows_equal(mc.rows(1), oc.track_boxes(fresh[0], fresh[1]), "reset clip vs oracle")
    assert mc.rows(1)["id"] and min(mc.rows(1)["id"]) == 1
    for c in (0, 2):
        _rows_equal(mc.rows(c), plain.rows(c), f"clip {c}")
    with pytest.raises(ValueError):
        mc.reset_clips([3])
    with pytest.raises(ValueError):
        mc.reset_clips([0, 0])
    with pytest.raises(ValueError):
        mc.reset_clips([])


# ---- 2. pipeline equivalence over the three tracker-launch paths ----
LENGTHS = [250, 700, 260, 300, 250, 280, 320, 250, 270, 290]
FPS = [30.0, 60.0, 60.0, 30.0, 60.0, 30.0, 30.0, 60.0, 30.0, 60.0]


@pytest.fixture(scope="module")
def ten_clips():
    from vbt_amd import synth
    return [synth.clip_frames(40 + i, 13 * i, n) for i, n in enumerate(LENGTHS)]


def _stream(pipe, clips, fps, concurrent):
    """Drives `pipe` through shard.stream_schedule with close_clips / reopen; returns {clip: closed() result}."""
    from vbt_amd.shard import stream_schedule
    steps = stream_schedule([len(c) for c in clips], concurrent, pipe.n)
    nxt = {}                                          # (step, slot) of a close -> the clip that opens next in that slot
    for t, (_, _, closes) in enumerate(steps):
        for s in closes:
            nxt[(t, s)] = next((c for opens, _, _ in steps[t + 1:] for sl, c in opens if sl == s), None)
    out, clip_of, unread = {}, {}, {}
    for t, (opens, runs, closes) in enumerate(steps):
        for slot, c in opens:
            clip_of[slot] = c
            assert pipe.fps[slot] == fps[c]
        srcs = [clips[clip_of[s]][f0 - 1:f0 - 1 + n] for s, _, n, f0 in runs]
        pipe.step_runs(srcs, runs)
        for s in list(unread):
            r = pipe.closed(s, wait=False)
            if r is not None:
                out[unread.pop(s)] = r
        if closes:
            for s in closes:                          # (read before the slot closes again)
                if s in unread:
                    out[unread.pop(s)] = pipe.closed(s, wait=True)
            pipe.close_clips(closes, next_fps=[fps[nxt[(t, s)]] if nxt[(t, s)] is not None else fps[clip_of[s]] for s in closes])
            for s in closes:
                unread[s] = clip_of.pop(s)
    for s in list(unread):
        out[unread.pop(s)] = pipe.closed(s, wait=True)
    return out


@pytest.mark.parametrize("mode", ["own", "inline", "depth1"])
def test_pipeline_close_clips_equals_each_clip_alone(mode, ten_clips, monkeypatch):
    from vbt_amd.track import Pipeline
    if mode != "depth1":
        monkeypatch.setenv("VBT_TRACKER_STREAM", mode)
    pipe = Pipeline(MODEL_LITE0, 16, max_frames=max(LENGTHS), fps=FPS[:3], rows_per_frame=25, tracker_clips=3,
                    depth=1 if mode == "depth1" else None, slot_close=True)
    info = pipe.info()
    assert bool(info.tracker_inline) == (mode == "inline") and (info.depth == 1) == (mode == "depth1")
    out = _stream(pipe, ten_clips, FPS, 3)
    assert sorted(out) == list(range(len(ten_clips)))
    reps = 0
    for c, frames in enumerate(ten_clips):
        _check_alone(out[c], ("ten", c), frames, FPS[c])
        reps += len(out[c][2])
    assert reps > 0, "the clips contain reps"


# ---- 3 + 6. plain steps (deferred groups) and `active` steps; vbt_pipeline_close after recycling ----
@pytest.mark.parametrize("kind", ["plain", "active"])
def test_plain_and_active_steps_reopen_with_fresh_frame_numbers(kind):
    from vbt_amd import synth
    from vbt_amd.track import Pipeline
    T, cut = 40, 22                                   # 22 % 4 = 2: the close falls in the middle of a deferred group
    first = [synth.clip_frames(60 + c, 7 * c, T) for c in range(4)]
    second = synth.clip_frames(77, 5, T - cut)
    pipe = Pipeline(MODEL_LITE0, 4, max_frames=T, fps=60.0, rows_per_frame=25, slot_close=True)
    if kind == "plain":
        assert pipe.info().defer > 0, "the deferred group walk is on"
    act = np.ones(4, bool) if kind == "active" else None
    for t in range(T):
        if t == cut:
            pipe.close_clips([2], next_fps=30.0)
        batch = np.stack([second[t - cut] if (c == 2 and t >= cut) else first[c][t] for c in range(4)])
        pipe.step(batch, active=act)
    _check_alone(pipe.closed(2), ("first", 2, cut), first[2][:cut], 60.0)
    best, nrows, nph, ovf, ph = pipe.close(cap=512)       # vbt_pipeline_close after recycling: the clips open now
    for c in range(4):
        frames, fps = (second, 30.0) if c == 2 else (first[c], 60.0)
        want_rows, want_best, want_ovf, want_ph = _alone(("second",) if c == 2 else ("first", c, T), frames, fps)
        _rows_equal(pipe.rows(c), want_rows, (kind, c))
        assert (best[c], ovf[c], nrows[c]) == (want_best, want_ovf, len(want_rows["id"])), (kind, c)
        assert np.array_equal(ph[c, :nph[c]], want_ph), (kind, c)
    assert pipe.rows(2)["time"][0] == min(pipe.rows(2)["time"]) < 3 / 30.0    # the new clip's frame 1 is at 1 / fps


# ---- 4. live analysis restarts in a recycled slot ----
def test_live_record_restarts_in_a_recycled_slot():
    from vbt_amd import synth
    from vbt_amd.track import Pipeline
    a, b, c = synth.clip_frames(81, 0, 400), synth.clip_frames(82, 3, 40), synth.clip_frames(83, 9, 260)
    pipe = Pipeline(MODEL_LITE0, 16, max_frames=400, fps=60.0, rows_per_frame=25, tracker_clips=2, slot_close=True)
    pipe.enable_live()
    fa = 0

    def step(src1, run1):
        nonlocal fa
        pipe.step_runs([a[fa:fa + 8], src1], [(0, 0, 8, fa + 1), (1, 8) + run1])
        fa += 8

    for f0 in range(0, len(b), 8):
        step(b[f0:f0 + 8], (8, f0 + 1))
    flush_b = pipe.live(flush_view=True)[1]
    pipe.close_clips([1])
    got_b = pipe.closed(1)
    assert got_b[0] == flush_b.leader and np.array_equal(_phase_rows(got_b[2]), _phase_rows(flush_b.phases))
    _check_alone(got_b, ("live_b",), b, 60.0)
    rec = pipe.live()[1]
    assert (rec.rows, rec.leader) == (0, -1)
    # the new clip one frame at a time: rows_consumed counts its rows only; the leader stays -1 until an id has 2 rows
    seen_single = False
    for f in range(6):
        step(c[f:f + 1], (1, f + 1))
        rec, ids = pipe.live()[1], pipe.rows(1)["id"]
        two = any(ids.count(i) >= 2 for i in set(ids))
        assert rec.rows == len(ids) and (rec.leader >= 1) == two, f
        seen_single = seen_single or (len(ids) > 0 and not two)
    assert seen_single and rec.leader >= 1
    for f0 in range(6, len(c), 8):
        n = min(8, len(c) - f0)
        step(c[f0:f0 + n], (n, f0 + 1))
    flush = pipe.live(flush_view=True)
    pipe.close_clips([0, 1])
    for slot in (0, 1):
        best, _, phases, _ = got = pipe.closed(slot)
        assert best == flush[slot].leader and np.array_equal(_phase_rows(phases), _phase_rows(flush[slot].phases)), slot
        if slot == 1:
            assert len(phases) > 0, "the new clip contains reps"
            _check_alone(got, ("live_c",), c, 60.0)


# ---- 5. refusals ----
def test_refusals():
    from vbt_amd import _lib, synth
    from vbt_amd.track import Pipeline
    L = _lib.lib()
    pipe = Pipeline(MODEL_LITE0, 4, max_frames=16, fps=60.0, rows_per_frame=25)
    frames = [synth.clip_frames(90 + c, 0, 12) for c in range(4)]
    for t in range(12):
        pipe.step(np.stack([frames[c][t] for c in range(4)]))
    h = pipe._h

    def close(clips, fps=None):
        cl = np.asarray(clips, np.int32)
        nf = np.asarray(fps, np.float64) if fps is not None else None
        return L.vbt_pipeline_close_clips(h, cl.ctypes.data, len(cl), nf.ctypes.data if nf is not None else None)

    rec, ready = _lib.ClosedClip(), ctypes.c_int()
    ph = np.zeros((512, 6), np.float64)
    rows = np.zeros(1024, np.dtype([("id", "<i8")] + [(k, "<f8") for k in COLS]))

    def read(clip, cap_rows=len(rows), cap_phases=512):
        return L.vbt_pipeline_closed_clip(h, clip, 1, ctypes.byref(ready), ctypes.byref(rec), ph.ctypes.data, cap_phases, rows.ctypes.data, cap_rows)

    assert close([1]) == ERR_STATE                                       # not enabled: no close allocates
    assert L.vbt_pipeline_close_clips_enable(h) == 0 and L.vbt_pipeline_close_clips_enable(h) == 0
    assert close([4]) == ERR_ARG and close([-1]) == ERR_ARG
    assert close([1, 1]) == ERR_ARG
    assert close([1], [0.0]) == ERR_ARG and close([0, 1], [30.0, -1.0]) == ERR_ARG
    assert read(1) == ERR_STATE and read(4) == ERR_ARG                  # nothing pending / out of range
    assert close([1, 3], [30.0, 60.0]) == 0
    assert close([3]) == ERR_STATE                                       # slot 3's result is unread
    assert read(1, cap_rows=1) == ERR_CAPACITY and rec.n_rows > 1       # undersized: the result stays readable
    assert read(1) == 0 and ready.value == 1 and (rec.clip, rec.n_rows) == (1, rec.n_rows)
    want_rows, want_best, _, _ = _alone(("refusal", 1), frames[1], 60.0)
    assert rec.best_id == want_best and rows["id"][:rec.n_rows].tolist() == want_rows["id"]
    assert read(1) == ERR_STATE                                          # read once
    assert read(3) == 0 and close([3]) == 0 and read(3) == 0 and rec.n_rows == 0


# ---- 7. CLI ----
def test_cli_track_concurrent_matches_one_at_a_time(tmp_path, model_path):
    import pandas as pd
    from click.testing import CliRunner
    from vbt_amd import synth
    from vbt_amd.cli import main
    srcs = []
    for i, n in enumerate([90, 150, 60, 120, 80]):
        fr = synth.clip_frames(100 + i, 4 * i, n, size=320 if i % 2 == 0 else 400)
        if i % 2:
            fr = np.ascontiguousarray(fr[:, 80:320])                    # 240 x 400: resized on the device
        path = str(tmp_path / f"clip{i}.npy")
        np.save(path, fr)
        srcs.append(path)
    outs = {}
    for conc, d in ((3, "A"), (1, "B")):
        res = CliRunner().invoke(main, ["track", *srcs, "--model", model_path, "--df_dir", str(tmp_path / d), "--concurrent", str(conc)])
        assert res.exit_code == 0, res.output
        outs[d] = res.output.replace(str(tmp_path / d), "DIR")
    assert outs["A"] == outs["B"] and outs["A"].count("export id") == 5
    # a file that cannot be read: the files before it are tracked and printed, then its error - with either setting
    bad = str(tmp_path / "missing.npy")
    errs = {}
    for conc, d in ((3, "C"), (1, "D")):
        res = CliRunner().invoke(main, ["track", srcs[0], srcs[1], bad, srcs[2], "--model", model_path, "--df_dir", str(tmp_path / d),
                                        "--concurrent", str(conc)])
        assert isinstance(res.exception, FileNotFoundError), res.output
        errs[d] = res.output.replace(str(tmp_path / d), "DIR")
    assert errs["C"] == errs["D"] and errs["C"].count("export id") == 2
    files = sorted(os.listdir(tmp_path / "B"))
    assert sorted(os.listdir(tmp_path / "A")) == files and len(files) == 5
    for f in files:
        da, db = pd.read_pickle(str(tmp_path / "A" / f)), pd.read_pickle(str(tmp_path / "B" / f))
        assert da.equals(db) and da.index.equals(db.index), f
