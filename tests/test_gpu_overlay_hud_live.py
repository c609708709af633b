"""Rep panel that follows the live rep analysis, on the GPU (include/vbt_hip.h, "Rep panel from the live analysis"): after
hud_follow_update a draw writes the bytes it writes after a live poll at the same point followed by set_hud with the polled phases - the
table, integer for integer, at every tracker launch of three reference clips, and the pixels, bit for bit against the numpy statement
of the panel (tests/overlay_hud_ref.py), wherever the polled list changed; the blank states; the pipeline's ordering; `track --live_hud`."""
import os

import numpy as np
import pytest
from click.testing import CliRunner

import overlay_hud_ref as HR
from test_gpu_overlay import assert_same, noise

pytestmark = pytest.mark.gpu

CLIPS = ("029", "013", "017")          # three ids and a leader that changes; one id and a phase the filter drops; the shortest clip
FPS = 30.0
FG, BG = (252, 3, 115), (10, 200, 30)
# pixel format, H, W, panel origin, scale
SHAPES = (("rgb24", 72, 64, (3, 5), 1), ("nv12", 72, 64, (4, 6), 1), ("i420", 72, 64, (4, 6), 1), ("rgb24", 112, 128, (3, 5), 2))
FLAGGED, BAD_PHASE, CAPACITY = 1, 2, 4
B, STEP = 3, 4


def frame_shape(fmt, H, W):
    return (H, W, 3) if fmt == "rgb24" else (H * 3 // 2, W)


@pytest.fixture(scope="module")
def replay():
    """(dets, counts, times, last real frame index per clip) of the three clips side by side - shared, read-only"""
    from test_gpu_tracker import _pack
    from test_oracle_ocsort import frames_from_rows
    from test_oracle_ocsort_corpus import load_all
    corpus = load_all()
    assert all(corpus[c][2] == FPS for c in CLIPS)
    data = [frames_from_rows(corpus[c][0]) for c in CLIPS]
    dets, counts, times = _pack([d[0] for d in data], [d[1] for d in data])
    for a in (dets, counts, times):
        a.setflags(write=False)
    return dets, counts, times, [len(d[0]) for d in data]


def tracker(phase_cap=128, n=len(CLIPS)):
    from vbt_amd.ocsort import MultiClipTracker
    mc = MultiClipTracker(n, 8192, max_age=30, asso_func="diou", iou_threshold=0.1)
    mc.enable_live(path_cap=4096, phase_cap=phase_cap)
    return mc


def follower(mc, clip, shape, **kw):
    from vbt_amd.overlay import Overlay
    fmt, H, W, (x, y), s = shape
    ov = Overlay(H, W, fmt, rgb=FG)
    ov.hud_follow(mc, clip, FPS, **dict(dict(x=x, y=y, scale=s, bg=BG), **kw))
    return ov


class Painter:
    """the reference panel over noise frames, its masks shared between the shapes of one scale"""

    def __init__(self):
        self.frames = {sh: noise((B,) + frame_shape(*sh[:3]), 40 + i) for i, sh in enumerate(SHAPES)}
        self.masks = {}

    def want(self, shape, tab, frame0):
        fmt, H, W, (x, y), s = shape
        out = self.frames[shape].copy()
        for i in range(B):
            key = (tab.tobytes(), frame0 + i * STEP, s)
            if key not in self.masks:
                self.masks[key] = HR.panel_mask(tab, frame0 + i * STEP, STEP, s, 200)
            out[i] = HR.paint_panel(out[i], self.masks[key], x, y, fmt, FG, BG)
        return out

    def got(self, ov, shape, frame0):
        from vbt_amd.mem import DeviceBuffer
        buf = DeviceBuffer.from_host(self.frames[shape])
        ov.draw(buf.ptr, B, frame0, STEP)
        return buf.to_host(self.frames[shape].shape, np.uint8)


@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_update_equals_poll_then_set_hud_on_reference_clips(replay, chunk):
    """Clips 029, 013 and 017 through one tracker, `chunk` frames per launch, a following handle per (clip, frame shape).  After every
    launch and update - flush view and plain view in turn - every handle's table is the table of a static handle given the polled
    phases; where a clip's polled seq changed (and at the first launch, a late one and after the last frame) three frames drawn by
    every handle of the clip equal the numpy panel of the polled phases, bit for bit."""
    from vbt_amd.overlay import Overlay
    dets, counts, times, last = replay
    F = counts.shape[0]
    mc = tracker()
    ovs = [[follower(mc, ci, sh) for sh in SHAPES] for ci in range(len(CLIPS))]
    static = [Overlay(72, 64, "rgb24") for _ in CLIPS]
    tables = [{} for _ in CLIPS]                                   # polled phases -> the static handle's table
    paint = Painter()
    launches = list(range(0, F, chunk)) + [F]                      # the last one: an update after the last frame, no new rows
    late = launches[(3 * len(launches)) // 4]
    seq = [None] * len(CLIPS)
    leaders, shrank, drawn = set(), 0, 0
    prev_len = [0] * len(CLIPS)
    for k, f0 in enumerate(launches):
        f1 = min(f0 + chunk, F)
        if f0 < F:
            mc.update_frames(dets[f0:f1], counts[f0:f1], times[f0:f1])
        flush = bool(k % 2)
        for row in ovs:
            for ov in row:
                ov.hud_follow_update(flush)
        recs = mc.live(flush_view=flush)
        for ci, rec in enumerate(recs):
            assert rec.overflow == 0
            ph = HR.phases6(rec.phases)
            key = ph.tobytes()
            if key not in tables[ci]:
                static[ci].set_hud(ph, FPS, x=3, y=5, scale=1)
                tables[ci][key] = static[ci].hud_table().copy()
                assert np.array_equal(tables[ci][key], HR.table(ph, FPS))      # the numpy statement: independent of the shared arithmetic
            want = tables[ci][key]
            assert len(want) == len(ph)
            for ov in ovs[ci]:
                assert np.array_equal(ov.hud_table(), want), (CLIPS[ci], f1, flush)
            assert ovs[ci][0].hud_follow_status() == (rec.leader, len(ph), 0), (CLIPS[ci], f1)
            if len(ph):
                leaders.add((ci, rec.leader))
            if not flush:                                          # (the flush view may hold one phase more: compare like with like)
                shrank += len(ph) < prev_len[ci]
                prev_len[ci] = len(ph)
            if rec.seq == seq[ci] and f0 not in (0, late, F):
                continue
            seq[ci] = rec.seq
            t_last = times[min(f1, last[ci]) - 1, ci]              # the clip's last time stamp of the chunk (its own last one past its end)
            frame0 = max(int(np.rint(t_last * FPS)), 1)
            for ov, sh in zip(ovs[ci], SHAPES):
                assert_same(paint.got(ov, sh, frame0), paint.want(sh, want.astype(np.int64), frame0))
                drawn += 1
    assert len({ld for ci, ld in leaders if ci == 0}) >= 2         # clip 029: the panel changed hands with phases on it
    assert shrank >= 1                                             # the filter dropped a phase: a table got shorter
    assert drawn >= 3 * len(CLIPS) * len(SHAPES)


def blank(shape, frames, frame0=7):
    fmt, H, W, (x, y), s = shape
    out = frames.copy()
    for i in range(len(out)):
        m = HR.panel_mask(np.zeros((0, 6), np.int64), frame0 + i, 1, s, 200)
        out[i] = HR.paint_panel(out[i], m, x, y, fmt, FG, BG)
    assert HR.text_lines(np.zeros((0, 6), np.int64), frame0) == ["REP    0", "ROM     ", "ACV     "]
    return out


def draw_back(ov, frames, frame0=7, step=1):
    from vbt_amd.mem import DeviceBuffer
    buf = DeviceBuffer.from_host(frames)
    ov.draw(buf.ptr, len(frames), frame0, step)
    return buf.to_host(frames.shape, np.uint8)


def test_before_any_row_the_panel_is_blank_and_refusals_that_need_a_tracker():
    from vbt_amd import _lib
    from vbt_amd.ocsort import MultiClipTracker
    from vbt_amd.overlay import Overlay
    mc = tracker()
    for sh in SHAPES[:2]:
        frames = noise((2,) + frame_shape(*sh[:3]), 3)
        ov = follower(mc, 1, sh)
        assert ov.hud_follow_status() == (-1, 0, 0) and len(ov.hud_table()) == 0      # bound, never updated
        assert_same(draw_back(ov, frames), blank(sh, frames))
        ov.hud_follow_update()
        assert ov.hud_follow_status() == (-1, 0, 0) and len(ov.hud_table()) == 0      # updated before any row
        assert_same(draw_back(ov, frames), blank(sh, frames))
    ov = Overlay(72, 64, "nv12")
    L = _lib.lib()
    prm = _lib.OverlayHudParams()
    L.vbt_overlay_hud_default_params(prm)
    prm.x, prm.y, prm.scale = 4, 6, 1

    def follow(t=mc.handle, clip=0, **kw):
        p = _lib.OverlayHudParams.from_buffer_copy(prm)
        for k, v in kw.items():
            setattr(p, k, v)
        return L.vbt_overlay_hud_follow(ov._h, p, t, clip, FPS), L.vbt_last_error().decode()
    rc, msg = follow(t=None)
    assert rc == -1 and "tracker is NULL" in msg
    for clip in (-1, 3):
        rc, msg = follow(clip=clip)
        assert rc == -1 and "clip" in msg
    rc, msg = follow(x=5)
    assert rc == -1 and "even" in msg
    rc, msg = follow(x=14)
    assert rc == -1 and "inside" in msg
    plain = MultiClipTracker(1, 64)                                 # no live analysis
    rc, msg = follow(t=plain.handle)
    assert rc == -5 and "live analysis is not enabled" in msg
    with pytest.raises(_lib.VbtError, match="follows no live analysis"):
        ov.hud_follow_update()                                      # every refusal left the handle without a panel
    frames = noise((1, 108, 64), 5)
    assert_same(draw_back(ov, frames), frames)
    assert follow()[0] == 0


def test_phase_cap_one_is_flagged_and_blank(replay):
    dets, counts, times, last = replay
    mc = tracker(phase_cap=1)
    sh = SHAPES[0]
    ov = follower(mc, 2, sh)
    mc.update_frames(dets[:last[2]], counts[:last[2]], times[:last[2]])
    ov.hud_follow_update()
    rec = mc.live()[2]
    assert rec.overflow != 0 and rec.phases == []                   # the second phase of clip 017 did not fit
    leader, n, flags = ov.hud_follow_status()
    assert (leader, n, flags) == (rec.leader, 0, FLAGGED) and len(ov.hud_table()) == 0
    frames = noise((2,) + frame_shape(*sh[:3]), 8)
    assert_same(draw_back(ov, frames, frame0=600), blank(sh, frames, frame0=600))


def test_more_than_64_phases_carry_the_count_across_strides():
    """A plate that goes up and down every 1.5 s for 100 s: about 130 phases, so the kernel forms the table in three strides of 64 lanes
    and carries the running concentric count from one to the next - against the numpy table of the polled phases, half way (a
    partial second stride) and at the end."""
    T = 3000
    f = np.arange(1, T + 1, dtype=np.float64)
    y = 0.5 + 0.14 * np.sin(2 * np.pi * f / (1.5 * FPS))
    dets = np.zeros((T, 1, 25, 6))
    dets[:, 0, 0] = np.stack([np.full(T, 0.36), y - 0.08, np.full(T, 0.64), y + 0.08, np.full(T, 0.9), np.zeros(T)], 1)
    counts = np.ones((T, 1), np.int32)
    times = (f / FPS).reshape(T, 1)
    mc = tracker(phase_cap=256, n=1)
    sh = SHAPES[0]
    ov = follower(mc, 0, sh)
    seen = []
    for f0, f1, flush in ((0, 1700, False), (1700, T, True)):
        mc.update_frames(dets[f0:f1], counts[f0:f1], times[f0:f1])
        ov.hud_follow_update(flush)
        rec = mc.live(flush_view=flush)[0]
        assert rec.overflow == 0 and rec.leader >= 0
        want = HR.table(rec.phases, FPS)
        tab = ov.hud_table()
        assert np.array_equal(tab, want) and ov.hud_follow_status() == (rec.leader, len(want), 0)
        seen.append(len(want))
        frames = noise((2,) + frame_shape(*sh[:3]), 11)
        ref = frames.copy()
        for i in range(2):
            ref[i] = HR.paint_panel(ref[i], HR.panel_mask(want, f1 + i, 1, 1, 200), 3, 5, "rgb24", FG, BG)
        assert_same(draw_back(ov, frames, frame0=f1), ref)
    assert 64 < seen[0] < 128 < seen[1] and want[-1, 5] > 64


def test_reset_of_the_followed_clip_set_hud_and_the_bytes_outside_the_panel(replay):
    from vbt_amd import _lib
    from vbt_amd.overlay import Overlay
    from test_gpu_overlay import FPS as ROW_FPS, synthetic_rows
    dets, counts, times, last = replay
    mc = tracker()
    sh = SHAPES[0]
    ovs = [follower(mc, ci, sh) for ci in range(3)]
    n = last[2]
    mc.update_frames(dets[:n], counts[:n], times[:n])
    for ov in ovs:
        ov.hud_follow_update()
    before = [ov.hud_table().copy() for ov in ovs]
    assert all(len(t) > 0 for t in before)
    mc.reset_clips([1])
    for ov in ovs:
        ov.hud_follow_update()
    assert ovs[1].hud_follow_status() == (-1, 0, 0) and len(ovs[1].hud_table()) == 0
    frames = noise((2,) + frame_shape(*sh[:3]), 9)
    assert_same(draw_back(ovs[1], frames, frame0=500), blank(sh, frames, frame0=500))
    for ci in (0, 2):                                               # the other clips' panels are what they were
        assert np.array_equal(ovs[ci].hud_table(), before[ci])
        tab = before[ci].astype(np.int64)
        want = frames.copy()
        for i in range(2):
            want[i] = HR.paint_panel(want[i], HR.panel_mask(tab, 500 + i, 1, 1, 200), 3, 5, "rgb24", FG, BG)
        assert_same(draw_back(ovs[ci], frames, frame0=500), want)
    # set_hud on a following handle: back to a static table, and the follow calls say so
    ph = np.array([[1 / FPS, 11 / FPS, 0.4, 0.6, 0.5, 0.0]])
    ovs[0].set_hud(ph, FPS, x=3, y=5, scale=1, bg=BG)
    assert np.array_equal(ovs[0].hud_table(), HR.table(ph, FPS))
    with pytest.raises(_lib.VbtError, match="follows no live analysis"):
        ovs[0].hud_follow_update()
    mc.update_frames(dets[n:n + 40], counts[n:n + 40], times[n:n + 40])
    assert np.array_equal(ovs[0].hud_table(), HR.table(ph, FPS))     # later launches do not reach it
    ovs[0].set_hud(None)
    assert_same(draw_back(ovs[0], frames), frames)                   # and the switch-off switches it off
    # a handle with rows: the panel changes its rectangle and nothing else
    rows = synthetic_rows()
    H, W = 72, 104
    frames = noise((3, H, W, 3), 10)
    only_rows = Overlay(H, W, "rgb24", rgb=FG)
    only_rows.set_rows(rows, ROW_FPS)
    both = Overlay(H, W, "rgb24", rgb=FG)
    both.set_rows(rows, ROW_FPS)
    both.hud_follow(mc, 2, ROW_FPS, x=40, y=10, scale=1, bg=BG)
    both.hud_follow_update()
    a, b = draw_back(only_rows, frames, frame0=127), draw_back(both, frames, frame0=127)
    assert (a != frames).any()
    outside = np.ones((H, W), bool)
    outside[10:60, 40:92] = False
    assert_same(b[:, outside], a[:, outside])
    tab = both.hud_table().astype(np.int64)
    assert len(tab) > 0
    for i in range(3):
        want = HR.paint_panel(a[i], HR.panel_mask(tab, 127 + i, 1, 1, 200), 40, 10, "rgb24", FG, BG)
        assert_same(b[i], want)


# ---- pipeline and CLI ----

REP_FPS, REP_T = 7.5, 36


def rep_clip(S=416):
    """The synthetic clip sampled every 8th frame, 36 frames = 4.8 s at 7.5 frames/s.  On that trajectory oracle/velocity.py gives an
    eccentric phase by frame 20, drops it for the concentric rep that ends at 2.93 s (frame 22) and has a second eccentric phase by frame
    36: the polled list is not empty, changes from batch to batch and gets shorter once."""
    from vbt_amd import synth
    bg = synth.background(12, S)
    return np.stack([synth.render(bg, 8 * i) for i in range(REP_T)])


def _lists(recs):
    return [HR.phases6(r.phases).tobytes() for r in recs]


def _reference_frames(frames, model_path, batch, stride, hud_params, fps=60.0):
    """track_frames(one_pass=True, live=collector): its frames with the numpy panel of the collected polls on them, batch by batch -
    the last batch with the flush view, which the export loop asks for there; (rows, frames, the poll of every batch)"""
    from vbt_amd.track import track_frames
    polls = []
    out = np.zeros((len(frames) // stride,) + frames.shape[1:], np.uint8)
    data = track_frames(frames, model_path, fps=fps, detection_treshold=0.3, frame_stride=stride, time_batch=batch, video_out=out, one_pass=True,
                        live=lambda rec, final: polls.append((rec, final)))
    kept = len(out)
    starts = list(range(0, kept, batch))
    assert [f for _, f in polls] == [False] * len(starts) + [True]
    used = []
    for bi, i0 in enumerate(starts):
        rec = polls[-1][0] if bi == len(starts) - 1 else polls[bi][0]
        assert rec.overflow == 0
        used.append(rec)
        nb = min(batch, kept - i0)
        out[i0:i0 + nb] = HR.draw(out[i0:i0 + nb], None, fps, rec.phases, frame0=(i0 + 1) * stride, frame_step=stride, hud_params=hud_params)
    return data, out, used


def test_pipeline_overlay_draw_updates_the_panel_in_every_tracker_placement(model_path, monkeypatch):
    """One clip with reps in it (rep_clip), one frame per step, drawn in place four frames at a time through vbt_pipeline_overlay_draw
    by a handle whose panel follows the pipeline's tracker - the tracker inline, on its own stream and with deferred groups.  After
    every draw the handle's leader and phase count are those of a poll at that point - an update that never ran, or ran before the
    tracker launch, leaves others - and the frames are those of the row-only draw with the numpy panel of the polled phases on them,
    the same bytes in every placement.  The polled list is not empty and changes between the batches.  The last batch is drawn with
    the handle's flush setting on."""
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.overlay import Overlay
    from vbt_amd.track import Pipeline
    T, S = REP_T, 416
    frames = rep_clip(S)
    fb = frames[0].nbytes
    hp = dict(x=7, y=9, scale=1)
    outs = {}
    for mode in ("inline", "own", "defer"):
        monkeypatch.setenv("VBT_TRACKER_STREAM", "own" if mode == "own" else "inline")
        monkeypatch.setenv("VBT_TRACKER_DEFER", "1" if mode == "defer" else "0")
        bufs, polls = [], []
        for panel in (False, True):
            pipe = Pipeline(model_path, 1, max_frames=T, fps=REP_FPS, detection_treshold=0.3, rows_per_frame=25, depth=2 if mode == "own" else 3)
            assert pipe._trk_inline == (mode != "own") and (pipe._defer > 0) == (mode == "defer")
            pipe.enable_live(path_cap=256, phase_cap=16)
            buf = DeviceBuffer.from_host(frames)
            ov = Overlay(S, S)
            ov.follow(*pipe.tracker.rows_dev(0), max_frame=T, max_rows_per_frame=25, fps=REP_FPS)
            if panel:
                ov.hud_follow(pipe.tracker, 0, REP_FPS, **hp)
            for t in range(T):
                pipe.step(buf.ptr + t * fb, stream=0, src_hw=(S, S))
                if t % 4 == 3:
                    if panel and t == T - 1:
                        ov.hud_follow_flush(True)
                    pipe.overlay_draw(ov, buf.ptr + (t - 3) * fb, 4, t - 2, stream=0)
                    rec = pipe.live(flush_view=t == T - 1)[0]
                    assert rec.overflow == 0 and rec.leader >= 0
                    if panel:
                        assert ov.hud_follow_status(0) == (rec.leader, len(rec.phases), 0), (mode, t)
                        assert _lists([rec]) == _lists([polls[t // 4]])       # the run without the panel saw the same analysis
                    else:
                        polls.append(rec)
            assert ov.follow_status(0)[1] == 0
            pipe.finish()
            assert len(pipe.rows(0)["id"]) > 0
            bufs.append(buf.to_host(frames.shape, np.uint8))
        lists = _lists(polls)
        assert len(polls) == T // 4 and any(len(r.phases) for r in polls[:-1]) and len(set(lists)) >= 3, [len(r.phases) for r in polls]
        assert max(HR.table(r.phases, REP_FPS)[:, 5].max(initial=0) for r in polls) >= 1      # a completed rep: the count leaves 0
        want = bufs[0].copy()
        for k, rec in enumerate(polls):
            want[4 * k:4 * k + 4] = HR.draw(want[4 * k:4 * k + 4], None, REP_FPS, rec.phases, frame0=4 * k + 1, hud_params=hp)
        unset = HR.draw(bufs[0][-4:], None, REP_FPS, [], frame0=T - 3, hud_params=hp)
        assert (bufs[0] != frames).any() and (want[-4:] != unset).any()          # the last panel is not the one a handle never updated draws
        assert_same(bufs[1], want)
        outs[mode] = bufs[1]
    assert_same(outs["own"], outs["inline"])
    assert_same(outs["defer"], outs["inline"])


def _track(tmp_path, src, model_path, tag, extra, fps="60"):
    from vbt_amd.cli import main
    out, dfs = tmp_path / ("out" + tag), tmp_path / ("dfs" + tag)
    res = CliRunner().invoke(main, ["track", str(src), "--model", model_path, "--df_dir", str(dfs), "--detection_treshold", "0.3", "--video_dir", str(out),
                                    "--one_pass", "--fps", fps] + extra)
    assert res.exit_code == 0, res.output
    files = os.listdir(dfs)
    assert len(files) == 1, res.output
    return out, dfs / files[0], res.output.replace(str(dfs), "DFS")


@pytest.mark.parametrize("case", ["raw", "mjpeg", "raw-batch5", "reps-batch5"])
def test_track_live_hud_draws_the_polled_panel_and_changes_nothing_else(tmp_path, model_path, case):
    """`track --one_pass --live_hud` against the same command without it, on the 12-frame clip of
    test_track_one_pass_writes_the_same_files (too short for a phase: the blank panel) and, reps-batch5, on rep_clip in batches of 5 -
    eight batches, the last one of one frame - where the panel carries phases that change from batch to batch and the last batch
    shows the flush view."""
    import pandas as pd
    from vbt_amd import synth
    reps = case == "reps-batch5"
    frames = rep_clip() if reps else synth.clip_frames(12, 0, 12, size=416)
    fps = REP_FPS if reps else 60.0
    src = tmp_path / "demo.npy"
    np.save(str(src), frames)
    batch = 5 if case.endswith("batch5") else 64                   # 5: several batches, the last one short
    extra = ["--time_batch", str(batch)] + (["--video_format", "mjpeg"] if case == "mjpeg" else [])
    hud = ["--live_hud", "--hud_scale", "2", "--hud_pos", "7,9"]
    plain, df0, line0 = _track(tmp_path, src, model_path, "0", extra, repr(fps))
    live, df1, line1 = _track(tmp_path, src, model_path, "1", extra + hud, repr(fps))
    assert df1.name == df0.name and line1 == line0
    a, b = pd.read_pickle(str(df1)), pd.read_pickle(str(df0))
    assert len(a) > 0 and a.equals(b)
    if case == "mjpeg":
        got, base = (live / "demo.avi").read_bytes(), (plain / "demo.avi").read_bytes()
        assert got[:4] == b"RIFF" and got != base                  # the panel is in the encoded frames
        return
    got, base = np.load(str(live / "demo.npy")), np.load(str(plain / "demo.npy"))
    data, want, used = _reference_frames(frames, model_path, batch, 1, dict(x=7, y=9, scale=2), fps)
    assert len(data["id"]) == len(a)
    if reps:                                                       # panels a handle that is never updated, or updated late, does not draw
        assert any(len(r.phases) for r in used[:-1]) and len(set(_lists(used))) >= 3, [len(r.phases) for r in used]
        assert max(HR.table(r.phases, fps)[:, 5].max(initial=0) for r in used) >= 1
    assert_same(got, want)
    outside = np.ones(frames.shape[1:3], bool)
    outside[9:9 + 100, 7:7 + 104] = False
    assert_same(got[:, outside], base[:, outside])                 # rows, ids and bar paths as without the panel
    assert (got[:, ~outside] != base[:, ~outside]).any()
