"""Live rep analysis on the device (vbt_*_live_*): per-id phases that equal the reference VelocityTracker on the rows emitted so far,
bit for bit, at any point of a clip and whatever the tracker launches walked; the leader = the clip close's export rule so far; the
flush view after the last frame = the clip close.  Live analysis never changes what the tracker or the close compute."""
import os
import re

import numpy as np
import pytest

from conftest import MODEL_LITE0

pytestmark = pytest.mark.gpu
COLS = ["time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width"]


def _oracle_phases(rows, tid, flush=False):
    """oracle/velocity.py on the rows of `tid` so far: preprocess + VelocityTracker (end_processing() only with flush)."""
    from oracle import velocity as ov
    m = np.asarray(rows["id"]) == tid
    cols = ov.preprocess(*[np.asarray(rows[c])[m].tolist() for c in COLS])
    vt = ov.VelocityTracker(0.45)
    for i in range(len(cols[0])):
        vt.process_measurements(*[c[i] for c in cols])
    if flush:
        vt.end_processing()
    return np.asarray([p.as_row() for p in vt.phases], np.float64).reshape(-1, 6)


def _export_rule(rows):
    """reference track.py:107-115 on the rows so far (-1: no id with two rows yet)"""
    from vbt_amd.track import export_dataframe
    ids = np.asarray(rows["id"])
    if not any((ids == i).sum() >= 2 for i in set(ids.tolist())):
        return -1
    return export_dataframe(rows, "clip", "model", write=False)[1]


def _phase_rows(phases):
    return np.asarray([[p.time_start, p.time_end, p.y_start, p.y_end, p.rom, float(p.type)] for p in phases], np.float64).reshape(-1, 6)


@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_corpus_prefix_exact(chunk):
    """All 34 reference clips replayed through the tracker `chunk` frames per launch: at several points of every clip each analysed id's
    phases equal the oracle's on that id's rows so far, the analysed ids include every id that can still win, and the leader is the
    export rule on the rows so far; after the last frame the flush view is the clip close, exactly."""
    from test_gpu_tracker import _pack
    from test_oracle_ocsort import frames_from_rows
    from test_oracle_ocsort_corpus import load_all
    from vbt_amd.ocsort import MultiClipTracker
    corpus = load_all()
    clips = sorted(corpus)
    data = [frames_from_rows(corpus[c][0]) for c in clips]
    dets, counts, times = _pack([d[0] for d in data], [d[1] for d in data])
    F = counts.shape[0]
    mc = MultiClipTracker(len(clips), 8192, max_age=30, asso_func="diou", iou_threshold=0.1)
    mc.enable_live(path_cap=4096, phase_cap=128)
    checks = sorted({((F * q) // 4 // chunk) * chunk for q in (1, 2, 3)} - {0})
    checked = 0
    for f0 in range(0, F, chunk):
        f1 = min(f0 + chunk, F)
        mc.update_frames(dets[f0:f1], counts[f0:f1], times[f0:f1])
        if f1 not in checks:
            continue
        recs = mc.live()
        for ci, clip in enumerate(clips):
            rows = mc.rows(ci)
            tracks = mc.live_tracks(ci)
            assert recs[ci].overflow == 0 and recs[ci].rows == len(rows["id"])
            lead = _export_rule(rows)
            assert recs[ci].leader == lead, (clip, f1)
            if lead >= 0:
                assert lead in tracks
                assert np.array_equal(_phase_rows(recs[ci].phases), tracks[lead].phases)
            live_ids = {k.id + 1 for k in mc.trackers(ci)} & set(rows["id"])
            assert live_ids <= set(tracks), (clip, f1)
            for tid, tr in tracks.items():
                assert tr.flags == 0 and tr.rows == rows["id"].count(tid)
                want = _oracle_phases(rows, tid)
                assert np.array_equal(tr.phases, want), (clip, f1, tid)
                checked += len(want)
    assert checked > 50
    final = mc.live(flush_view=True)
    mc.finish(0.45)
    for ci, clip in enumerate(clips):
        best, ph = mc.phases(ci)
        assert best == corpus[clip][1] and final[ci].leader == best, clip
        assert np.array_equal(_phase_rows(final[ci].phases), ph), clip
        rows = mc.rows(ci)
        assert np.array_equal(mc.live_tracks(ci, flush_view=True)[best].phases, _oracle_phases(rows, best, flush=True)), clip


def _frames(n, T, seed=70):
    from vbt_amd import synth
    return np.stack([np.stack([synth.render(synth.background(seed + c), 7 * c + t) for c in range(n)]) for t in range(T)])


def _run(mode, fd, live, n, T, monkeypatch, polls=(), pipe=None):
    """The clips through one of the step paths; returns (close outputs + rows, final flush view, mid-run polls, the pipeline)."""
    import torch
    from vbt_amd.track import Pipeline
    st = torch.cuda.current_stream().cuda_stream
    if pipe is None:
        monkeypatch.setenv("VBT_TRACKER_STREAM", "inline" if mode in ("inline", "defer") else "own")
        monkeypatch.setenv("VBT_TRACKER_DEFER", "1" if mode == "defer" else "0")
        if mode == "runs":
            pipe = Pipeline(MODEL_LITE0, 64, max_frames=T, fps=60.0, tracker_clips=n)
        else:
            pipe = Pipeline(MODEL_LITE0, n, max_frames=T, fps=60.0, depth=3 if mode != "own" else 2)
        assert pipe._defer == (3 if mode == "defer" else 0)
        if live:
            pipe.enable_live(path_cap=1024, phase_cap=64)
    seen = []
    if mode == "runs":
        per = 64 // n
        for t0 in range(0, T, per):
            nf = min(per, T - t0)
            batch = torch.cat([fd[t0:t0 + nf, c] for c in range(n)])
            pipe.step_runs(batch, [(c, c * nf, nf, t0 + 1) for c in range(n)], stream=st)
            if live and t0 // per in polls:
                seen.append(pipe.live())
    else:
        for t in range(T):
            pipe.step(fd[t], st)
            if live and t in polls:
                seen.append(pipe.live())
    final = pipe.live(flush_view=True) if live else None
    best, n_rows, nph, ovf, ph = pipe.close(cap=32)
    counts, rows = pipe.rows_all()
    out = (best.copy(), n_rows.copy(), nph.copy(), ovf.copy(), ph.copy(), [rows[c][:counts[c]].tobytes() for c in range(n)])
    return out, final, seen, pipe


def _same(a, b):
    for i in range(5):
        assert np.array_equal(a[i], b[i]), i
    assert a[5] == b[5]


def _final_is_close(final, out):
    best, _, nph, ovf, ph = out[:5]
    for c, r in enumerate(final):
        assert ovf[c] == 0 and r.overflow == 0
        assert r.leader == best[c]
        assert np.array_equal(_phase_rows(r.phases), ph[c, :nph[c]]), c


@pytest.mark.parametrize("mode", ["own", "inline", "defer", "runs"])
def test_live_on_every_step_path_equals_close_and_does_not_perturb(mode, monkeypatch):
    """plain steps with the tracker on its own stream / inline, deferred small-batch groups, time-batched runs: rows and close() are the
    same with live analysis on and off, the final flush view is close(), and the polls in between see rows and seq only grow."""
    import torch
    n, T = 3, 420                                     # > 2 synthetic reps (3.3 s at 60 fps) per clip
    fd = torch.from_numpy(_frames(n, T)).to("cuda:0")
    base, _, _, _ = _run("own", fd, False, n, T, monkeypatch)
    assert int(base[2].sum()) > 0
    out, final, seen, pipe = _run(mode, fd, True, n, T, monkeypatch, polls=(3, 100, 250) if mode != "runs" else (1, 5))
    _same(base, out)
    _final_is_close(final, out)
    for a, b in zip(seen, seen[1:] + [final]):
        for ra, rb in zip(a, b):
            assert ra.rows <= rb.rows and ra.seq <= rb.seq
    if mode == "inline":                             # reset() clears the live state: the same clips again give the same answers
        pipe.reset()
        again, final2, _, _ = _run(mode, fd, True, n, T, monkeypatch, pipe=pipe)
        _same(base, again)
        _final_is_close(final2, again)


def test_tracker_only_steps_feed_the_live_analysis(monkeypatch):
    import torch
    n, T = 2, 200
    fd = torch.from_numpy(_frames(n, T, seed=90)).to("cuda:0")
    out, final, _, pipe = _run("own", fd, True, n, T, monkeypatch)
    _final_is_close(final, out)
    pipe.reset()
    st = torch.cuda.current_stream().cuda_stream
    pipe.step(fd[0], st)
    pipe._drain()
    before = pipe.live()
    pipe.tracker_only_steps(8, slot=0)
    after = pipe.live()
    rows = [len(pipe.rows(c)["id"]) for c in range(n)]
    assert [r.rows for r in after] == rows and sum(rows) > sum(r.rows for r in before)


def test_refusals_leave_the_handles_usable(monkeypatch):
    import torch
    from vbt_amd import _lib
    from vbt_amd.ocsort import LIVE_PATH_FULL, LIVE_PHASES_FULL, MultiClipTracker
    from vbt_amd.track import Pipeline
    monkeypatch.setenv("VBT_TRACKER_STREAM", "own")
    fd = torch.from_numpy(_frames(2, 4)).to("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    pipe = Pipeline(MODEL_LITE0, 2, max_frames=8, fps=30.0)
    for bad in ((1, 8), (64, 0), (64, 513), (65537, 8)):
        with pytest.raises(_lib.VbtArgError):
            pipe.enable_live(*bad)
    with pytest.raises(_lib.VbtError, match="error -5"):
        pipe.live()
    pipe.step(fd[0], st)
    with pytest.raises(_lib.VbtError, match="error -5"):
        pipe.enable_live()
    with pytest.raises(_lib.VbtError, match="error -5"):
        pipe.live()
    pipe.step(fd[1], st)                               # still usable
    pipe.reset()
    pipe.enable_live(path_cap=64, phase_cap=8)       # after a reset: allowed
    with pytest.raises(_lib.VbtError, match="error -5"):
        pipe.enable_live()                            # once
    pipe.step(fd[0], st)
    assert len(pipe.live()) == 2

    # tiny capacities on reference clip 001 (12 phases): flagged, never a wrong list
    from test_gpu_tracker import _pack
    from test_oracle_ocsort import frames_from_rows
    from test_oracle_ocsort_corpus import load_all
    corpus = load_all()
    fr, tm = frames_from_rows(corpus["001"][0])
    dets, counts, times = _pack([fr, fr], [tm, tm])
    mc = MultiClipTracker(2, 8192, max_age=30, asso_func="diou", iou_threshold=0.1)
    with pytest.raises(_lib.VbtError, match="error -5"):
        mc.live()
    mc.enable_live(path_cap=2, phase_cap=1)
    flags_seen = set()
    for f0 in range(0, counts.shape[0], 50):
        mc.update_frames(dets[f0:f0 + 50], counts[f0:f0 + 50], times[f0:f0 + 50])
        rows = mc.rows(0)
        for tid, tr in mc.live_tracks(0).items():
            flags_seen.add(tr.flags)
            if tr.flags == 0:
                assert np.array_equal(tr.phases, _oracle_phases(rows, tid))
            else:
                assert len(tr.phases) == 0
        r = mc.live()[0]
        assert r.overflow or np.array_equal(_phase_rows(r.phases), _oracle_phases(rows, r.leader))
    final = mc.live(flush_view=True)[0]
    assert final.overflow & LIVE_PATH_FULL and final.phases == []
    assert any(f & LIVE_PATH_FULL for f in flags_seen)
    mc2 = MultiClipTracker(1, 8192, max_age=30, asso_func="diou", iou_threshold=0.1)
    mc2.enable_live(path_cap=4096, phase_cap=1)
    mc2.update_frames(dets[:, :1], counts[:, :1], times[:, :1])
    r = mc2.live(flush_view=True)[0]
    assert r.overflow & LIVE_PHASES_FULL and r.phases == []
    with pytest.raises(_lib.VbtError, match="error -5"):
        mc2.enable_live()
    mc2.reset()                                       # the handle stays usable: same clip again, same flags
    mc2.update_frames(dets[:, :1], counts[:, :1], times[:, :1])
    assert mc2.live(flush_view=True)[0].overflow & LIVE_PHASES_FULL


def _standing_reps(output):
    """The rep lines `track --live` leaves standing: a rep line replaces rep i and everything after it, a revision drops from rep k."""
    reps = []
    for line in output.splitlines():
        m = re.match(r"  rep (\d+): ", line)
        if m:
            reps = reps[:int(m.group(1)) - 1] + [line]
        m = re.match(r"  revised: id -?\d+, from rep (\d+)", line)
        if m:
            reps = reps[:int(m.group(1)) - 1]
    return reps


def test_cli_track_live_prints_the_reps_analyze_prints(tmp_path):
    from click.testing import CliRunner
    from vbt_amd import synth
    from vbt_amd.cli import main
    frames = synth.clip_frames(12, 0, 460)
    src = tmp_path / "live_clip.npy"
    np.save(str(src), frames)
    out = tmp_path / "dfs"
    res = CliRunner().invoke(main, ["track", str(src), "--model", MODEL_LITE0, "--df_dir", str(out), "--fps", "60", "--detection_treshold", "0.3",
                                    "--live"])
    assert res.exit_code == 0, res.output
    plain = tmp_path / "plain"
    res2 = CliRunner().invoke(main, ["track", str(src), "--model", MODEL_LITE0, "--df_dir", str(plain), "--fps", "60", "--detection_treshold", "0.3"])
    assert res2.exit_code == 0, res2.output
    files = os.listdir(out)
    assert files == os.listdir(plain)
    import pandas as pd
    assert pd.read_pickle(os.path.join(out, files[0])).equals(pd.read_pickle(os.path.join(plain, files[0])))   # the export is untouched
    ana = CliRunner().invoke(main, ["analyze", os.path.join(out, files[0])])
    assert ana.exit_code == 0, ana.output
    want = [ln for ln in ana.output.splitlines() if ln.startswith("  rep ")]
    assert len(want) >= 1
    assert _standing_reps(res.output) == want
