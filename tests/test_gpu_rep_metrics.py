"""Rep metrics on the device ("Rep metrics"): the eight per-phase values formed inside the scan equal the reference
(tests/rep_metrics_ref.py: the oracle's VelocityTracker recording them in _end_phase) bit for bit - on crafted tracks, on the 34 golden
clips, at the clip close, in the live analysis and on a recycled pipeline slot - and enabling them changes no other output."""
import csv
import ctypes
import os
import re

import numpy as np
import pytest

import rep_metrics_ref as R
from conftest import MODEL_LITE0

pytestmark = pytest.mark.gpu
COLS = list(R.COLS)
ERR_CAPACITY, ERR_STATE = -4, -5


def _phase_rows(phases):
    return np.asarray([[p.time_start, p.time_end, p.y_start, p.y_end, p.rom, float(p.type)] for p in phases], np.float64).reshape(-1, 6)


def _device(rows7, **kw):
    """vbt_analyze_metrics and vbt_analyze on the same rows: (phases [P,6], metrics [P,8]); the two phase lists must be the same bytes"""
    from vbt_amd.velocity import analyze_rows
    ph, m = analyze_rows(rows7, metrics=True, **kw)
    plain = analyze_rows(rows7, **kw)
    ph = _phase_rows(ph)
    assert ph.tobytes() == _phase_rows(plain).tobytes()
    return ph, m


def _against_ref(rows7, what, **kw):
    ph, m = _device(rows7, **kw)
    rph, rm, vt = R.run(rows7, **kw)
    assert np.array_equal(ph, rph), what
    assert m.shape == rm.shape and np.array_equal(m, rm), (what, m, rm)
    return ph, m, vt


# ---- 1. vbt_analyze_metrics on crafted tracks (preprocess = 0: the test controls dy exactly) ----
def _track(ys, times=None):
    """rows [T,7] from a y series: x wanders, the plate size breathes a little, 30 fps unless times are given"""
    ys = np.asarray(ys, np.float64)
    T = len(ys)
    t = (np.arange(T) + 1) / 30.0 if times is None else np.asarray(times, np.float64)
    x = 0.5 + 0.01 * np.sin(np.arange(T) * 0.7) + 0.002 * np.arange(T)
    h = 0.2 + 0.003 * np.cos(np.arange(T) * 0.3)
    w = 0.21 + 0.002 * np.sin(np.arange(T) * 0.5)
    return np.stack([t, x, ys, np.zeros(T), np.zeros(T), h, w], axis=1)


def _ramp(y0, step, n):
    return [y0 + step * (i + 1) for i in range(n)]


UP_DOWN = [0.3] + _ramp(0.3, 0.02, 10) + _ramp(0.5, -0.02, 10) + _ramp(0.3, 0.02, 4)    # eccentric, concentric, then the rise that ends it
RAW = dict(preprocess=False, plate_diameter=0.45)


def test_crafted_eccentric_then_concentric():
    ph, m, _ = _against_ref(_track(UP_DOWN), "a", flush=True, **RAW)
    assert ph[:2, 5].tolist() == [1.0, 0.0] and np.all(m[:2, R.N_STEPS] >= 8) and np.all(m[:2, R.PV] > 0)


def test_crafted_hold_row_leaves_a_gap_in_the_path():
    ys = [0.3, 0.32, 0.34, 0.34, 0.36] + _ramp(0.36, 0.02, 8) + _ramp(0.52, -0.02, 3)     # row 3: dy == 0 in HOLD, neither appended nor a reset
    ph, m, vt = _against_ref(_track(ys), "b", flush=True, **RAW)
    assert vt.gaps >= 1 and len(ph) >= 1


def test_crafted_filter_drops_a_phase_after_its_metrics_were_stored():
    ys = [0.3] + _ramp(0.3, 0.01, 9) + _ramp(0.39, -0.02, 12) + _ramp(0.15, 0.02, 3)      # eccentric of 0.07, then a concentric of 0.2
    ph, m, vt = _against_ref(_track(ys), "c", flush=False, **RAW)
    assert vt.appended == 2 and len(ph) == 1 and ph[0, 5] == 0.0


def test_crafted_phase_that_only_the_flush_ends():
    ys = UP_DOWN[:21] + _ramp(0.3, 0.02, 9)                                                 # the last rise never turns
    open_, _, _ = _against_ref(_track(ys), "d0", flush=False, **RAW)
    flushed, m, _ = _against_ref(_track(ys), "d1", flush=True, **RAW)
    assert len(flushed) == len(open_) + 1 and m[-1, R.N_STEPS] >= 7


def test_crafted_empty_step_range():
    ys = [0.5, 0.49, 0.48, 0.47, 0.9, 0.91]               # concentric whose path has its minimum before its maximum: st > en
    ph, m, _ = _against_ref(_track(ys), "e", flush=False, min_distance=0.0, **RAW)
    assert len(ph) == 1 and ph[0, 4] == 0.0
    assert m[0, R.N_STEPS] == 0.0 and m[0, R.T_PV] == ph[0, 0] and not m[0, [R.PV, R.ROM_Y, R.ROM_X, R.PV_Y, R.MV, R.X_DEV]].any()


def test_crafted_equal_time_stamps():
    t = ((np.arange(len(UP_DOWN)) + 1) / 30.0).tolist()
    t[5] = t[4]                                             # inside the eccentric phase ...
    t[15] = t[14]                                           # ... and inside the concentric one: those steps count for the sums only
    ph, m, _ = _against_ref(_track(UP_DOWN, t), "f", flush=True, **RAW)
    assert len(ph) >= 2 and np.all(np.isfinite(m))


def test_capacity_smaller_than_the_phase_count():
    from vbt_amd import _lib
    rows = np.ascontiguousarray(_track(UP_DOWN))
    ph, m, n = np.zeros((1, 6)), np.zeros((1, 8)), ctypes.c_int()
    args = (rows.ctypes.data, len(rows), 0, 1, 0.45, 0.6, 0.1)
    assert _lib.lib().vbt_analyze_metrics(*args, ph.ctypes.data, m.ctypes.data, 1, ctypes.byref(n), 0) == ERR_CAPACITY
    assert _lib.lib().vbt_analyze(*args, ph.ctypes.data, 1, ctypes.byref(n), 0) == ERR_CAPACITY
    assert not ph.any() and not m.any()                    # refused: nothing written


def test_corpus_all_34_clips():
    total = 0
    for name, cols, gold in R.corpus():
        ph, m = _device(cols, plate_diameter=0.45, preprocess=True)
        rph, rm, _ = R.corpus_ref(name, cols)
        assert np.array_equal(ph, gold) and np.array_equal(ph, rph), name
        assert np.array_equal(m, rm), name
        total += len(ph)
    assert total == 508


def test_velocity_tracker_class_rep_metrics():
    from vbt_amd.velocity import VelocityTracker
    rows = _track(UP_DOWN)
    vt = VelocityTracker(0.45)
    for r in rows:
        vt.process_measurements(*r)
    with pytest.raises(RuntimeError):
        vt.rep_metrics
    vt.end_processing()
    assert np.array_equal(vt.rep_metrics, R.run(rows, preprocess=False)[1]) and len(vt.phases) == len(vt.rep_metrics)


# ---- 2 + 3. tracker close and live analysis on two corpus clips ----
CLIPS = ["005", "007"]                                      # both hold phases whose path skips a row


def _clips_packed(clips):
    """the clips' boxes as the tracker takes them, the way tests/test_gpu_live.py replays the corpus"""
    from test_gpu_tracker import _pack
    from test_oracle_ocsort import frames_from_rows
    from test_oracle_ocsort_corpus import load_all
    corpus = load_all()
    data = [frames_from_rows(corpus[c][0]) for c in clips]
    return _pack([d[0] for d in data], [d[1] for d in data])


@pytest.fixture(scope="module")
def replay():
    """The two clips through four trackers fed the same launches: plain, live only, metrics only, live + metrics (polled twice mid-clip)."""
    from vbt_amd.ocsort import MultiClipTracker
    dets, counts, times = _clips_packed(CLIPS)
    F = counts.shape[0]
    kw = dict(max_age=30, asso_func="diou", iou_threshold=0.1)
    plain, live = MultiClipTracker(2, 8192, **kw), MultiClipTracker(2, 8192, **kw)
    met, both = MultiClipTracker(2, 8192, rep_metrics=True, **kw), MultiClipTracker(2, 8192, **kw)
    both.enable_live(path_cap=4096, phase_cap=128)         # the metrics enable after the live enable ...
    both.enable_rep_metrics()
    live.enable_live(path_cap=4096, phase_cap=128)
    cuts = [0, F // 3, (2 * F) // 3, F]
    polls = []
    for f0, f1 in zip(cuts, cuts[1:]):
        for mc in (plain, live, met, both):
            mc.update_frames(dets[f0:f1], counts[f0:f1], times[f0:f1])
        polls.append(dict(rows=[both.rows(c) for c in range(2)], open=both.live(), flush=both.live(flush_view=True),
                          seq=[r.seq for r in live.live()]))
    for mc in (plain, live, met, both):
        mc.finish(0.45)
    return dict(plain=plain, live=live, met=met, both=both, polls=polls)


def _id_rows(rows, tid):
    m = np.asarray(rows["id"]) == tid
    return np.stack([np.asarray(rows[c], np.float64)[m] for c in COLS], axis=1)


def test_tracker_close_metrics(replay):
    from vbt_amd import _lib
    plain, met = replay["plain"], replay["met"]
    best, n_rows, nph, ovf, ph, m = met.summary_ex(cap=64)
    pbest, prows, pnph, povf, pph = plain.summary(cap=64)
    for a, b in ((best, pbest), (n_rows, prows), (nph, pnph), (ovf, povf), (ph, pph)):
        assert a.tobytes() == b.tobytes()                   # enabling metrics changed nothing else
    for c in range(2):
        assert met.rows(c) == plain.rows(c)
        bid, phc = met.phases(c)
        assert phc.tobytes() == plain.phases(c)[1].tobytes()
        want_ph, want_m = _device(_id_rows(met.rows(c), bid), plate_diameter=0.45, preprocess=True)
        rph, rm, _ = R.run(_id_rows(met.rows(c), bid))
        assert np.array_equal(want_ph, rph) and np.array_equal(want_m, rm)
        assert len(want_ph) > 4 and np.array_equal(phc, want_ph)
        assert np.array_equal(met.rep_metrics(c), want_m), c
        assert nph[c] == len(want_m) and np.array_equal(m[c, :nph[c]], want_m), c
    with pytest.raises(_lib.VbtError, match="error -5"):
        plain.rep_metrics(0)
    with pytest.raises(_lib.VbtError, match="error -5"):
        plain.summary_ex()
    with pytest.raises(_lib.VbtError, match="error -5"):
        plain.enable_rep_metrics()                          # stepped: too late


def test_live_metrics_equal_the_reference_on_the_rows_so_far(replay):
    both, polls = replay["both"], replay["polls"]
    seen = 0
    for p in polls:
        for c in range(2):
            for rec, flush in ((p["open"][c], False), (p["flush"][c], True)):
                assert rec.overflow == 0 and rec.leader >= 0
                rph, rm, _ = R.run(_id_rows(p["rows"][c], rec.leader), flush=flush)
                assert np.array_equal(_phase_rows(rec.phases), rph), (c, flush)
                assert rec.metrics.shape == rm.shape and np.array_equal(rec.metrics, rm), (c, flush)
                seen += len(rm)
        assert [r.seq for r in p["open"]] == p["seq"] == [r.seq for r in p["flush"]]      # the seq counters of a run without metrics
    assert seen > 20
    for c, rec in enumerate(polls[-1]["flush"]):            # after the last frame the flush view is the close
        bid, ph = both.phases(c)
        assert rec.leader == bid and np.array_equal(_phase_rows(rec.phases), ph)
        assert np.array_equal(rec.metrics, both.rep_metrics(c)) and np.array_equal(rec.metrics, replay["met"].rep_metrics(c))
    assert replay["live"].rows(0) == both.rows(0) and replay["live"].phases(1)[1].tobytes() == both.phases(1)[1].tobytes()


def test_live_phase_list_overflow_reports_no_metrics():
    from vbt_amd.ocsort import LIVE_PHASES_FULL, MultiClipTracker
    dets, counts, times = _clips_packed(CLIPS[:1])
    mc = MultiClipTracker(1, 8192, max_age=30, asso_func="diou", iou_threshold=0.1, rep_metrics=True)    # ... and before it
    mc.enable_live(path_cap=4096, phase_cap=2)
    mc.update_frames(dets, counts, times)
    r = mc.live(flush_view=True)[0]
    assert r.overflow & LIVE_PHASES_FULL and r.phases == [] and r.metrics.shape == (0, 8)
    mc.finish(0.45)
    assert len(mc.rep_metrics(0)) > 2                       # the close is not bound by phase_cap


# ---- 4. pipeline: a recycled slot ----
def test_pipeline_recycled_slot_metrics():
    from vbt_amd import _lib, synth
    from vbt_amd.track import Pipeline
    a, b = synth.clip_frames(41, 13, 260), synth.clip_frames(44, 52, 460)

    def feed(pipe, frames):
        for f0 in range(0, len(frames), 16):
            n = min(16, len(frames) - f0)
            pipe.step_runs([np.ascontiguousarray(frames[f0:f0 + n])], [(0, 0, n, f0 + 1)])

    kw = dict(max_frames=460, fps=60.0, rows_per_frame=25, tracker_clips=1)
    pipe = Pipeline(MODEL_LITE0, 16, slot_close=True, rep_metrics=True, **kw)
    feed(pipe, a)
    pipe.close_clips([0])
    best_a, rows_a, ph_a, ovf_a, m_a = pipe.closed_ex(0)
    feed(pipe, b)
    best, _, nph, ovf, ph, m = pipe.close_ex(cap=64)
    fresh = Pipeline(MODEL_LITE0, 16, rep_metrics=True, **kw)
    feed(fresh, b)
    fbest, _, fnph, fovf, fph, fm = fresh.close_ex(cap=64)
    assert ovf[0] == fovf[0] == ovf_a == 0 and best[0] == fbest[0] and nph[0] == fnph[0] >= 1
    assert ph.tobytes() == fph.tobytes() and m.tobytes() == fm.tobytes()
    for frames_rows, tid, got_ph, got_m in ((rows_a, best_a, _phase_rows(ph_a), m_a), (fresh.rows(0), fbest[0], fph[0, :fnph[0]], fm[0, :fnph[0]])):
        rph, rm, _ = R.run(_id_rows(frames_rows, tid))
        assert len(rm) >= 1 and np.array_equal(got_ph, rph) and np.array_equal(got_m, rm)
    off = Pipeline(MODEL_LITE0, 16, **kw)
    with pytest.raises(_lib.VbtError, match="error -5"):
        off.close_ex()


# ---- 5. CLI ----
def test_cli_analyze_report_and_csv(tmp_path):
    import pandas as pd
    from click.testing import CliRunner
    from vbt_amd.cli import REPORT_CSV_COLUMNS, main
    name, cols, _ = R.corpus()[4]
    df = pd.DataFrame({"id": np.full(len(cols), 3, np.int64), **{c: cols[:, j] for j, c in enumerate(COLS)}})
    path = tmp_path / f"clip{name}_id3_lite0.pkl.gz"
    df.to_pickle(str(path))
    out = tmp_path / "report.csv"
    res = CliRunner().invoke(main, ["analyze", str(path), "--report", "--report_csv", str(out)])
    assert res.exit_code == 0, res.output
    plain = CliRunner().invoke(main, ["analyze", str(path)])
    ph, m, _ = R.corpus_ref(name, cols)
    rep, loss = R.set_report(ph, m, 0.0)
    conc = [i for i in range(len(ph)) if ph[i, 5] == 0.0]
    lines, plines = res.output.splitlines(), plain.output.splitlines()
    assert lines[0] == plines[0] and len(lines) == len(plines) + 1
    for k, i in enumerate(conc, 1):
        assert lines[k].startswith(plines[k] + "  PV ")       # the plain rep line, then the new columns
        assert lines[k].endswith(f"  PV {m[i, R.PV]:.6f} m/s  TTP {m[i, R.T_PV] - ph[i, 0]:.4f} s  vROM {m[i, R.ROM_Y]:.6f} m"
                                 f"  xdev {m[i, R.X_DEV]:.6f} m  loss {loss[k - 1]:.2f} %")
    assert lines[-1].startswith(f"  set: {rep['n_reps']} reps  best ACV {rep['best_mv']:.6f} m/s (rep {rep['best_rep']})  mean ACV {rep['mean_mv']:.6f} m/s")
    assert f"loss {rep['loss_last_pct']:.2f} %" in lines[-1] and f"max PV {rep['max_pv']:.6f} m/s" in lines[-1]
    with open(out, newline="") as f:
        table = list(csv.reader(f))
    assert tuple(table[0]) == REPORT_CSV_COLUMNS and len(table) == 1 + len(conc)
    for k, i in enumerate(conc, 1):
        row = dict(zip(table[0], table[k]))
        assert (row["video"], row["id"], row["rep"]) == (f"clip{name}", "3", str(k))
        want = dict(time_start=ph[i, 0], time_end=ph[i, 1], rom=ph[i, 4], acv=m[i, R.MV], pv=m[i, R.PV], t_pv=m[i, R.T_PV],
                    time_to_peak=m[i, R.T_PV] - ph[i, 0], rom_y=m[i, R.ROM_Y], rom_x=m[i, R.ROM_X], pv_y=m[i, R.PV_Y], x_dev=m[i, R.X_DEV],
                    n_steps=m[i, R.N_STEPS], loss_pct=loss[k - 1])
        for key, v in want.items():
            assert float(row[key]) == float(v), (k, key)


def test_cli_track_live_report_and_stop_loss(tmp_path):
    import pandas as pd
    from click.testing import CliRunner
    from test_gpu_live import _standing_reps
    from vbt_amd import synth
    from vbt_amd.cli import main
    src = tmp_path / "live_clip.npy"
    np.save(str(src), synth.clip_frames(12, 0, 460))
    base = ["track", str(src), "--model", MODEL_LITE0, "--fps", "60", "--detection_treshold", "0.3", "--live"]
    plain = CliRunner().invoke(main, base + ["--df_dir", str(tmp_path / "dfs")])
    assert plain.exit_code == 0, plain.output
    files = os.listdir(tmp_path / "dfs")
    df = pd.read_pickle(os.path.join(tmp_path / "dfs", files[0]))
    tid = int(re.search(r"_id(\d+)_", files[0]).group(1))
    ph, m, _ = R.run(np.stack([df[df["id"] == tid][c].to_numpy(np.float64) for c in COLS], axis=1))
    worst = max(R.set_report(ph, m, 0.0)[1])
    thr = repr(worst / 2) if worst > 0 else "0.5"           # a threshold the set reaches, whenever it loses any velocity at all
    rep, loss = R.set_report(ph, m, float(thr))
    assert (rep["stop_rep"] > 0) == (worst > 0)
    res = CliRunner().invoke(main, base + ["--report", "--stop_loss", thr])
    assert res.exit_code == 0, res.output
    want, got = _standing_reps(plain.output), _standing_reps(res.output)
    assert len(want) == rep["n_reps"] >= 2 and len(got) == len(want)
    conc = [i for i in range(len(ph)) if ph[i, 5] == 0.0]
    for k, (w, g, i) in enumerate(zip(want, got, conc)):
        assert g == w + (f"  PV {m[i, R.PV]:.6f} m/s  TTP {m[i, R.T_PV] - ph[i, 0]:.4f} s  vROM {m[i, R.ROM_Y]:.6f} m"
                         f"  xdev {m[i, R.X_DEV]:.6f} m  loss {loss[k]:.2f} %")
    stops = [ln for ln in res.output.splitlines() if ln.startswith("  STOP: ")]
    if rep["stop_rep"]:
        assert stops and stops[-1] == f"  STOP: rep {rep['stop_rep']} lost {loss[rep['stop_rep'] - 1]:.2f} % (threshold {float(thr):g} %)"
    else:
        assert stops == []
