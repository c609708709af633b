"""vbt_set_summary (host only: the library is loaded, no device is touched) against a few lines of numpy on the corpus' reference
metrics and on crafted lists; the usage errors of the new CLI flags."""
import ctypes
import math

import numpy as np
import pytest

import rep_metrics_ref as R

FIELDS = ("n_reps", "best_rep", "stop_rep", "best_mv", "last_mv", "mean_mv", "mean_pv", "max_pv", "loss_last_pct", "concentric_s", "eccentric_s",
          "mean_x_dev")


def _call(ph, m, stop, cap=None):
    from vbt_amd import _lib
    ph = np.ascontiguousarray(ph, np.float64).reshape(-1, 6)
    m = np.ascontiguousarray(m, np.float64).reshape(-1, 8)
    cap = len(ph) if cap is None else cap
    rep, loss = _lib.SetReport(), np.full(max(cap, 1) + 1, -7.0)
    rc = _lib.lib().vbt_set_summary(ph.ctypes.data, m.ctypes.data, len(ph), float(stop), ctypes.byref(rep), loss.ctypes.data, cap)
    return rc, rep, loss


def _numpy(ph, m, stop):
    """the ten lines: sums in list order (cumsum), best so far by maximum.accumulate"""
    ph, m = np.asarray(ph, np.float64).reshape(-1, 6), np.asarray(m, np.float64).reshape(-1, 8)
    c = ph[:, 5] == 0
    mv, pv, xd = m[c, R.MV], m[c, R.PV], m[c, R.X_DEV]
    n = int(c.sum())
    best = np.maximum.accumulate(mv) if n else mv
    loss = np.where(best > 0, 100.0 * (1.0 - mv / np.where(best > 0, best, 1.0)), 0.0)
    hit = np.flatnonzero(loss >= stop) if stop > 0 else []
    tot = lambda v: float(np.cumsum(v)[-1]) if len(v) else 0.0                                   # noqa: E731
    dur = ph[:, 1] - ph[:, 0]
    return dict(n_reps=n, best_rep=int(np.argmax(mv)) + 1 if n else 0, stop_rep=int(hit[0]) + 1 if len(hit) else 0,
                best_mv=float(mv.max()) if n else 0.0, last_mv=float(mv[-1]) if n else 0.0, mean_mv=tot(mv) / n if n else 0.0,
                mean_pv=tot(pv) / n if n else 0.0, max_pv=float(pv.max()) if n else 0.0, loss_last_pct=float(loss[-1]) if n else 0.0,
                concentric_s=tot(dur[c]), eccentric_s=tot(dur[ph[:, 5] == 1]), mean_x_dev=tot(xd) / n if n else 0.0), loss


def _check(ph, m, stop, cap=None):
    rc, rep, loss = _call(ph, m, stop, cap)
    assert rc == 0
    want, wloss = _numpy(ph, m, stop)
    for k in FIELDS:
        assert getattr(rep, k) == want[k], (k, getattr(rep, k), want[k])
    ref, rloss = R.set_report(ph, m, stop)                      # and the plain Python statement of the same
    assert {k: getattr(rep, k) for k in FIELDS} == ref
    k = want["n_reps"] if cap is None else min(cap, want["n_reps"])
    assert np.array_equal(loss[:k], wloss[:k]) and np.array_equal(loss[:k], np.asarray(rloss[:k]))
    assert np.all(loss[k:] == -7.0)                              # nothing written past min(n_reps, cap)
    return rep


def test_corpus_sets():
    stops = 0
    for name, cols, _ in R.corpus():
        ph, m, _ = R.corpus_ref(name, cols)
        for stop in (0.0, 10.0, 20.0):
            stops += _check(ph, m, stop).stop_rep > 0
    assert stops > 10                                            # the thresholds are reached on real sets


def _list(mvs, types=None, pvs=None):
    n = len(mvs)
    ph, m = np.zeros((n, 6)), np.zeros((n, 8))
    ph[:, 0] = np.arange(n) * 2.0
    ph[:, 1] = ph[:, 0] + 0.5 + 0.125 * np.arange(n)
    ph[:, 4] = 0.5
    ph[:, 5] = 0 if types is None else types
    m[:, R.MV] = mvs
    m[:, R.PV] = np.asarray(mvs) * 1.5 if pvs is None else pvs
    m[:, R.X_DEV] = 0.01 * (1 + np.arange(n))
    return ph, m


def test_crafted_lists():
    rep = _check(*_list([0.5, 0.4], types=[1, 1]), 10.0)                     # no concentric phase
    assert (rep.n_reps, rep.best_rep, rep.stop_rep, rep.mean_mv, rep.concentric_s) == (0, 0, 0, 0.0, 0.0) and rep.eccentric_s > 0
    rep = _check(np.zeros((0, 6)), np.zeros((0, 8)), 10.0)                   # no phase at all
    assert rep.n_reps == 0
    rep = _check(*_list([0.7]), 10.0)                                        # a single rep
    assert (rep.n_reps, rep.best_rep, rep.stop_rep, rep.loss_last_pct, rep.best_mv) == (1, 1, 0, 0.0, 0.7)
    rep = _check(*_list([0.6, 0.8, 0.8, 0.7, 0.8]), 10.0)                    # ties go to the earlier rep
    assert (rep.best_rep, rep.stop_rep) == (2, 4)
    rep = _check(*_list([0.0, 0.0, 0.0]), 10.0)                              # mv = 0 throughout: no loss, no stop
    assert (rep.best_rep, rep.stop_rep, rep.loss_last_pct, rep.best_mv) == (1, 0, 0.0, 0.0)
    ph, m = _list([0.8, 1.0, 0.9, 0.5, 0.7], types=[0, 1, 0, 0, 0])          # an eccentric phase between the reps
    assert _check(ph, m, 30.0).stop_rep == 3
    assert _check(ph, m, 0.0).stop_rep == 0 and _check(ph, m, -5.0).stop_rep == 0
    rep = _check(ph, m, 20.0, cap=2)                                         # cap smaller than the number of reps
    assert (rep.n_reps, rep.stop_rep) == (4, 3)
    _check(ph, m, 20.0, cap=0)


def test_refused_arguments():
    from vbt_amd import _lib
    L = _lib.lib()
    ph, m = _list([0.8, 0.6])
    for bad in (math.nan, math.inf, -math.inf):
        assert _call(ph, m, bad)[0] == -1                                    # VBT_ERR_ARG
    rep, loss = _lib.SetReport(), np.zeros(4)
    args = [ph.ctypes.data, m.ctypes.data, 2, 10.0, ctypes.byref(rep), loss.ctypes.data, 4]
    assert L.vbt_set_summary(*args) == 0
    for i, v in ((0, None), (1, None), (4, None), (5, None), (2, -1), (6, -1)):
        a = list(args)
        a[i] = v
        assert L.vbt_set_summary(*a) == -1, i
    assert b"vbt_set_summary" in L.vbt_last_error()


def test_abi_entries_are_declared_and_bound():
    import os
    import re
    from vbt_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "vbt_hip.h")).read()
    for name in ("vbt_analyze_metrics", "vbt_tracker_rep_metrics_enable", "vbt_tracker_rep_metrics", "vbt_tracker_summary_ex", "vbt_tracker_live_poll_ex",
                 "vbt_pipeline_rep_metrics_enable", "vbt_pipeline_close_ex", "vbt_pipeline_closed_clip_ex", "vbt_pipeline_live_poll_ex", "vbt_set_summary"):
        assert re.search(rf"\bint {name}\(", hdr), name
        assert name in _lib.declared_symbols(), name
    macros = dict(re.findall(r"#define (VBT_RM_\w+|VBT_REP_METRICS) (\d+)", hdr))
    assert macros == dict(VBT_REP_METRICS="8", VBT_RM_PV="0", VBT_RM_T_PV="1", VBT_RM_ROM_Y="2", VBT_RM_ROM_X="3", VBT_RM_PV_Y="4", VBT_RM_MV="5",
                          VBT_RM_X_DEV="6", VBT_RM_N_STEPS="7")
    assert (R.PV, R.T_PV, R.ROM_Y, R.ROM_X, R.PV_Y, R.MV, R.X_DEV, R.N_STEPS) == tuple(range(8))
    assert ctypes.sizeof(_lib.SetReport) == 16 + 9 * 8


def test_set_report_wrapper():
    from vbt_amd.velocity import Phase, set_report
    ph, m = _list([0.8, 1.0, 0.9, 0.5, 0.7], types=[0, 1, 0, 0, 0])
    rep = set_report([Phase(r[0], r[1], r[2], r[3], r[4], int(r[5])) for r in ph], m, 30.0)
    want, loss = R.set_report(ph, m, 30.0)
    assert {k: getattr(rep, k) for k in FIELDS} == want and rep.loss_pct.tolist() == loss
    with pytest.raises(ValueError):
        set_report(ph, m[:3])


@pytest.mark.parametrize("args, text", [
    (["track", "x.npy", "--stop_loss", "20"], "--stop_loss watches the reps as they complete: give --live"),
    (["track", "x.npy", "--live", "--stop_loss", "0"], "must be a finite percentage above 0"),
    (["track", "x.npy", "--live", "--stop_loss", "-3"], "must be a finite percentage above 0"),
    (["track", "x.npy", "--live", "--stop_loss", "nan"], "must be a finite percentage above 0"),
    (["track", "x.npy", "--live", "--stop_loss", "inf"], "must be a finite percentage above 0"),
    (["track", "x.npy", "--report"], "--report extends the rep lines of --live"),
    (["analyze", "x_id1_m.pkl.gz", "--report_csv", "out.csv"], "--report_csv writes the rows of --report: give --report"),
])
def test_cli_usage_errors(args, text):
    from click.testing import CliRunner
    from vbt_amd.cli import main
    r = CliRunner().invoke(main, args)
    assert r.exit_code == 2 and text in r.output, r.output
