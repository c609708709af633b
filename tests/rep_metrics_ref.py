"""Reference of the per-phase rep metrics ("Rep metrics"): oracle.velocity.VelocityTracker with the eight
values recorded in _end_phase, from the very path arrays and step range `rom` is summed over, and dropped in _filter together with
their phase.  Plain Python floats in index order i = st+1 .. en: the device forms the same doubles in the same order, so every
comparison against this file is array_equal.  Test infrastructure only."""
import json
import math
import os

import numpy as np

from oracle import velocity as ov

PV, T_PV, ROM_Y, ROM_X, PV_Y, MV, X_DEV, N_STEPS = range(8)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COLS = ("time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width")


class MetricsTracker(ov.VelocityTracker):
    def __init__(self, plate_diameter, diff_threshold=0.6, min_distance=0.1):
        super().__init__(plate_diameter, diff_threshold, min_distance)
        self.metrics = []          # one list of 8 floats per phase of self.phases, same order
        self.appended = 0          # phases ever appended (those the filter dropped later included)
        self.gaps = 0              # appended phases whose path skipped a row (see process_measurements)
        self._rows_seen = 0
        self._row_of = []          # row number of every path sample

    def _filter(self):
        thr = self.max_y_diff / 2
        keep = [not (p.y_diff < thr) for p in self.phases]
        self.metrics = [m for m, k in zip(self.metrics, keep) if k]
        self.phases = [p for p, k in zip(self.phases, keep) if k]

    def _append(self, x, y, w, h, t):
        super()._append(x, y, w, h, t)
        self._row_of.append(self._rows_seen)

    def _reset(self):
        super()._reset()
        self._row_of = []

    def process_measurements(self, *a):
        self._rows_seen += 1
        super().process_measurements(*a)

    def _phase_metrics(self, s, e, rom):
        xs, ys, ws, hs, ts, D = self.xs, self.ys, self.widths, self.heights, self.times, self.plate_diameter
        pv, t_pv, rom_y, rom_x, pv_y, x_dev = 0.0, ts[s], 0.0, 0.0, 0.0, 0.0
        for i in range(s + 1, e + 1):
            ddx = abs(xs[i] - xs[i - 1]) / ((ws[i] + ws[i - 1]) / 2) * D
            ddy = abs(ys[i] - ys[i - 1]) / ((hs[i] + hs[i - 1]) / 2) * D
            rom_x += ddx
            rom_y += ddy
            dt = ts[i] - ts[i - 1]
            if dt > 0:
                v = (ddx + ddy) / dt
                if v > pv:
                    pv, t_pv = v, ts[i]
                vy = ddy / dt
                if vy > pv_y:
                    pv_y = vy
            dev = abs(xs[i] - xs[s]) / ((ws[i] + ws[s]) / 2) * D
            if dev > x_dev:
                x_dev = dev
        dur = ts[e] - ts[s]
        mv = rom / dur if dur > 0 else 0.0
        return [pv, t_pv, rom_y, rom_x, pv_y, mv, x_dev, float(e - s) if e > s else 0.0]

    def _end_phase(self):
        # oracle.velocity.VelocityTracker._end_phase, statement for statement, + the metrics of the phase it appends
        if self.current_phase == ov.CONCENTRIC:
            s, e = self._argmax(self.ys), self._argmin(self.ys)
        else:
            s, e = self._argmin(self.ys), self._argmax(self.ys)
        y_diff = abs(self.ys[s] - self.ys[e])
        if self.max_y_diff is None or y_diff > self.max_y_diff:
            self.max_y_diff = y_diff
            self._filter()
        if y_diff > self.max_y_diff * self.diff_threshold:
            distance = 0
            for i in range(s + 1, e + 1):
                ddx = abs(self.xs[i] - self.xs[i - 1]) / ((self.widths[i] + self.widths[i - 1]) / 2) * self.plate_diameter
                ddy = abs(self.ys[i] - self.ys[i - 1]) / ((self.heights[i] + self.heights[i - 1]) / 2) * self.plate_diameter
                distance += ddx + ddy
            if distance < self.min_distance:
                self.neg = self.pos = 0
                self.current_phase = ov.HOLD
                return
            self.phases.append(ov.Phase(self.times[s], self.times[e], self.ys[s], self.ys[e], distance, self.current_phase))
            self.metrics.append(self._phase_metrics(s, e, distance))
            self.appended += 1
            r = self._row_of
            if any(b - a != 1 for a, b in zip(r, r[1:])):
                self.gaps += 1
            self._filter()
        self.current_phase = ov.HOLD
        self.pos = self.neg = 0


def run(cols7, plate_diameter=0.45, diff_threshold=0.6, min_distance=0.1, preprocess=True, flush=True):
    """cols7 [T,7] = time,x,y,dx,dy,h,w of one track -> (phases float64 [P,6], metrics float64 [P,8], the tracker)"""
    c = np.asarray(cols7, np.float64).reshape(-1, 7)
    cols = [c[:, j].tolist() for j in range(7)]
    if preprocess:
        cols = ov.preprocess(*cols)
    vt = MetricsTracker(plate_diameter, diff_threshold, min_distance)
    for i in range(len(c)):
        vt.process_measurements(*(col[i] for col in cols))
    if flush:
        vt.end_processing()
    return (np.asarray([p.as_row() for p in vt.phases], np.float64).reshape(-1, 6),
            np.asarray(vt.metrics, np.float64).reshape(-1, 8), vt)


def set_report(phases6, metrics8, stop_loss_pct):
    """vbt_set_summary in plain Python: (dict of the report's fields, per-rep loss list).  Sums run in list order."""
    ph = np.asarray(phases6, np.float64).reshape(-1, 6)
    m = np.asarray(metrics8, np.float64).reshape(-1, 8)
    conc = [i for i in range(len(ph)) if ph[i, 5] == 0.0]
    rep = dict(n_reps=len(conc), best_rep=0, stop_rep=0, best_mv=0.0, last_mv=0.0, mean_mv=0.0, mean_pv=0.0, max_pv=0.0,
               loss_last_pct=0.0, concentric_s=0.0, eccentric_s=0.0, mean_x_dev=0.0)
    for i in range(len(ph)):
        if ph[i, 5] == 0.0:
            rep["concentric_s"] += float(ph[i, 1] - ph[i, 0])
        elif ph[i, 5] == 1.0:
            rep["eccentric_s"] += float(ph[i, 1] - ph[i, 0])
    loss, best, s_mv, s_pv, s_xd = [], -math.inf, 0.0, 0.0, 0.0
    for k, i in enumerate(conc, 1):
        mv, pv = float(m[i, MV]), float(m[i, PV])
        if mv > best:
            best, rep["best_rep"] = mv, k
        lk = 100.0 * (1.0 - mv / best) if best > 0 else 0.0
        loss.append(lk)
        if stop_loss_pct > 0 and rep["stop_rep"] == 0 and lk >= stop_loss_pct:
            rep["stop_rep"] = k
        s_mv += mv
        s_pv += pv
        s_xd += float(m[i, X_DEV])
        if pv > rep["max_pv"]:
            rep["max_pv"] = pv
        rep["last_mv"], rep["loss_last_pct"] = mv, lk
    if conc:
        n = float(len(conc))
        rep.update(best_mv=best, mean_mv=s_mv / n, mean_pv=s_pv / n, mean_x_dev=s_xd / n)
    return rep, loss


_corpus = None


def corpus():
    """The 34 golden clips: list of (name, cols7 [T,7] raw rows of the exported id, golden phases [P,6]), loaded once."""
    global _corpus
    if _corpus is None:
        z = np.load(os.path.join(GOLDEN, "dfs_ocsort_main.npz"))
        with open(os.path.join(GOLDEN, "phases_ocsort.json")) as f:
            want = json.load(f)
        _corpus = []
        for name in sorted(k for k in want if len(k) == 3):
            cols7 = np.stack([np.asarray(z[f"c{name}_{c}"], np.float64) for c in COLS], axis=1)
            gold = np.asarray([[float.fromhex(v) for v in w[:5]] + [float(w[5])] for w in want[name]["phases"]], np.float64).reshape(-1, 6)
            _corpus.append((name, cols7, gold))
    return _corpus


_ref = {}


def corpus_ref(name, cols7):
    """run(cols7) of a corpus clip with the reference's settings, computed once per clip and shared; callers leave it unchanged"""
    if name not in _ref:
        _ref[name] = run(cols7)
    return _ref[name]
