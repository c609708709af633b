"""`VelocityTracker` / `Phase`: the rep analyser of the reference, computed on the GPU.

Mirrors reference VelocityTracker.py:15-230 and Phase.py:6-40 as used by plot.py:33-47:
  VelocityTracker(plate_diameter, diff_threshold=0.6, min_distance=0.1)
  .process_measurements(time, x, y, dx, dy, norm_plate_height, norm_plate_width)
  .end_processing()
  .phases -> objects with time_start,time_end,y_start,y_end,rom,type,y_diff,duration
The state machine is strictly sequential per track, so samples are buffered on the host and the
scan runs as one device launch (vbt_analyze) when `.phases` is read / `end_processing()` is called.
"""
import collections
import ctypes

import numpy as np

from . import _lib


class Phase:
    CONCENTRIC = 0      # reference Phase.py:12-14
    ECCENTRIC = 1
    HOLD = 2

    def __init__(self, time_start, time_end, y_start, y_end, rom, phase_type):
        self.time_start, self.time_end = time_start, time_end
        self.y_start, self.y_end = y_start, y_end
        self.type = phase_type
        self.rom = rom

    @property
    def y_diff(self):
        return abs(self.y_start - self.y_end)

    @property
    def duration(self):
        return self.time_end - self.time_start

    def __str__(self):
        name = {0: "concentric", 1: "eccentric"}.get(self.type, "hold")
        return f"{name}, t_start: {self.time_start}, t_end: {self.time_end}, y_start: {self.y_start}, y_end: {self.y_end}"


# columns of a metrics array [P, 8] (VBT_RM_*, include/vbt_hip.h): peak velocity and its time stamp, vertical / horizontal travel, peak
# vertical velocity, mean velocity (= the reference's ACV), largest sideways excursion from the start, steps of the path
RM_PV, RM_T_PV, RM_ROM_Y, RM_ROM_X, RM_PV_Y, RM_MV, RM_X_DEV, RM_N_STEPS = range(8)

SetReport = collections.namedtuple("SetReport", "n_reps best_rep stop_rep best_mv last_mv mean_mv mean_pv max_pv loss_last_pct concentric_s "
                                                "eccentric_s mean_x_dev loss_pct")


def _phases6(phases):
    if isinstance(phases, np.ndarray):
        return np.ascontiguousarray(phases, np.float64).reshape(-1, 6)
    return np.asarray([[p.time_start, p.time_end, p.y_start, p.y_end, p.rom, float(p.type)] for p in phases], np.float64).reshape(-1, 6)


def set_report(phases, metrics, stop_loss_pct=0.0):
    """The report of a set (vbt_set_summary; host only): phases = list[Phase] or float64 [P,6], metrics = float64 [P,8] in the same
    order.  The concentric phases are the reps; loss_pct[k] = 100 * (1 - mv_k / best mv so far); stop_rep = the first rep (1-based)
    whose loss reaches stop_loss_pct, 0 when none does or no threshold is given."""
    ph = _phases6(phases)
    m = np.ascontiguousarray(metrics, np.float64).reshape(-1, 8)
    if len(m) != len(ph):
        raise ValueError(f"{len(ph)} phases but {len(m)} metrics records")
    rep, loss = _lib.SetReport(), np.zeros(max(1, len(ph)), np.float64)
    _lib.check(_lib.lib().vbt_set_summary(ph.ctypes.data, m.ctypes.data, len(ph), float(stop_loss_pct), ctypes.byref(rep), loss.ctypes.data, len(loss)))
    return SetReport(rep.n_reps, rep.best_rep, rep.stop_rep, rep.best_mv, rep.last_mv, rep.mean_mv, rep.mean_pv, rep.max_pv, rep.loss_last_pct,
                     rep.concentric_s, rep.eccentric_s, rep.mean_x_dev, loss[:rep.n_reps].copy())


def analyze_rows(rows7, plate_diameter=0.45, diff_threshold=0.6, min_distance=0.1, preprocess=True, flush=True, device=0, metrics=False):
    """rows7 [T,7] = time,x,y,dx,dy,h,w of one track -> list[Phase].  preprocess=True applies the
    rolling(5)/expanding means of reference plot.py:90-95 on the device first (analyze_df input).
    metrics=True: (list[Phase], float64 [P,8] rep metrics, columns RM_*), formed in the same scan."""
    rows7 = np.ascontiguousarray(rows7, np.float64).reshape(-1, 7)
    ph = np.empty((512, 6), np.float64)
    n = ctypes.c_int()
    if metrics:
        m = np.empty((512, 8), np.float64)
        _lib.check(_lib.lib().vbt_analyze_metrics(rows7.ctypes.data if len(rows7) else None, len(rows7), int(preprocess), int(flush),
                                                  float(plate_diameter), float(diff_threshold), float(min_distance), ph.ctypes.data,
                                                  m.ctypes.data, 512, ctypes.byref(n), device))
        return [Phase(r[0], r[1], r[2], r[3], r[4], int(r[5])) for r in ph[:n.value]], m[:n.value].copy()
    _lib.check(_lib.lib().vbt_analyze(rows7.ctypes.data if len(rows7) else None, len(rows7), int(preprocess), int(flush),
                                      float(plate_diameter), float(diff_threshold), float(min_distance), ph.ctypes.data, 512,
                                      ctypes.byref(n), device))
    return [Phase(r[0], r[1], r[2], r[3], r[4], int(r[5])) for r in ph[:n.value]]


class VelocityTracker:
    def __init__(self, plate_diameter, diff_threshold=0.6, min_distance=0.1, device=0):
        self.plate_diameter = plate_diameter
        self.min_distance = min_distance
        self.diff_threshold = diff_threshold
        self.device = device
        self._rows = []
        self._flushed = False
        self._cache = None
        self._metrics = None

    def process_measurements(self, time, x, y, dx, dy, norm_plate_height, norm_plate_width):
        if self._flushed:
            raise RuntimeError("process_measurements after end_processing")
        self._rows.append((time, x, y, dx, dy, norm_plate_height, norm_plate_width))
        self._cache = None

    def end_processing(self):
        self._flushed = True
        self._cache = None

    @property
    def phases(self):
        if self._cache is None:
            self._cache = analyze_rows(np.asarray(self._rows, np.float64).reshape(-1, 7), self.plate_diameter, self.diff_threshold,
                                       self.min_distance, preprocess=False, flush=self._flushed, device=self.device)
        return self._cache

    @property
    def rep_metrics(self):
        """float64 [P,8] (columns RM_*) of .phases, after end_processing()"""
        if not self._flushed:
            raise RuntimeError("rep_metrics before end_processing")
        if self._metrics is None:
            self._cache, self._metrics = analyze_rows(np.asarray(self._rows, np.float64).reshape(-1, 7), self.plate_diameter, self.diff_threshold,
                                                      self.min_distance, preprocess=False, flush=True, device=self.device, metrics=True)
        return self._metrics


def analyze_df(df, plate_diameter):
    """reference plot.py:33-47: df has columns time,x,y,dx,dy,norm_plate_height,norm_plate_width (already preprocessed)."""
    cols = ["time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width"]
    return analyze_rows(np.stack([np.asarray(df[c], np.float64) for c in cols], axis=1), plate_diameter, preprocess=False)
