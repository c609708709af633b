"""Trajectory validation against Kinovea / Qualisys exports.

Mirrors the reference's accuracy study:
  reference kinovea.py:73-172   Kinovea text export vs a tracked DataFrame
  reference qualysis.py:79-187  Qualisys .tsv export (marker "Osa L", X and Z) vs a tracked DataFrame
Steps: parse the export; smooth the tracked rows (window means on the GPU, `vbt_window_means`); convert normalised
image coordinates to metres with the plate diameter; shift both axes so the means agree; resample both trajectories
linearly onto a 30 Hz grid over the common time span; report MSE and Pearson r per axis.

Two ways to the numbers.  `validate_pair` is one pair at a time: the window means on the device, the rest in numpy.  `Validation`
(vbt_validation, include/vbt_hip.h "Validation figure") and `validate_many` take a corpus of pairs through one upload and one
prepare launch per batch, compute all of the above on the device - its sums in a fixed order of their own, so the last bits differ
from numpy's - and render the reference's figure of every pair (two stacked panels, X and Y over time, ground truth against
tracker) into RGB24 frames that the JPEG encoder takes from device memory.  Not offered: a display (`--show_fig`), the LaTeX
table, p-values (the reference drops them before it prints).
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np

from . import _lib
from .figure import FigureHandle, write_frames

KINDS = {"kinovea": 0, "qualisys": 1}
VALIDATION_PARAMS = ("width", "height", "scale", "thickness", "max_pairs", "max_rows", "max_ref_rows", "max_grid")
STATS = ("mse_x", "mse_y", "r_x", "r_y", "n", "t_min", "t_max", "flags")


def read_kinovea(path):
    """Kinovea 'trajectory data export': `#` comment lines, then `time x y` separated by blanks with decimal commas in
    x / y (centimetres).  Returns [N,3] float64 time [s], x [m], y [m]   (reference kinovea.py:73-88)."""
    rows = []
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            p = line.split(" ")
            rows.append((float(p[0]), float(p[1].replace(",", ".")) / 100.0, float(p[2].replace(",", ".")) / 100.0))
    return np.asarray(rows, dtype=np.float64).reshape(-1, 3)


def read_qualisys(path, marker="Osa L"):
    """Qualisys .tsv: 11 header lines, a tab separated column-name line, then frames.  x = -X/1000, y = Z/1000 of the
    marker [m]   (reference qualysis.py:79-108).  Returns [N,3] float64 time, x, y."""
    with open(path) as f:
        lines = f.read().splitlines()
    names = lines[11].rstrip("\t").split("\t")
    it, ix, iz = names.index("Time"), names.index(f"{marker} X"), names.index(f"{marker} Z")
    out = []
    for line in lines[12:]:
        if not line.strip():
            continue
        p = line.split("\t")
        out.append((float(p[it]), -float(p[ix]) / 1000.0, float(p[iz]) / 1000.0))
    return np.asarray(out, dtype=np.float64).reshape(-1, 3)


def window_means(table, windows, device=0):
    """pandas rolling(window, min_periods=1).mean() (window > 0) / expanding().mean() (0) / copy (< 0) per column,
    computed on the GPU."""
    table = np.ascontiguousarray(table, dtype=np.float64)
    T, nc = table.shape
    w = np.ascontiguousarray(windows, dtype=np.int32)
    if w.shape != (nc,):
        raise ValueError("one window per column expected")
    out = np.empty_like(table)
    _lib.check(_lib.lib().vbt_window_means(table.ctypes.data, T, nc, w.ctypes.data, out.ctypes.data, device))
    return out


def metric_trajectory(rows, ref, plate_diameter=0.45, source="kinovea", device=0):
    """rows [T,5] = time, x, y, norm_plate_height, norm_plate_width of ONE track (sorted by time) -> [T,3]
    time, x, y in metres, aligned to `ref` ([N,3] time, x, y).
    kinovea: expanding mean of the plate size, rolling(5) of x and y   (reference kinovea.py:99-116)
    qualisys: rolling(30) of the plate size, raw x and y               (reference qualysis.py:113-131)"""
    rows = np.asarray(rows, dtype=np.float64)
    if source == "kinovea":
        sm = window_means(rows, [-1, 5, 5, 0, 0], device)
    elif source == "qualisys":
        sm = window_means(rows, [-1, -1, -1, 30, 30], device)
    else:
        raise ValueError("source must be 'kinovea' or 'qualisys'")
    x = sm[:, 1] * plate_diameter / sm[:, 4]
    y = -sm[:, 2] * plate_diameter / sm[:, 3]             # image y grows downwards
    y = y + (_mean(ref[:, 2]) - _mean(y))
    x = x + (_mean(ref[:, 1]) - _mean(x))
    return np.stack([rows[:, 0], x, y], axis=1)


def _mean(v):
    # pandas Series.mean(): bottleneck-free nanmean = pairwise np.sum / count
    return np.sum(v) / v.size


def _interp_linear(t, v, ts):
    """scipy.interpolate.interp1d(kind='linear') arithmetic: slope * (t_new - t_lo) + v_lo on the bracketing pair."""
    order = np.argsort(t, kind="mergesort")
    t, v = t[order], v[order]
    if ts.size and (ts.min() < t[0] or ts.max() > t[-1]):
        raise ValueError("A value in x_new is outside the interpolation range.")
    hi = np.clip(np.searchsorted(t, ts), 1, len(t) - 1)
    lo = hi - 1
    slope = (v[hi] - v[lo]) / (t[hi] - t[lo])
    return slope * (ts - t[lo]) + v[lo]


def _pearson(a, b):
    """scipy.stats.pearsonr statistic (normalise the centred vectors, then dot)."""
    am = a - a.mean()
    bm = b - b.mean()
    na, nb = np.linalg.norm(am), np.linalg.norm(bm)
    return float(max(min(np.dot(am / na, bm / nb), 1.0), -1.0))


def compare(ref, traj, rate=30):
    """-> dict(mse_x, mse_y, r_x, r_y, n) on a `rate` Hz grid over the common time span
    (reference kinovea.py:151-172, qualysis.py:166-187; the grid has int(t_max * 30) points)."""
    t_max = min(ref[:, 0].max(), traj[:, 0].max())
    t_min = max(ref[:, 0].min(), traj[:, 0].min())
    ts = np.linspace(t_min, t_max, int(t_max * rate))
    xr, xm = _interp_linear(ref[:, 0], ref[:, 1], ts), _interp_linear(traj[:, 0], traj[:, 1], ts)
    yr, ym = _interp_linear(ref[:, 0], ref[:, 2], ts), _interp_linear(traj[:, 0], traj[:, 2], ts)
    return {"mse_x": float(np.mean((xr - xm) ** 2)), "mse_y": float(np.mean((yr - ym) ** 2)),
            "r_x": _pearson(xr, xm), "r_y": _pearson(yr, ym), "n": int(ts.size)}


def validate_pair(ref, rows, plate_diameter=0.45, source="kinovea", device=0):
    if len(rows) < 2 or not math.isfinite(float(np.sum(rows))):
        raise ValueError("tracked rows are empty or not finite")
    return compare(ref, metric_trajectory(rows, ref, plate_diameter, source, device))


def default_params():
    p = _lib.ValidationParams()
    _lib.lib().vbt_validation_default_params(ctypes.byref(p))
    return {k: getattr(p, k) for k in VALIDATION_PARAMS}


class Validation(FigureHandle):
    """vbt_validation (include/vbt_hip.h): one figure size, scale and curve thickness; up to max_pairs pairs per set.
    params: width=1280, height=640, scale=2, thickness=2, max_pairs=64, max_rows=4096, max_ref_rows=4096, max_grid=4096."""
    API, Params, PARAMS = "vbt_validation", _lib.ValidationParams, VALIDATION_PARAMS

    def __init__(self, device=0, **params):
        super().__init__(device, **params)
        self.params["max_figures"] = self.params["max_pairs"]                          # (figure.write_frames sizes its encoder by it)

    def set(self, pairs, source="kinovea", plate_diameter=0.45, rate=30.0, stream=None):
        """pairs: [(ref, rows), ...] - ref float64 [N, 3] time, x, y in metres; rows float64 [T, 5] time, x, y, norm_plate_height,
        norm_plate_width of one track sorted by time; source: 'kinovea' or 'qualisys', for all pairs or one per pair.  One upload, one prepare launch."""
        sources = [source] * len(pairs) if isinstance(source, str) else list(source)
        if len(sources) != len(pairs) or any(s not in KINDS for s in sources):
            raise ValueError("source must be 'kinovea' or 'qualisys', once or per pair")
        kinds = np.array([KINDS[s] for s in sources], np.int32)
        refs = [np.ascontiguousarray(np.asarray(p[0], np.float64).reshape(-1, 3)) for p in pairs]
        rows = [np.ascontiguousarray(np.asarray(p[1], np.float64).reshape(-1, 5)) for p in pairs]
        rc = np.array([len(r) for r in refs], np.int32)
        kc = np.array([len(r) for r in rows], np.int32)
        allr = np.ascontiguousarray(np.concatenate(refs)) if refs else np.zeros((0, 3))
        allk = np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros((0, 5))
        _lib.check(_lib.lib().vbt_validation_set(self._h, len(refs), kinds.ctypes.data, float(plate_diameter), float(rate), allr.ctypes.data, rc.ctypes.data,
                                                 allk.ctypes.data, kc.ctypes.data, stream))
        self.n = len(refs)

    def stats(self):
        """float64 [n, 8]: mse_x, mse_y, r_x, r_y, n, t_min, t_max, flags per pair, in one copy"""
        out = np.zeros((self.n, len(STATS)), np.float64)
        _lib.check(_lib.lib().vbt_validation_stats(self._h, out.ctypes.data, self.n))
        return out

    def table(self, pair):
        """(head float64 [6] = time lo, hi, X lo, hi, Y lo, hi; aligned trajectory float64 [T, 3]; grid float64 [n, 5] = ts, ref x, tracker x,
        ref y, tracker y; counts int32 [4]; merged points int32 [sum, 3]; records int32 [n, 28]) as prepared"""
        L = _lib.lib()
        head, counts = np.zeros(6, np.float64), np.zeros(4, np.int32)
        n = [ctypes.c_int() for _ in range(4)]
        rc = L.vbt_validation_table(self._h, int(pair), head.ctypes.data, None, 0, ctypes.byref(n[0]), None, 0, ctypes.byref(n[1]), counts.ctypes.data,
                                    None, 0, ctypes.byref(n[2]), None, 0, ctypes.byref(n[3]))
        if rc != -4:
            _lib.check(rc)
        traj, grid = np.zeros((n[0].value, 3), np.float64), np.zeros((n[1].value, 5), np.float64)
        pts, recs = np.zeros((n[2].value, 3), np.int32), np.zeros((n[3].value, 28), np.int32)
        _lib.check(L.vbt_validation_table(self._h, int(pair), head.ctypes.data, traj.ctypes.data, len(traj), ctypes.byref(n[0]), grid.ctypes.data, len(grid),
                                          ctypes.byref(n[1]), counts.ctypes.data, pts.ctypes.data, len(pts), ctypes.byref(n[2]), recs.ctypes.data, len(recs),
                                          ctypes.byref(n[3])))
        return head, traj, grid, counts, pts, recs


def grid_size(ref, rows, rate=30.0):
    """the number of grid points of a pair: int(t_max * rate)"""
    return int(min(ref[-1, 0], rows[-1, 0]) * rate)


def validate_many(pairs, source, plate_diameter=0.45, fig_dir=None, fig_format="jpg", quality=90, device=0, **params):
    """A corpus of pairs [(ref, rows) or (ref, rows, name), ...] in batches of max_pairs: per batch one set (one upload, one prepare
    launch), one read-back of the numbers and, with fig_dir, one render, one encode and one read-back of FIG_DIR/{name}.jpg|ppm
    (name: the pair's third element, else pairNNN).  Returns (the list of the dicts validate_pair returns, the paths written)."""
    if fig_format not in ("jpg", "ppm"):
        raise ValueError(f"fig_format {fig_format!r}: jpg or ppm")
    if source not in KINDS:
        raise ValueError("source must be 'kinovea' or 'qualisys'")
    items = [(np.asarray(p[0], np.float64).reshape(-1, 3), np.asarray(p[1], np.float64).reshape(-1, 5), p[2] if len(p) > 2 else f"pair{i:03d}")
             for i, p in enumerate(pairs)]
    if not items:
        return [], []
    if fig_dir is not None:
        os.makedirs(fig_dir, exist_ok=True)
    base = dict(default_params(), **params)
    base["max_rows"] = max(base["max_rows"], max(len(k) for _, k, _ in items))
    base["max_ref_rows"] = max(base["max_ref_rows"], max(len(r) for r, _, _ in items))
    base["max_grid"] = max([base["max_grid"]] + [grid_size(r, k) for r, k, _ in items if len(r) and len(k)])
    base["max_pairs"] = min(base["max_pairs"], len(items))
    v = Validation(device, **base)
    results, written = [], []
    for b0 in range(0, len(items), base["max_pairs"]):
        batch = items[b0:b0 + base["max_pairs"]]
        v.set([(r, k) for r, k, _ in batch], source, plate_diameter)
        results += [{"mse_x": float(s[0]), "mse_y": float(s[1]), "r_x": float(s[2]), "r_y": float(s[3]), "n": int(s[4])} for s in v.stats()]
        if fig_dir is not None:
            written += write_frames(v, [os.path.join(fig_dir, f"{name}.{fig_format}") for _, _, name in batch], fig_format, quality)
    return results, written
