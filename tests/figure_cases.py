"""TEST INFRASTRUCTURE ONLY: the figures the rep figure's host and GPU tests share (tests/test_figure_host.py runs them through the
sanitized host program, tests/test_gpu_figure.py through the kernels), and the numpy reference of each, computed once."""
import functools

import numpy as np

import figure_ref as FR

# (width, height, scale, thickness): the 32-bit store path (W % 4 == 0) and the byte path, every thickness, scale 2 once
CONFIGS = ((160, 100, 1, 1), (160, 100, 1, 2), (161, 99, 1, 3), (161, 99, 1, 2), (320, 200, 2, 2))
CONC, ECC, HOLD = 0.0, 1.0, 2.0


def _rows(time, x, y, dx, dy):
    n = len(time)
    return np.stack([time, x, y, dx, dy, np.full(n, 0.2), np.full(n, 0.21)], axis=1).astype(np.float64)


def figure_a():
    """40 rows from 0.5 s to 7 s; a phase that starts before t0, two that share a boundary column, a hold, one that ends after t1 and
    whose rep label is clipped by the rectangle's right edge; negative velocities"""
    t = 0.5 + np.arange(40) / 6.0
    y = 0.5 + 0.25 * np.sin(t * 1.7)
    x = 0.45 + 0.02 * np.cos(t * 0.9)
    rows = _rows(t, x, y, np.gradient(x, t), np.gradient(y, t))
    phases = np.array([[0.2, 1.0, 0.6, 0.4, 0.31, ECC], [1.0, 2.0, 0.4, 0.6, 0.455, CONC], [2.0, 3.0, 0.6, 0.4, 0.52, ECC],
                       [3.0, 3.5, 0.4, 0.4, 0.0, HOLD], [5.8, 8.0, 0.4, 0.6, 0.6, CONC]], np.float64)
    return rows, phases


def figure_b():
    """T = 1: a dot per series; a concentric phase of zero duration (ACV 0.00) whose labels the left edge clips"""
    rows = _rows(np.array([2.0]), np.array([0.5]), np.array([0.4]), np.array([0.0]), np.array([-0.3]))
    return rows, np.array([[2.0, 2.0, 0.4, 0.4, 0.3, CONC]], np.float64)


def figure_c():
    return np.zeros((0, 7), np.float64), np.zeros((0, 6), np.float64)


def figure_d():
    """700 rows on a plot about 100 columns wide: many points per column, a two-row velocity spike (a steep segment), a long flat
    run (horizontal segments of equal values), a ROM of 250 m"""
    rng = np.random.default_rng(20240607)
    t = np.arange(700) / 30.0
    y = 0.5 + 0.3 * np.sin(t * 1.1) + rng.normal(0, 0.004, 700)
    x = 0.5 + 0.01 * rng.normal(0, 1, 700)
    x[400:600], y[400:600] = 0.5, 0.62
    dx, dy = np.gradient(x, t), np.gradient(y, t)
    dy[300:302] = 40.0
    dx[400:600], dy[400:600] = 0.0, 0.0
    phases = np.array([[1.0, 2.5, 0.7, 0.3, 250.0, CONC], [2.5, 4.0, 0.3, 0.7, 0.5, ECC], [6.0, 8.2, 0.7, 0.3, 0.62, CONC],
                       [8.2, 8.2, 0.3, 0.3, 0.0, HOLD], [20.0, 23.0, 0.7, 0.3, 0.58, CONC]], np.float64)
    return _rows(t, x, y, dx, dy), phases


@functools.lru_cache(maxsize=None)
def figures():
    return (figure_a(), figure_b(), figure_c(), figure_d())


def params(cfg):
    w, h, s, t = cfg
    return dict(width=w, height=h, scale=s, thickness=t)


@functools.lru_cache(maxsize=None)
def reference(cfg):
    """[(head, points, records, frame)] of the four figures at one configuration; never modified"""
    out = []
    for rows, phases in figures():
        hd, pts, recs = FR.prepare(rows, phases, **params(cfg))
        frame = FR.render_one(hd, pts, recs, **params(cfg))
        for a in (hd, pts, recs, frame):
            a.setflags(write=False)
        out.append((hd, pts, recs, frame))
    return tuple(out)
