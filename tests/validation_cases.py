"""TEST INFRASTRUCTURE ONLY: the pairs and handle configurations of the validation figure's tests (tests/test_validation_host.py,
tests/test_gpu_validation.py), each small and each there because something can go wrong at that shape:
  a  kinovea, 40 tracked rows, 55 reference rows at another rate that start later and end earlier: t_min / t_max from different series,
     brackets at both grid ends, the dX < dY widening of the X panel
  b  qualisys, 12 tracked rows, 300 reference rows: window 30 longer than the series, the dX > dY widening of the Y panel
  c  2 rows each at times 0 and 0.1: n = 3, hi clipped to 1, a single segment
  d  qualisys, 330 tracked rows over 11 s, 700 reference rows: a grid of more than 256 points and no multiple of 256 (the partial sums
     take a second round); many points per column, so the run merge drops points and a tile holds more merged points than are staged
     (the global-memory path, at every configuration; every other pair is staged); dX <= dY, so qualisys widens the X panel
  e  x constant in both series: the d == 0 range, mse_x == 0, r_x NaN with its flag (no other pair carries a flag)
The plate diameter is 0.5 so that (e)'s metric x is the same double in every row."""
import numpy as np

import validation_ref as VR

NAMES = ("a", "b", "c", "d", "e")
KINDS = ("kinovea", "qualisys", "kinovea", "qualisys", "kinovea")
PLATE, RATE = 0.5, 30.0
# width, height, scale, thickness: 32-bit stores; an odd width (byte stores) with thickness 2; scale 2 (two tiles across)
CONFIGS = ((160, 100, 1, 1), (161, 101, 1, 2), (320, 200, 2, 2))
MAX = dict(max_pairs=5, max_rows=330, max_ref_rows=700, max_grid=329)
_cache = {}


def params(cfg):
    return dict(width=cfg[0], height=cfg[1], scale=cfg[2], thickness=cfg[3])


def _rows(t, x, y, h, w):
    return np.stack([t, x, y, h, w], axis=1).astype(np.float64)


def pairs():
    if "pairs" in _cache:
        return _cache["pairs"]
    rng = np.random.default_rng(2024)
    out = []
    # a
    t = np.arange(40) / 10.0
    rows = _rows(t, 0.5 + 0.008 * np.sin(2 * t) + rng.normal(0, 0.001, 40), 0.5 + 0.2 * np.cos(1.5 * t), 0.21 + rng.normal(0, 0.002, 40),
                 0.2 + rng.normal(0, 0.002, 40))
    tr = 0.35 + 0.06 * np.arange(55)
    out.append((np.stack([tr, 0.3 + 0.02 * np.sin(2 * tr), 1.0 - 0.5 * np.cos(1.5 * tr)], axis=1), rows))
    # b
    t = np.arange(12) / 10.0
    rows = _rows(t, 0.3 + 0.25 * t + rng.normal(0, 0.002, 12), 0.5 + 0.01 * np.sin(5 * t), 0.2 + rng.normal(0, 0.003, 12), 0.21 + rng.normal(0, 0.003, 12))
    tr = 0.004 * np.arange(300)
    out.append((np.stack([tr, -0.4 + 0.6 * tr + rng.normal(0, 0.001, 300), 0.9 - 0.025 * np.sin(5 * tr)], axis=1), rows))
    # c
    out.append((np.array([[0.0, 0.1, 0.2], [0.1, 0.15, 0.1]]), _rows(np.array([0.0, 0.1]), np.array([0.4, 0.42]), np.array([0.5, 0.55]), np.array([0.2, 0.21]),
                                                                   np.array([0.2, 0.2]))))
    # d
    t = np.arange(330) / 30.0
    rows = _rows(t, 0.5 + 0.05 * np.sin(3 * t) + rng.normal(0, 0.004, 330), 0.5 + 0.15 * np.cos(2 * t) + rng.normal(0, 0.004, 330),
                 0.2 + rng.normal(0, 0.002, 330), 0.2 + rng.normal(0, 0.002, 330))
    tr = t[-1] * np.arange(700) / 699.0
    out.append((np.stack([tr, 0.125 * np.sin(3 * tr) + rng.normal(0, 0.01, 700), 2.0 - 0.375 * np.cos(2 * tr) + rng.normal(0, 0.01, 700)], axis=1), rows))
    # e
    t = np.arange(20) / 15.0
    rows = _rows(t, np.full(20, 0.5), 0.4 + 0.1 * np.sin(4 * t), 0.2 + rng.normal(0, 0.002, 20), np.full(20, 0.25))
    tr = 0.05 * np.arange(25)
    out.append((np.stack([tr, np.full(25, 2.0), 0.7 - 0.25 * np.sin(4 * tr)], axis=1), rows))
    _cache["pairs"] = [(np.ascontiguousarray(r, np.float64), np.ascontiguousarray(k, np.float64)) for r, k in out]
    return _cache["pairs"]


def reference(cfg):
    """per pair (prepare()'s dict, the frame uint8 [H, W, 3]) from the numpy statement, computed once per configuration"""
    if cfg not in _cache:
        p = params(cfg)
        preps = [VR.prepare(r, k, kind, PLATE, RATE, **p) for (r, k), kind in zip(pairs(), KINDS)]
        _cache[cfg] = [(q, VR.render_one(q, **p)) for q in preps]
    return _cache[cfg]
