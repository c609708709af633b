"""TEST INFRASTRUCTURE ONLY: the figures the curve figure's host and GPU tests share (tests/test_curve_figure_host.py runs them
through the sanitized host program, tests/test_gpu_curve_figure.py through the kernels), and the numpy reference of each, computed once.

Which staging path each configuration takes (tests/curve_figure_ref.py `staged`, asserted by both tests): figure (d) holds 3000 points
in 100 stretches of 30 of one x; each stretch keeps exactly four points through the merge.  At 160 and 161 pixels of width two
neighbouring stretches share a column on most of the 75 columns they span, the merged table holds about 300 points and the tile stages
them in LDS; at 320 pixels every stretch has a column of its own, 400 merged points exceed VBT_CURVE_FIGURE_STAGE_POINTS = 384 and the
tile reads global memory.  Unmerged, the 3000 points would exceed it everywhere.  Figure (g), the six real curves, holds 400 merged
points too: the narrow figures' one tile column sees all of them (global memory), the 320-pixel figure's two see a part each (LDS).
Every other figure renders from LDS."""
import functools
import os

import numpy as np

import curve_figure_ref as CR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (width, height, scale, thickness): the 32-bit store path (W % 4 == 0) and the byte path, three thicknesses, scale 2 once
CONFIGS = ((320, 200, 2, 2), (160, 100, 1, 1), (161, 100, 1, 3))
NAMES = "abcdefgh"


def params(cfg):
    return dict(width=cfg[0], height=cfg[1], scale=cfg[2], thickness=cfg[3])


def sawtooth(n, seed, x_step=3):
    """n points whose x repeats x_step times before it moves on and whose y jumps up and down; two exactly equal neighbours"""
    rng = np.random.default_rng(seed)
    x = np.repeat(np.linspace(0.02, 0.97, (n + x_step - 1) // x_step), x_step)[:n]
    y = 0.5 + 0.35 * np.sin(np.arange(n) * 0.9) * rng.uniform(0.3, 1.0, n)
    xy = np.stack([x, y], axis=1)
    xy[11] = xy[10]
    return xy


def figure_a():
    """three series of about 40 points with repeated columns and a sawtooth in y, exactly equal consecutive points; the second one is
    given decreasing in x; legend lower left; minor grid on y only (the combined PR figure's)"""
    s = [sawtooth(40, 1), sawtooth(41, 2)[::-1].copy(), sawtooth(39, 3, 2)]
    return CR.figure([(s[0], "first, AP50=0.9123", 0), (s[1], "second_whole, AP50=0.8765", 1), (s[2], "third (x2) ~ [ok]", 2)],
                     x_title="Recall", y_title="Precision", corner=CR.LOWER_LEFT, minor_y=100)


def figure_b():
    """a one-point series (a dot) and an n = 0 series (its legend row only); legend lower right; minor grid 100 on both axes"""
    return CR.figure([(np.array([[0.4, 0.6]]), "dot", 3), (np.zeros((0, 2)), "nothing", 4)], x_title="FP Rate", y_title="TP Rate",
                     corner=CR.LOWER_RIGHT, minor_x=100, minor_y=100)


def figure_c():
    """a series whose first points have NaN x (the NO_NEGATIVES shape), one of all NaN, one with a NaN in the middle (an isolated point
    behind it), and points exactly at (1.01, 1.01) and (0, 0)"""
    nan = np.nan
    lead = np.array([[nan, 0.0], [nan, 0.3], [0.2, 0.5], [0.5, 0.55], [0.9, 0.9]])
    hole = np.array([[0.1, 0.2], [0.3, 0.25], [nan, nan], [0.45, 0.8], [0.6, nan], [0.7, 0.3], [0.8, 0.35]])
    corners = np.array([[0.0, 0.0], [0.5, 0.1], [1.01, 1.01]])
    return CR.figure([(lead, "nan first", 5), (np.full((4, 2), nan), "all nan", 6), (hole, "hole", 7), (corners, "corners", 8)],
                     x_title="x", y_title="y", corner=CR.LOWER_RIGHT, minor_x=50, minor_y=50)


def figure_d():
    """one series of 3000 points: 100 values of x in [0.01, 0.6], 30 points each, whose y goes first, down to the stretch's lowest at
    its 8th point, up to its highest at its 20th, and back - so first, lowest, highest and last are four different points"""
    xs = np.linspace(0.01, 0.6, 100)
    j = np.arange(30)
    shape = np.where(j <= 7, -j / 7.0, np.where(j <= 19, -1.0 + 2.0 * (j - 7) / 12.0, 1.0 - 0.7 * (j - 19) / 10.0))
    y = 0.5 + 0.3 * np.sin(np.arange(100) * 0.21)[:, None] + 0.15 * shape[None, :]
    return CR.figure([(np.stack([np.repeat(xs, 30), y.reshape(-1)], axis=1), "3000 points", 9)], x_title="Recall", y_title="Precision",
                     corner=CR.LOWER_LEFT, minor_x=50, minor_y=50)


def figure_e():
    """five annotations on the lower-left side: one whose text leaves the frame (clipped by the left edge), one on the first and one on
    the last point of the series, two on the same point"""
    xy = np.stack([np.linspace(0.0, 1.0, 21), 0.95 - 0.6 * np.linspace(0.0, 1.0, 21) ** 2], axis=1)
    marks = [(0, 0, "0.9876"), (0, 20, "0.0123"), (0, 10, "0.5000"), (0, 10, "0.5001"), (0, 1, "left edge clips")]
    return CR.figure([(xy, "model, AP=0.7000", 1)], marks, x_title="Recall", y_title="Precision", corner=CR.LOWER_LEFT, minor_x=50, minor_y=50)


def figure_f():
    """eight series with 63-byte legend texts: the legend box is wider than a 160-pixel figure and is clipped by the frame"""
    series = []
    for k in range(8):
        x = np.linspace(0.0, 1.0, 12)
        text = (f"series {k} " + "".join(chr(0x21 + (7 * k + i) % 94) for i in range(63)))[:63]
        series.append((np.stack([x, np.clip(x ** (0.3 + 0.2 * k), 0, 1)], axis=1), text, k))
    return CR.figure(series, x_title="FP Rate", y_title="TP Rate", corner=CR.LOWER_RIGHT, minor_x=100, minor_y=100)


@functools.lru_cache(maxsize=None)
def _golden_curves():
    d = np.load(os.path.join(GOLDEN, "eval_curves_ref.npz"))
    return {k: d[k] for k in d.files}


def figure_g():
    """models 0..5 of tests/golden/eval_curves_ref.npz at t0 as the combined PR figure: the real shape of the data"""
    d = _golden_curves()
    names = [str(n) for n in d["model_names"]]
    series = [(np.stack([d[f"m{k}_t0_recall"], d[f"m{k}_t0_precision"]], axis=1), f"{names[k]}, AP50={float(d[f'm{k}_t0_ap']):.4f}"[:63], k)
              for k in range(6)]
    return CR.figure(series, x_title="Recall", y_title="Precision", corner=CR.LOWER_LEFT, minor_y=100)


def figure_h():
    """the same models as the combined ROC figure, with two annotations on the lower-right side"""
    d = _golden_curves()
    names = [str(n) for n in d["model_names"]]
    series = [(np.stack([d[f"m{k}_t0_fpr"], d[f"m{k}_t0_tpr"]], axis=1), f"{names[k]}, AUC={float(d[f'm{k}_t0_auc']):.4f}"[:63], k) for k in range(6)]
    marks = [(2, 5, "0.8000"), (2, len(series[2][0]) - 2, "0.2000")]
    return CR.figure(series, marks, x_title="FP Rate", y_title="TP Rate", corner=CR.LOWER_RIGHT, minor_x=100, minor_y=100)


@functools.lru_cache(maxsize=None)
def figures():
    return (figure_a(), figure_b(), figure_c(), figure_d(), figure_e(), figure_f(), figure_g(), figure_h())


MAX = dict(max_figures=8, max_series=8, max_points=3000, max_marks=5)


@functools.lru_cache(maxsize=None)
def reference(cfg):
    """per figure (counts, merged points, records, frame of the UNMERGED polyline) at one configuration"""
    p = params(cfg)
    return tuple(CR.prepare(f, **p) + (CR.render_one(f, **p),) for f in figures())
