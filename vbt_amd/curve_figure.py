"""Curve figure: the figures of the reference's eval.py without a plotting library (include/vbt_hip.h, "Curve figure").  `CurveFigure`
is vbt_curve_figure: N figures - each some series of (x, y) points with a legend, a grid and annotations - rendered on the GPU into N
RGB24 frames that stay in device memory.  evaluate.plot_precision_recall / plot_roc build the reference's figures from it.  torch-free."""
import ctypes

import numpy as np

from . import _lib
from .figure import FigureHandle

PARAMS = ("width", "height", "scale", "thickness", "max_figures", "max_series", "max_points", "max_marks")
RECORD = ("kind", "x0", "y0", "x1", "y1", "ox", "oy", "value", "aux", "n", "pad0", "pad1") + tuple(f"chars{k}" for k in range(16))
LOWER_LEFT, LOWER_RIGHT = 0, 1
PALETTE_SIZE = 10


def default_params():
    p = _lib.CurveFigureParams()
    _lib.lib().vbt_curve_figure_default_params(ctypes.byref(p))
    return {k: getattr(p, k) for k in PARAMS}


def figure(series=(), marks=(), x_title="", y_title="", corner=LOWER_LEFT, minor_x=0, minor_y=0):
    """One figure as `CurveFigure.set` takes it: series = [(xy [n, 2], legend text, palette index 0..9), ...]; marks = [(series, point,
    text), ...]; the axis titles; the legend's corner (LOWER_LEFT / LOWER_RIGHT); the minor grid steps in thousandths (0: none)."""
    return dict(series=list(series), marks=list(marks), x_title=x_title, y_title=y_title, corner=corner, minor_x=minor_x, minor_y=minor_y)


def _bytes(text, what):
    try:
        return str(text).encode("ascii")
    except UnicodeEncodeError:
        raise ValueError(f"{what} {text!r}: printable ASCII only") from None


def pack(figures):
    """(descs, series, xy float64 [P, 2], marks) - the arrays of vbt_curve_figure_set.  A text that is too long for its field is a
    ValueError here; everything else is the library's to refuse."""
    ns, nm = sum(len(f["series"]) for f in figures), sum(len(f["marks"]) for f in figures)
    descs = (_lib.CurveFigureDesc * max(len(figures), 1))()
    series = (_lib.CurveSeries * max(ns, 1))()
    marks = (_lib.CurveMark * max(nm, 1))()
    xy, s, m = [], 0, 0
    for i, f in enumerate(figures):
        d = descs[i]
        d.n_series, d.n_marks, d.legend_corner, d.minor_x, d.minor_y = len(f["series"]), len(f["marks"]), int(f["corner"]), int(f["minor_x"]), int(f["minor_y"])
        for key, field in (("x_title", "x_title"), ("y_title", "y_title")):
            b = _bytes(f[key], key)
            if len(b) > 31:
                raise ValueError(f"figure {i}: {key} of {len(b)} bytes, at most 31")
            setattr(d, field, b)
        for k, (pts, text, colour) in enumerate(f["series"]):
            pts = np.ascontiguousarray(np.asarray(pts, np.float64).reshape(-1, 2))
            b = _bytes(text, "legend text")
            if len(b) > 63:
                raise ValueError(f"figure {i}, series {k}: legend text of {len(b)} bytes, at most 63")
            series[s].n_points, series[s].colour, series[s].text = len(pts), int(colour), b
            xy.append(pts)
            s += 1
        for k, (sr, pt, text) in enumerate(f["marks"]):
            b = _bytes(text, "mark text")
            if len(b) > 15:
                raise ValueError(f"figure {i}, mark {k}: text of {len(b)} bytes, at most 15")
            marks[m].series, marks[m].point, marks[m].text = int(sr), int(pt), b
            m += 1
    allxy = np.ascontiguousarray(np.concatenate(xy)) if xy else np.zeros((0, 2), np.float64)
    return descs, series, allxy, marks


class CurveFigure(FigureHandle):
    """vbt_curve_figure (include/vbt_hip.h): one figure size, scale and curve thickness; up to max_figures figures per set.
    params: width=1120, height=640, scale=2, thickness=2, max_figures=16, max_series=8, max_points=131072, max_marks=8."""
    API, Params, PARAMS = "vbt_curve_figure", _lib.CurveFigureParams, PARAMS

    def set(self, figures, stream=None):
        """figures: a list of `figure(...)` dicts.  One upload, one prepare launch."""
        figures = list(figures)
        descs, series, xy, marks = pack(figures)
        _lib.check(_lib.lib().vbt_curve_figure_set(self._h, len(figures), ctypes.addressof(descs), ctypes.addressof(series), xy.ctypes.data,
                                                   ctypes.addressof(marks), stream))
        self.n = len(figures)

    def table(self, fig):
        """(counts int32 [K] = merged points per series; points int32 [sum, 3] = column, row, join; records int32 [n, 28]) as prepared"""
        L = _lib.lib()
        ns, npts, nrec = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        rc = L.vbt_curve_figure_table(self._h, int(fig), None, 0, ctypes.byref(ns), None, 0, ctypes.byref(npts), None, 0, ctypes.byref(nrec))
        if rc != -4:
            _lib.check(rc)
        counts = np.zeros(ns.value, np.int32)
        pts = np.zeros((npts.value, 3), np.int32)
        recs = np.zeros((nrec.value, 28), np.int32)
        _lib.check(L.vbt_curve_figure_table(self._h, int(fig), counts.ctypes.data, len(counts), ctypes.byref(ns), pts.ctypes.data, len(pts),
                                            ctypes.byref(npts), recs.ctypes.data, len(recs), ctypes.byref(nrec)))
        return counts, pts, recs
