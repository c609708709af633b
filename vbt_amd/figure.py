"""Rep figure: the reference's plot.py without a plotting library (include/vbt_hip.h, "Rep figure").  `Figure` is vbt_figure: N tracks,
each given as rows and phases, rendered on the GPU into N RGB24 frames that stay in device memory; `plot` has the reference's call
shape (plot.py:73) and `plot_many` takes a corpus of DataFrames through one set / render / encode per batch of figures.  torch-free."""
import ctypes
import os

import numpy as np

from . import _lib
from .mem import DeviceBuffer
from .overlay import phases6

COLUMNS = ("time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width")
PARAMS = ("width", "height", "scale", "thickness", "max_figures", "max_rows", "max_phases")
RECORD = ("kind", "x0", "y0", "x1", "y1", "ox", "oy", "chars0", "chars1", "chars2", "value", "aux")
KIND_SPAN, KIND_LINE, KIND_SWATCH, KIND_TEXT = 0, 1, 2, 3
FIXED_RECORDS = 384


def default_params():
    p = _lib.FigureParams()
    _lib.lib().vbt_figure_default_params(ctypes.byref(p))
    return {k: getattr(p, k) for k in PARAMS}


class FigureHandle:
    """What the figure handles of include/vbt_hip.h share: create and destroy, render into device memory, the handle's own frames.
    A subclass names its entry points' prefix (API), its params struct (Params) and its fields (PARAMS), and has `set` and `table`."""
    API, Params, PARAMS = None, None, ()

    def __init__(self, device=0, **params):
        L = _lib.lib()
        prm = self.Params()
        getattr(L, self.API + "_default_params")(ctypes.byref(prm))
        for k, v in params.items():
            if k not in self.PARAMS:
                raise TypeError(f"{type(self).__name__}: unknown parameter {k!r}")
            setattr(prm, k, int(v))
        self.params = {k: getattr(prm, k) for k in self.PARAMS}
        self.W, self.H, self.device = prm.width, prm.height, int(device)
        self.frame_bytes = self.W * self.H * 3
        h = ctypes.c_void_p()
        _lib.check(getattr(L, self.API + "_create")(self.device, ctypes.byref(prm), ctypes.byref(h)))
        self._h = h
        self.n = 0
        self._buf = None
        self._enc = None                                                               # (quality, mjpeg.Encoder) of write_frames

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and getattr(_lib, "_lib", None) is not None:
            getattr(_lib._lib, self.API + "_destroy")(h)

    def render(self, frames_ptr, fig0=0, n=None, stream=None):
        """figures fig0 .. fig0 + n - 1 into n contiguous RGB24 frames at device pointer `frames_ptr`; enqueue only, on `stream`"""
        n = self.n - fig0 if n is None else n
        _lib.check(getattr(_lib.lib(), self.API + "_render")(self._h, int(frames_ptr), int(fig0), int(n), stream))

    def device_frames(self, stream=None):
        """all figures rendered into the handle's own device buffer; returns its device pointer (enqueue only)"""
        need = max(self.n, 1) * self.frame_bytes
        if self._buf is None or self._buf.nbytes < need:
            self._buf = DeviceBuffer(need, self.device)
        if self.n:
            self.render(self._buf.ptr, 0, self.n, stream)
        return self._buf.ptr

    def frames(self, stream=None):
        """uint8 [n, H, W, 3]: every figure rendered and read back in one copy"""
        self.device_frames(stream)
        _lib.check(_lib.lib().vbt_stream_synchronize(stream))
        return self._buf.to_host((self.n, self.H, self.W, 3), np.uint8)


class Figure(FigureHandle):
    """vbt_figure (include/vbt_hip.h): one figure size, scale and curve thickness; up to max_figures figures per set.
    params: width=1280, height=800, scale=2, thickness=2, max_figures=64, max_rows=16384, max_phases=512."""
    API, Params, PARAMS = "vbt_figure", _lib.FigureParams, PARAMS

    def set(self, figures, stream=None):
        """figures: [(rows, phases), ...] - rows float64 [T, 7] (time, x, y, dx, dy, norm_plate_height, norm_plate_width) of one id
        sorted by time, phases float64 [P, 6] or a list of velocity.Phase.  One upload, one prepare launch."""
        rows = [np.ascontiguousarray(np.asarray(r, np.float64).reshape(-1, 7)) for r, _ in figures]
        phs = [phases6(p) for _, p in figures]
        rc = np.array([len(r) for r in rows], np.int32)
        pc = np.array([len(p) for p in phs], np.int32)
        allr = np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros((0, 7))
        allp = np.ascontiguousarray(np.concatenate(phs)) if phs else np.zeros((0, 6))
        _lib.check(_lib.lib().vbt_figure_set(self._h, len(rows), allr.ctypes.data, rc.ctypes.data, allp.ctypes.data, pc.ctypes.data, stream))
        self.n = len(rows)

    def table(self, fig):
        """(head float64 [6] = t0, t1, position lo, hi, velocity lo, hi; points int32 [T, 5]; records int32 [n, 12]) as prepared"""
        L = _lib.lib()
        head = np.zeros(6, np.float64)
        npts, nrec = ctypes.c_int(), ctypes.c_int()
        rc = L.vbt_figure_table(self._h, int(fig), head.ctypes.data, None, 0, ctypes.byref(npts), None, 0, ctypes.byref(nrec))
        if rc != -4:
            _lib.check(rc)
        pts = np.zeros((npts.value, 5), np.int32)
        recs = np.zeros((nrec.value, 12), np.int32)
        _lib.check(L.vbt_figure_table(self._h, int(fig), head.ctypes.data, pts.ctypes.data, len(pts), ctypes.byref(npts), recs.ctypes.data, len(recs),
                                      ctypes.byref(nrec)))
        return head, pts, recs


def ppm(frame):
    """one RGB24 frame [H, W, 3] behind a P6 header"""
    h, w = frame.shape[:2]
    return b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(frame, np.uint8).tobytes()


def write_frames(handle, paths, fig_format, quality):
    """The figures set in `handle` (a FigureHandle), one file per path: rendered, then as "jpg" encoded on the same stream without a
    synchronisation in between, or as "ppm" wrapped; one read-back either way.  Returns the paths."""
    if fig_format == "jpg":
        if handle._enc is None or handle._enc[0] != quality:
            from .mjpeg import Encoder
            handle._enc = (quality, Encoder(handle.H, handle.W, "rgb24", quality, handle.params["max_figures"], handle.device))
        enc = handle._enc[1]
        enc.encode(handle.device_frames(), handle.n)
        blobs = enc.read()
    else:
        blobs = [ppm(f) for f in handle.frames()]
    for path, blob in zip(paths, blobs):
        with open(path, "wb") as f:
            f.write(blob)
    return list(paths)


def figure_name(src, fig_format):
    return f'{os.path.basename(src).split(".")[0]}.{fig_format}'                      # reference plot.py:220 with the new extension


def load(src, plate_diameter):
    """(rows [T, 7], phases) of the id the file name gives, or None for a name the reference refuses (plot.py:78-88)"""
    import pandas as pd
    from .cli import FILENAME_RE, _id_phases
    m = FILENAME_RE.match(os.path.basename(src))
    if not m:
        return None
    df = pd.read_pickle(src)
    tid = m.group(2)
    one = df.query(f"id == {tid}")
    rows = np.stack([one[c].to_numpy(np.float64) for c in COLUMNS], axis=1).reshape(-1, 7)
    return rows, _id_phases(df, tid, plate_diameter)


def plot_many(paths, fig_dir, plate_diameter=0.45, fig_format="jpg", quality=90, device=0, on_file=None, **params):
    """Every DataFrame of `paths` as FIG_DIR/{name}.jpg|ppm: up to max_figures files per set / render / encode, each batch read back
    once.  on_file(src, loaded) is called per file in input order (loaded None: the name did not match and the file is skipped).
    Returns the paths written."""
    if fig_format not in ("jpg", "ppm"):
        raise ValueError(f"fig_format {fig_format!r}: jpg or ppm")
    os.makedirs(fig_dir, exist_ok=True)
    items = []
    for s in paths:
        if not os.path.isfile(s):
            raise FileNotFoundError(s)                                                # reference plot.py:67-68
        loaded = load(s, plate_diameter)
        if on_file:
            on_file(s, loaded)
        if loaded is not None:
            items.append((s, loaded))
    if not items:
        return []
    base = dict(default_params(), **params)
    base["max_rows"] = max(base["max_rows"], max(len(r) for _, (r, _) in items))
    base["max_phases"] = max(base["max_phases"], max(len(p) for _, (_, p) in items))
    base["max_figures"] = min(base["max_figures"], len(items))
    fig = Figure(device, **base)
    written = []
    for b0 in range(0, len(items), base["max_figures"]):
        batch = items[b0:b0 + base["max_figures"]]
        fig.set([ld for _, ld in batch])
        written += write_frames(fig, [os.path.join(fig_dir, figure_name(s, fig_format)) for s, _ in batch], fig_format, quality)
    return written


def plot(src, show_fig=False, save_fig=True, plate_diameter=0.45, fig_dir=None, **kw):
    """The reference's plot(src, show_fig, save_fig, plate_diameter, fig_dir) (plot.py:73): one DataFrame, one figure file.  There is no
    display: show_fig is refused.  Without save_fig nothing is written (the figure is still rendered) and None is returned."""
    if show_fig:
        raise ValueError("plot: there is no display here, show_fig is not offered")
    loaded = load(src, plate_diameter)
    if loaded is None:
        print(f"Couldn't create a plot for file '{src}'.")                             # reference plot.py:81-85
        return None
    if not save_fig:
        p = dict(default_params(), **{k: v for k, v in kw.items() if k in PARAMS})
        p.update(max_figures=1, max_rows=max(len(loaded[0]), 1), max_phases=max(len(loaded[1]), p["max_phases"]))
        f = Figure(kw.get("device", 0), **p)
        f.set([loaded])
        f.frames()
        return None
    out = plot_many([src], fig_dir if fig_dir is not None else ".", plate_diameter, **kw)
    return out[0] if out else None
