"""Tracking overlay: box, tracking id and bar path of the tracked plates drawn into the frames on the GPU - what the reference's
`track.py --video_dir` writes (draw_bounding_box / draw_bar_path, track.py:28-62,201-224) without cv2.

The renderer is a pure function of (frames, DataFrame rows, fps): `render` runs right after tracking or later from a stored
`*.pkl.gz`.  The raster contract (which pixels a box, a bar path segment, the marker and the label cover, and the YUV colour) is in
include/vbt_hip.h, "tracking overlay"; drawing happens in place, in the frames' own pixel format.  torch-free: device memory and
copies through vbt_device_alloc / vbt_memcpy, like Pipeline."""
import ctypes

import numpy as np

from . import _lib
from .mem import DeviceBuffer
from .ocsort import ROW_DTYPE
from .rawvideo import frame_shape, pix_fmt_code, source_hw

COLUMNS = ("id", "time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width")
HUD_PARAMS = ("x", "y", "scale", "full_scale_cm", "bg")
FOLLOW_FLAGS = {1: "BAD_ROW", 2: "ORDER", 4: "FRAME_RANGE", 8: "FRAME_FULL", 16: "REWOUND"}     # VBT_OVERLAY_FOLLOW_*
HUD_FOLLOW_FLAGS = {1: "FLAGGED", 2: "BAD_PHASE", 4: "CAPACITY"}                                   # VBT_OVERLAY_HUD_FOLLOW_*
HUD_FOLLOW_FLAGGED = 1                                                                             # the one bit that is a warning: the live analysis overflowed
COLORS = [(252, 3, 115), (255, 255, 255)]          # COLORS of reference track.py:23 (BGR there) as RGB; the reference draws with [1]


def sorted_rows(data):
    """DataFrame or dict of lists (reference track.py:144-145) -> ROW_DTYPE records sorted by (id, time), the order of track.py:105"""
    n = len(data["id"])
    rows = np.zeros(n, ROW_DTYPE)
    for k in COLUMNS:
        rows[k] = np.asarray(data[k])
    return rows[np.lexsort((rows["time"], rows["id"]))]


def phases6(phases):
    """[P,6] array (time_start, time_end, y_start, y_end, rom, type - what vbt_analyze returns) or a list of velocity.Phase -> float64 [P,6]"""
    if len(phases) and hasattr(phases[0], "time_start"):
        phases = [(p.time_start, p.time_end, p.y_start, p.y_end, p.rom, p.type) for p in phases]
    return np.ascontiguousarray(np.asarray(phases, np.float64).reshape(-1, 6))


class Overlay:
    """vbt_overlay (include/vbt_hip.h): one frame size, pixel format, colour and set of rows.
    params: trail=120, thickness=2, radius=10, label_scale=3, rgb=(255, 255, 255), label=True, box=True."""

    def __init__(self, H, W, pix_fmt="rgb24", device=0, **params):
        L = _lib.lib()
        prm = _lib.OverlayParams()
        L.vbt_overlay_default_params(ctypes.byref(prm))
        for k, v in params.items():
            if k == "rgb":
                prm.rgb[:] = [int(c) for c in v]
            elif k in ("trail", "thickness", "radius", "label_scale", "label", "box"):
                setattr(prm, k, int(v))
            else:
                raise TypeError(f"Overlay: unknown parameter {k!r}")
        self.H, self.W, self.pix_fmt, self.device = int(H), int(W), str(pix_fmt).lower(), int(device)
        h = ctypes.c_void_p()
        _lib.check(L.vbt_overlay_create(self.device, self.H, self.W, pix_fmt_code(pix_fmt), ctypes.byref(prm), ctypes.byref(h)))
        self._h = h
        self.n = 0
        self.hud_n = 0
        self._hud_tracker = None                   # the tracker a following panel borrows: kept alive with the handle

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and getattr(_lib, "_lib", None) is not None:
            _lib._lib.vbt_overlay_destroy(h)

    def set_rows(self, data, fps, stream=None):
        """data: DataFrame or dict of lists with the reference's columns, any order; sorted here by (id, time)."""
        rows = np.ascontiguousarray(sorted_rows(data))
        _lib.check(_lib.lib().vbt_overlay_set_rows(self._h, rows.ctypes.data, len(rows), float(fps), stream))
        self.n = len(rows)

    def follow(self, rows_ptr, nrows_ptr, rows_cap, max_frame, max_rows_per_frame, fps):
        """Follow mode (include/vbt_hip.h, "Following a device row log"): draw from a row log in device memory - rows_ptr its 64-byte
        records in emission order, nrows_ptr the device int32 that counts them (MultiClipTracker.rows_dev gives a clip's) - instead of
        rows from the host.  Replaces the handle's rows; set_rows switches back."""
        _lib.check(_lib.lib().vbt_overlay_follow(self._h, int(rows_ptr), int(nrows_ptr), int(rows_cap), int(max_frame), int(max_rows_per_frame), float(fps)))
        self.n = int(rows_cap)

    def follow_update(self, stream=None):
        """consume the rows the log gained since the last call: one launch on `stream`, enqueue only"""
        _lib.check(_lib.lib().vbt_overlay_follow_update(self._h, stream))

    def follow_status(self, stream=None):
        """(rows consumed, VBT_OVERLAY_FOLLOW_* flags) - synchronises `stream`"""
        n, flags = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(_lib.lib().vbt_overlay_follow_status(self._h, ctypes.byref(n), ctypes.byref(flags), stream))
        return n.value, flags.value

    def draw(self, frames_ptr, B, frame0, frame_step=1, stream=None):
        """B frames at device pointer `frames_ptr`, frame i = frame number frame0 + i * frame_step; in place, enqueue only"""
        _lib.check(_lib.lib().vbt_overlay_draw(self._h, int(frames_ptr), int(B), int(frame0), int(frame_step), stream))

    def set_hud(self, phases, fps=None, stream=None, **hud_params):
        """The rep panel (include/vbt_hip.h, "Rep panel") of ONE id on every frame drawn from now on: rep count, ROM / ACV of the last
        completed rep, a bar per recent rep, the phase timeline.  phases: [P,6] array or list of velocity.Phase (P = 0: "REP    0");
        None switches the panel off.  hud_params: x=16, y=16, scale=3, full_scale_cm=200, bg=(0, 0, 0)."""
        L = _lib.lib()
        if phases is None:
            if hud_params:
                raise TypeError("Overlay.set_hud: no parameters go with phases=None (the panel off)")
            _lib.check(L.vbt_overlay_set_hud(self._h, None, None, 0, 1.0, stream))
            self.hud_n = 0
            self._hud_tracker = None
            return
        if fps is None:
            raise TypeError("Overlay.set_hud: fps is needed with phases")
        prm = _hud_params("Overlay.set_hud", hud_params)
        ph = phases6(phases)
        _lib.check(L.vbt_overlay_set_hud(self._h, ctypes.byref(prm), ph.ctypes.data if len(ph) else None, len(ph), float(fps), stream))
        self.hud_n = len(ph)
        self._hud_tracker = None

    def hud_follow(self, tracker, clip, fps, **hud_params):
        """The rep panel from the live rep analysis (include/vbt_hip.h, "Rep panel from the live analysis"): the panel follows clip
        `clip` of `tracker` (an ocsort.MultiClipTracker with enable_live, or a Pipeline's .tracker) - its table is formed on the device
        from the leader's phase list by hud_follow_update; nothing visits the host.  Replaces a panel of set_hud; set_hud replaces it.
        hud_params: as set_hud."""
        prm = _hud_params("Overlay.hud_follow", hud_params)
        _lib.check(_lib.lib().vbt_overlay_hud_follow(self._h, ctypes.byref(prm), tracker.handle, int(clip), float(fps)))
        self._hud_tracker = tracker
        self.hud_n = int(getattr(tracker, "_live_phase_cap", 0)) or 512          # room for hud_table: the tracker's phase_cap

    def hud_follow_update(self, flush_view=False, stream=None):
        """the panel's table from the live analysis as it stands (flush_view: as if the clip ended now): one launch on `stream`,
        enqueue only.  `stream` is ordered behind the tracker launch to show and ahead of the next one (see the header, "Ordering")."""
        _lib.check(_lib.lib().vbt_overlay_hud_follow_update(self._h, int(bool(flush_view)), stream))

    def hud_follow_flush(self, flush_view):
        """the flush_view of the update Pipeline.overlay_draw makes for this handle"""
        _lib.check(_lib.lib().vbt_overlay_hud_follow_flush(self._h, int(bool(flush_view))))

    def hud_follow_status(self, stream=None):
        """(leader, phases in the table, VBT_OVERLAY_HUD_FOLLOW_* flags so far) - synchronises `stream`"""
        leader, n, flags = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(_lib.lib().vbt_overlay_hud_follow_status(self._h, ctypes.byref(leader), ctypes.byref(n), ctypes.byref(flags), stream))
        return leader.value, n.value, flags.value

    def hud_table(self):
        """int32 [P, 6] = fs, fe, rom_cm, acv_cm, type, concentric phases so far, of every phase of the panel (vbt_overlay_hud_table).
        A following panel: the table of the updates completed so far - synchronise the stream they were enqueued on first, unless it
        is the null stream."""
        out = np.zeros((max(self.hud_n, 1), 6), np.int32)
        n = ctypes.c_int()
        _lib.check(_lib.lib().vbt_overlay_hud_table(self._h, out.ctypes.data, len(out), ctypes.byref(n)))
        return out[:n.value]

    def geometry(self):
        """int32 [n, 8] = frame, cx, cy, xmin, ymin, xmax, ymax, trail length of every row (vbt_overlay_geometry)"""
        out = np.zeros((max(self.n, 1), 8), np.int32)
        n = ctypes.c_int()
        _lib.check(_lib.lib().vbt_overlay_geometry(self._h, out.ctypes.data, len(out), ctypes.byref(n)))
        return out[:n.value]


def follow_flag_names(flags):
    return [name for bit, name in FOLLOW_FLAGS.items() if flags & bit]


def hud_follow_flag_names(flags):
    return [name for bit, name in HUD_FOLLOW_FLAGS.items() if flags & bit]


def _hud_params(who, hud_params):
    """vbt_overlay_hud_params: the defaults with hud_params (x, y, scale, full_scale_cm, bg) over them"""
    prm = _lib.OverlayHudParams()
    _lib.lib().vbt_overlay_hud_default_params(ctypes.byref(prm))
    for k, v in hud_params.items():
        if k == "bg":
            prm.bg[:] = [int(c) for c in v]
        elif k in HUD_PARAMS:
            setattr(prm, k, int(v))
        else:
            raise TypeError(f"{who}: unknown parameter {k!r}")
    return prm


def render(frames, data, fps, frame_stride=1, pix_fmt="rgb24", batch=64, out=None, device=0, sink=None, quality=85, hud=None, hud_params=None,
           display_hw=None, **params):
    """The kept frames of a clip (1-based number a multiple of frame_stride, reference track.py:166) with the overlay of `data`:
    frames uint8 [T,H,W,3] (or [T,H*3//2,W] for "nv12" / "i420"; numpy array or memmap), `batch` frames at a time through the device.
    Returns (or fills `out`, e.g. a numpy.lib.format.open_memmap) uint8 [T // frame_stride, ...] of the same layout.  Unlike the
    reference (track.py:180-181,241-242) every kept frame is there: one without rows comes back undrawn.
    sink: an mjpeg.AviWriter - each batch is then uploaded, drawn, encoded as JPEG on the device at `quality` (mjpeg.Encoder, on the
    stream of the draw, nothing synchronised in between) and only its compressed bytes are read back and written to the sink; `out`
    is not used and the number of frames written is returned.
    hud: the phases of one id (what Overlay.set_hud takes) - the rep panel is then drawn on every kept frame, with hud_params (a dict).
    display_hw: (h, w) - every frame is drawn at full size and then resized to h x w on the device (include/vbt_hip.h, "Scaled
    export"; scale.display_size gives the reference's size for a height): `out` has the layout of (h, w), a sink gets h x w JPEGs."""
    stride = max(int(frame_stride), 1)
    H, W = source_hw(frames, pix_fmt)
    shape = frame_shape(pix_fmt, H, W)
    if tuple(frames.shape[1:]) != shape or frames.dtype != np.uint8:
        raise ValueError(f"render: {pix_fmt} frames must be uint8 [T, {', '.join(str(v) for v in shape)}], got {frames.dtype} {tuple(frames.shape)}")
    kept = int(frames.shape[0]) // stride
    if display_hw is not None:
        display_hw = (int(display_hw[0]), int(display_hw[1]))
    out_shape = shape if display_hw is None else frame_shape(pix_fmt, *display_hw)
    if sink is not None:
        out = None
    elif out is None:
        out = np.empty((kept,) + out_shape, np.uint8)
    elif tuple(out.shape) != (kept,) + out_shape or out.dtype != np.uint8:
        raise ValueError(f"render: out must be uint8 {(kept,) + out_shape}, got {out.dtype} {tuple(out.shape)}")
    ov = Overlay(H, W, pix_fmt, device=device, **params)
    ov.set_rows(data, fps)
    if hud is not None:
        ov.set_hud(hud, fps, **(hud_params or {}))
    L = _lib.lib()
    B = max(1, min(int(batch), max(kept, 1)))
    fb = int(np.prod(shape))
    buf = DeviceBuffer(B * fb, device)
    host = np.empty((B,) + shape, np.uint8)
    enc = scaler = None
    if sink is not None and kept:
        from .mjpeg import Encoder
        enc = Encoder(H, W, pix_fmt, quality=quality, max_batch=B, device=device, out_hw=display_hw)
    elif display_hw is not None and kept:                           # the raw route: scaled into a second buffer, that one copied back
        from .scale import Scaler
        scaler = Scaler(H, W, display_hw[0], display_hw[1], pix_fmt, device=device)
        ob = int(np.prod(out_shape))
        small = DeviceBuffer(B * ob, device)
        host_out = np.empty((B,) + out_shape, np.uint8)
    for i0 in range(0, kept, B):
        nb = min(B, kept - i0)
        first = (i0 + 1) * stride - 1                               # 0-based index of the batch's first kept frame
        host[:nb] = frames[first:first + (nb - 1) * stride + 1:stride]
        _lib.check(L.vbt_memcpy(buf.ptr, host.ctypes.data, nb * fb, 0))
        ov.draw(buf.ptr, nb, (i0 + 1) * stride, stride)
        if enc is not None:
            enc.encode(buf.ptr, nb)
            for jpeg in enc.read():
                sink.write(jpeg)
            continue
        if scaler is not None:
            scaler.run(buf.ptr, small.ptr, nb)
            _lib.check(L.vbt_stream_synchronize(None))
            _lib.check(L.vbt_memcpy(host_out.ctypes.data, small.ptr, nb * ob, 1))
            out[i0:i0 + nb] = host_out[:nb]
            continue
        _lib.check(L.vbt_stream_synchronize(None))
        _lib.check(L.vbt_memcpy(host.ctypes.data, buf.ptr, nb * fb, 1))
        out[i0:i0 + nb] = host[:nb]
    return kept if sink is not None else out
