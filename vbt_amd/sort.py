"""`SortTracker`: the second tracker of the reference hot loop, backed by libvbt_hip.so.

Mirrors what reference track.py uses of `sort.tracker` (sort-track 0.0.8, requirements.txt), the commented-out alternative of
track.py:16,156 that made the reference's dfs/ result set:
  SortTracker(max_age=30)                                            track.py:156
  .update(dets float64[N,6] = x1,y1,x2,y2,score,cls, _unused) -> float64[M,7] = x1,y1,x2,y2,id,cls,score   track.py:186-190
  .trackers: list of objects with .id (0-based) and .kf.x (7x1)      track.py:194-199
plus `MultiClipSortTracker`, the many-clip form: a `MultiClipTracker` (vbt_amd/ocsort.py) whose handle steps SORT, so rows, finish,
phases, summary, live analysis, reset_clips and rows_dev are the inherited ones.

id_base: the package numbers the tracks of ALL trackers of a process from one counter; here the ids of a clip start at id_base + 1
(default 0), and a reset keeps that."""
import ctypes

import numpy as np

from . import _lib
from .ocsort import MAXD, MultiClipTracker


def sort_params(max_age=1, min_hits=3, iou_threshold=0.3, id_base=0):
    """vbt_sort_params; the library refuses negative counts, a non-finite threshold and an id_base outside [0, 0x3fffffff]"""
    for name, v in (("max_age", max_age), ("min_hits", min_hits), ("id_base", id_base)):
        if int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
            raise ValueError(f"{name} must be a 32-bit integer (got {v!r})")
    return _lib.SortParams(int(max_age), int(min_hits), int(id_base), float(iou_threshold))


class MultiClipSortTracker(MultiClipTracker):
    def __init__(self, n_clips, rows_cap, max_age=1, min_hits=3, iou_threshold=0.3, id_base=0, device=0):
        self.n_clips, self.rows_cap = int(n_clips), int(rows_cap)
        self._h = ctypes.c_void_p()
        p = sort_params(max_age, min_hits, iou_threshold, id_base)
        _lib.check(_lib.lib().vbt_tracker_create_sort(self.n_clips, self.rows_cap, ctypes.byref(p), device, ctypes.byref(self._h)))


class SortTracker:
    """Single-clip tracker with the reference's call shape (reference track.py:156,186-199)."""

    def __init__(self, max_age=1, min_hits=3, iou_threshold=0.3, id_base=0, device=0, rows_cap=65536):
        self._mc = MultiClipSortTracker(1, rows_cap, max_age, min_hits, iou_threshold, id_base, device)
        self.frame_count = 0

    def update(self, dets, _=None, time=None):
        dets = np.asarray(dets, dtype=np.float64).reshape(-1, 6)
        n = dets.shape[0]
        if n > MAXD:
            raise ValueError(f"at most {MAXD} detections per frame (got {n})")
        self.frame_count += 1
        if n == 0:                      # the reference never calls update with N = 0 (track.py:180-181)
            return np.empty((0, 7))
        buf = np.zeros((1, 1, MAXD, 6), np.float64)
        buf[0, 0, :n] = dets
        t = float(self.frame_count if time is None else time)
        self._mc.update_frames(buf, np.array([[n]], np.int32), np.array([[t]], np.float64))
        out, self._last_vel = self._mc.last_output(0)
        return out

    @property
    def trackers(self):
        return self._mc.trackers(0)

    @property
    def multi(self):
        return self._mc
