"""Scaled export: frames resized on the GPU to the reference's `--display_image_height` (track.py:69,139-140,237-239) - there it is
the size of a window, here of the exported frames (include/vbt_hip.h, "Scaled export": the size rule, the axis tables and the sample,
pinned to integers).  `display_size` is the size rule, `Scaler` is vbt_scaler: frames of H x W in device memory in, frames of h x w
out, in the source's own pixel format.  torch-free."""
import ctypes

import numpy as np

from . import _lib
from .rawvideo import pix_fmt_code


def display_size(H, W, pix_fmt="rgb24", display_height=720):
    """(h, w) of a source of H x W pixels exported display_height lines high: w = int(h * (float(W) / float(H))), rounded down to even
    for "nv12" / "i420".  ValueError (VbtArgError) with the reason: a side outside 1..16384, an odd height with a YUV format."""
    h, w = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().vbt_display_size(int(H), int(W), pix_fmt_code(pix_fmt), int(display_height), ctypes.byref(h), ctypes.byref(w)))
    return h.value, w.value


class Scaler:
    """vbt_scaler (include/vbt_hip.h): one source size, output size and pixel format."""

    def __init__(self, H, W, h, w, pix_fmt="rgb24", device=0):
        self.H, self.W, self.h, self.w, self.pix_fmt, self.device = int(H), int(W), int(h), int(w), str(pix_fmt).lower(), int(device)
        p = ctypes.c_void_p()
        _lib.check(_lib.lib().vbt_scaler_create(self.device, self.H, self.W, self.h, self.w, pix_fmt_code(pix_fmt), ctypes.byref(p)))
        self._h = p

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and getattr(_lib, "_lib", None) is not None:
            _lib._lib.vbt_scaler_destroy(h)

    def run(self, src_ptr, dst_ptr, B, stream=None):
        """B frames at device pointer src_ptr -> B frames at dst_ptr (the layouts Overlay.draw takes); one launch, enqueue only"""
        _lib.check(_lib.lib().vbt_scaler_run(self._h, int(src_ptr), int(dst_ptr), int(B), stream))

    def tables(self, plane=0, axis=0):
        """(i0, a) int32 arrays of the handle's axis table, read back from the device: plane 0 = luma or RGB, 1 = chroma (YUV);
        axis 0 = y, 1 = x"""
        cap = max(self.h, self.w)
        i0, a, n = np.zeros(cap, np.int32), np.zeros(cap, np.int32), ctypes.c_int()
        _lib.check(_lib.lib().vbt_scaler_tables(self._h, int(plane), int(axis), i0.ctypes.data, a.ctypes.data, cap, ctypes.byref(n)))
        return i0[:n.value], a[:n.value]
