"""JPEG stills on the GPU (`vbt_jpeg_stills`, include/vbt_hip.h "JPEG stills"): one batch of baseline JPEG files, every file its own
size and sampling, decoded on the device - either straight to the network input (decode_resized: fancy upsampling, colour and the
bilinear resize of preprocess_image in one kernel, no RGB frame at source size is written) or to packed RGB24 frames (decode).
Only the compressed bytes cross the bus.  A thin ctypes wrapper: no torch."""
import ctypes

import numpy as np

from . import _lib
from .mjpeg import ENTROPY_MODES, STATUS_TEXT, probe  # noqa: F401  (re-exported: the stills share the import's scope and status codes)

MAX_BATCH = 1024
MAX_BLOCK_BUDGET = 1 << 24


def blocks(jpeg):
    """the 8 x 8 blocks one JPEG file takes of a handle's budget (vbt_jpeg_blocks: host only); VbtError with the reason when the
    decoder refuses the file"""
    buf = np.frombuffer(jpeg, np.uint8)
    n = ctypes.c_uint32()
    _lib.check(_lib.lib().vbt_jpeg_blocks(buf.ctypes.data, buf.nbytes, ctypes.byref(n)))
    return int(n.value)


def plan(block_counts, max_batch, block_budget):
    """cut a list of files, given by their block counts, into batches in the given order: [(first, end)], each of at most max_batch
    files and block_budget blocks.  ValueError when one file alone is over the budget."""
    out, first, used = [], 0, 0
    for i, n in enumerate(block_counts):
        if n > block_budget:
            raise ValueError(f"file {i} needs {n} blocks, the budget is {block_budget}")
        if i - first >= max_batch or used + n > block_budget:
            out.append((first, i))
            first, used = i, 0
        used += n
    if len(block_counts) > first:
        out.append((first, len(block_counts)))
    return out


class JpegStills:
    """vbt_jpeg_stills: batches of up to max_batch JPEG files that together take at most block_budget 8 x 8 blocks (196 bytes of
    device scratch per block of budget).  `entropy` / `subseq_bytes` as mjpeg.Decoder has them."""

    def __init__(self, max_batch=64, block_budget=1 << 22, device=0, entropy="auto", subseq_bytes=0):
        self.max_batch, self.block_budget, self.device = int(max_batch), int(block_budget), int(device)
        mode = self._mode(entropy)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().vbt_jpeg_stills_create(self.device, self.max_batch, self.block_budget, ctypes.byref(h)))
        self._h = h
        self._B, self._stream = 0, None
        if mode or subseq_bytes:
            self.set_entropy(mode, subseq_bytes)

    @staticmethod
    def _mode(mode):
        if isinstance(mode, str):
            if mode.lower() not in ENTROPY_MODES:
                raise ValueError(f"entropy mode {mode!r}: one of {', '.join(ENTROPY_MODES)}")
            return ENTROPY_MODES[mode.lower()]
        return int(mode)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and getattr(_lib, "_lib", None) is not None:
            _lib._lib.vbt_jpeg_stills_destroy(h)

    def set_entropy(self, mode, subseq_bytes=0):
        _lib.check(_lib.lib().vbt_jpeg_stills_set_entropy(self._h, self._mode(mode), int(subseq_bytes)))

    @property
    def entropy(self):
        """(mode, subseq_bytes, auto_min_interval_bytes), as mjpeg.Decoder.entropy"""
        v = [ctypes.c_int() for _ in range(3)]
        _lib.check(_lib.lib().vbt_jpeg_stills_get_entropy(self._h, *(ctypes.byref(x) for x in v)))
        return {n: k for k, n in ENTROPY_MODES.items()}[v[0].value], v[1].value, v[2].value

    def entropy_info(self):
        """{"path", "subseq_bytes", "rounds", "single"} of the last batch, as mjpeg.Decoder.entropy_info"""
        info = np.zeros(4, np.int32)
        _lib.check(_lib.lib().vbt_jpeg_stills_entropy_info(self._h, info.ctypes.data, self._stream))
        return dict(zip(("path", "subseq_bytes", "rounds", "single"), (int(x) for x in info)))

    def stage_ms(self):
        """the six stage times of the last batch in milliseconds (H2D copy, memsets, marker scan, entropy decode, IDCT, colour or
        colour + resize); needs VBT_MJPEG_DECODE_STAMPS=1 in the environment when the handle is made"""
        ms = (ctypes.c_float * 6)()
        _lib.check(_lib.lib().vbt_jpeg_stills_stage_ms(self._h, ms))
        return [float(v) for v in ms]

    def uploaded_bytes(self):
        """the bytes of the last batch's one H2D copy: descriptors, geometry table and entropy-coded segments"""
        n = ctypes.c_uint64()
        _lib.check(_lib.lib().vbt_jpeg_stills_uploaded_bytes(self._h, ctypes.byref(n)))
        return int(n.value)

    def plan(self, jpegs):
        """[(first, end)]: `jpegs` cut, in order, into batches this handle takes"""
        return plan([blocks(j) for j in jpegs], self.max_batch, self.block_budget)

    @staticmethod
    def _pack(jpegs):
        off = np.zeros(len(jpegs) + 1, np.uint64)
        off[1:] = np.cumsum([len(j) for j in jpegs])
        return np.frombuffer(b"".join(bytes(j) for j in jpegs) or b"\0", np.uint8), off

    def decode_resized(self, jpegs, dst_ptr, h, w, swap_rb=False, stream=None):
        """jpegs: a sequence of bytes-likes, one complete JPEG file each, of any accepted size and sampling; device pointer `dst_ptr`
        ([len(jpegs), h, w, 3] uint8) gets preprocess_image(decode(file), (h, w), swap_rb) of each.  Enqueue only, on `stream`."""
        data, off = self._pack(jpegs)
        _lib.check(_lib.lib().vbt_jpeg_stills_decode_resized(self._h, data.ctypes.data, off.ctypes.data, len(jpegs), int(dst_ptr), int(h), int(w),
                                                             int(bool(swap_rb)), stream))
        self._B, self._stream = len(jpegs), stream

    def decode(self, jpegs, frames_ptr, out_offsets=None, stream=None):
        """frame i as RGB24 [H_i, W_i, 3] at frames_ptr + out_offsets[i] (default: packed one behind the other, from the files'
        headers).  Returns the offsets used, len(jpegs) + 1 of them when they were computed here.  Enqueue only, on `stream`."""
        if out_offsets is None:
            sizes = [probe(j)[:2] for j in jpegs]
            out_offsets = np.zeros(len(jpegs) + 1, np.uint64)
            out_offsets[1:] = np.cumsum([H * W * 3 for H, W in sizes])
        oo = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        if len(oo) < len(jpegs):
            raise ValueError("decode: one output offset per file")
        data, off = self._pack(jpegs)
        _lib.check(_lib.lib().vbt_jpeg_stills_decode(self._h, data.ctypes.data, off.ctypes.data, len(jpegs), int(frames_ptr), oo.ctypes.data, stream))
        self._B, self._stream = len(jpegs), stream
        return oo

    def status(self):
        """int32 [B]: the scan status of every file of the last batch (0 = fine; STATUS_TEXT); one synchronisation of its stream"""
        st = np.zeros(max(self._B, 1), np.int32)
        _lib.check(_lib.lib().vbt_jpeg_stills_status(self._h, st.ctypes.data, self._stream))
        return st[:self._B]
