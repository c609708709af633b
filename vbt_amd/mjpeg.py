"""MJPEG export: the drawn frames encoded as baseline JPEG on the GPU (include/vbt_hip.h, "MJPEG export") and wrapped in an AVI that
ffmpeg, VLC and OpenCV open - the reference's `--video_dir` output (track.py:96-98,153-154,241-242) without cv2's VideoWriter.

`Encoder` is vbt_mjpeg: frames in device memory in, the compressed bytes of each frame out; nothing else crosses the bus.  `AviWriter`
is a plain AVI 1.0 writer on the host.  torch-free."""
import ctypes
import struct
from fractions import Fraction

import numpy as np

from . import _lib
from .rawvideo import pix_fmt_code

AVI_MAX_BYTES = 2 ** 31 - 1              # AVI 1.0: one RIFF chunk, 32-bit sizes that players read as signed (OpenDML is not written)


class Encoder:
    """vbt_mjpeg (include/vbt_hip.h): one frame size, pixel format and quality; batches of up to max_batch frames."""

    def __init__(self, H, W, pix_fmt="rgb24", quality=85, max_batch=64, device=0):
        self.H, self.W, self.pix_fmt, self.quality, self.max_batch = int(H), int(W), str(pix_fmt).lower(), int(quality), int(max_batch)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().vbt_mjpeg_create(int(device), self.H, self.W, pix_fmt_code(pix_fmt), self.quality, self.max_batch, ctypes.byref(h)))
        self._h = h
        self._B, self._stream = 0, None
        self._host = np.empty(max(4096, self.H * self.W // 2), np.uint8)
        self.last_bytes = 0

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and getattr(_lib, "_lib", None) is not None:
            _lib._lib.vbt_mjpeg_destroy(h)

    def encode(self, frames_ptr, B, stream=None):
        """B frames at device pointer `frames_ptr` (the layout Overlay.draw takes); enqueue only, on `stream`"""
        _lib.check(_lib.lib().vbt_mjpeg_encode(self._h, int(frames_ptr), int(B), stream))
        self._B, self._stream = int(B), stream

    def read(self):
        """the bytes of every frame of the batch, each a complete JPEG file: one synchronisation, the offsets, one copy"""
        L = _lib.lib()
        off = np.zeros(self._B + 1, np.uint64)
        while True:
            rc = L.vbt_mjpeg_read(self._h, self._host.ctypes.data, self._host.nbytes, off.ctypes.data, self._stream)
            if rc == -4 and self._B and int(off[-1]) > self._host.nbytes:      # room for less than the batch: it stays readable
                self._host = np.empty(int(off[-1]) * 5 // 4, np.uint8)
                continue
            _lib.check(rc)
            break
        self.last_bytes = int(off[-1])
        data = self._host[:self.last_bytes].tobytes()
        self._B = 0
        return [data[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def frame_rate(fps, frame_stride=1):
    """(rate, scale) of fps / frame_stride as a rational: 29.97 at stride 1 -> (2997, 100)"""
    f = Fraction(str(float(fps))).limit_denominator(100000) / max(int(frame_stride), 1)
    if f <= 0:
        raise ValueError(f"frame rate must be positive, got {fps}")
    return f.numerator, f.denominator


class AviWriter:
    """AVI 1.0 with one MJPG video stream: RIFF 'AVI ' = LIST hdrl (avih, LIST strl (strh, strf)), LIST movi (one '00dc' chunk per frame,
    padded to even length), idx1.  The frame rate is rate / scale.  Sizes and frame counts are patched by close()."""

    def __init__(self, path, W, H, rate, scale=1):
        self.W, self.H, self.rate, self.scale = int(W), int(H), int(rate), int(scale)
        if self.rate < 1 or self.scale < 1 or self.W < 1 or self.H < 1:
            raise ValueError(f"AviWriter: positive size and rate / scale, got {W}x{H} at {rate}/{scale}")
        self.path, self.frames, self._index, self._largest = path, 0, [], 0
        self._f = open(path, "wb")
        self._f.write(self._headers())
        self._movi = self._f.tell() - 4                                     # offset of the 'movi' fourcc: idx1 offsets count from it
        self._pos = self._f.tell()

    def _headers(self):
        n, us = self.frames, (1000000 * self.scale + self.rate // 2) // self.rate
        per_sec = (self._largest * self.rate + self.scale - 1) // self.scale
        avih = struct.pack("<14I", us, min(per_sec, 0xFFFFFFFF), 0, 0x10, n, 0, 1, self._largest, self.W, self.H, 0, 0, 0, 0)      # 0x10: AVIF_HASINDEX
        strh = struct.pack("<4s4sIHHIIIIIIiI4h", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, n, self._largest, -1, 0, 0, 0, self.W, self.H)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.W, self.H, 1, 24, b"MJPG", self.W * self.H * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        movi_size = 4 + sum(8 + size + (size & 1) for _, size in self._index)
        riff_size = 4 + 8 + len(hdrl) + 8 + movi_size + 8 + 16 * n
        return b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + \
            b"LIST" + struct.pack("<I", movi_size) + b"movi"

    def write(self, jpeg):
        """one frame: the bytes of a complete JPEG file"""
        if self._f is None:
            raise ValueError("AviWriter: write after close")
        size = len(jpeg)
        end = self._pos + 8 + size + (size & 1) + 8 + 16 * (self.frames + 1)    # the file once this frame and the index are in it
        if end > AVI_MAX_BYTES:
            raise ValueError(f"{self.path}: frame {self.frames + 1} would take the file to {end} bytes, past the AVI 1.0 limit of {AVI_MAX_BYTES} "
                             "bytes (2 GiB - 1): use a lower --video_quality or export a shorter clip")
        self._f.write(b"00dc" + struct.pack("<I", size) + jpeg + (b"\0" if size & 1 else b""))
        self._index.append((self._pos - self._movi, size))
        self._pos += 8 + size + (size & 1)
        self._largest = max(self._largest, size)
        self.frames += 1

    def close(self):
        if self._f is None:
            return
        f, self._f = self._f, None
        f.write(b"idx1" + struct.pack("<I", 16 * self.frames) + b"".join(struct.pack("<4sIII", b"00dc", 0x10, off, size) for off, size in self._index))
        f.seek(0)
        f.write(self._headers())
        f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
