"""MJPEG export: the drawn frames encoded as baseline JPEG on the GPU (include/vbt_hip.h, "MJPEG export") and wrapped in an AVI that
ffmpeg, VLC and OpenCV open - the reference's `--video_dir` output (track.py:96-98,153-154,241-242) without cv2's VideoWriter.

`Encoder` is vbt_mjpeg: frames in device memory in, the compressed bytes of each frame out; nothing else crosses the bus.  `AviWriter`
is a plain AVI 1.0 writer on the host.

MJPEG import (include/vbt_hip.h, "MJPEG import"), the way back in - the reference's cv2.VideoCapture (track.py:129-160): `AviReader`
walks the RIFF structure of a Motion-JPEG AVI on the host, `Decoder` is vbt_mjpeg_decoder (compressed bytes in, RGB24 frames in device
memory out) and `AviClip` presents a file as the array-like [T,H,W,3] that track_frames, track_many and overlay.render take.  torch-free."""
import ctypes
import mmap
import os
import struct
from fractions import Fraction

import numpy as np

from . import _lib
from .rawvideo import pix_fmt_code

AVI_MAX_BYTES = 2 ** 31 - 1              # AVI 1.0: one RIFF chunk, 32-bit sizes that players read as signed (OpenDML is not written)


class Encoder:
    """vbt_mjpeg (include/vbt_hip.h): one frame size, pixel format and quality; batches of up to max_batch frames.
    out_hw=(h, w): the frames of H x W are encoded as JPEGs of h x w (vbt_mjpeg_create_scaled; "Scaled export"), resized in the
    encoder's colour stage - the bytes Encoder(h, w) gives for the frames scale.Scaler gives."""

    def __init__(self, H, W, pix_fmt="rgb24", quality=85, max_batch=64, device=0, out_hw=None):
        self.H, self.W, self.pix_fmt, self.quality, self.max_batch = int(H), int(W), str(pix_fmt).lower(), int(quality), int(max_batch)
        self.out_hw = (self.H, self.W) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        h = ctypes.c_void_p()
        if out_hw is None:
            _lib.check(_lib.lib().vbt_mjpeg_create(int(device), self.H, self.W, pix_fmt_code(pix_fmt), self.quality, self.max_batch, ctypes.byref(h)))
        else:
            _lib.check(_lib.lib().vbt_mjpeg_create_scaled(int(device), self.H, self.W, self.out_hw[0], self.out_hw[1], pix_fmt_code(pix_fmt), self.quality,
                                                          self.max_batch, ctypes.byref(h)))
        self._h = h
        self._B, self._stream = 0, None
        self._host = np.empty(max(4096, self.out_hw[0] * self.out_hw[1] // 2), np.uint8)
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


# ---- import ----
STATUS_TEXT = {1: "an interval's bits ended before its MCUs did", 2: "a bit pattern no Huffman code matches", 3: "a coefficient index above 63",
               4: "the number of restart markers does not fit the restart interval", 5: "restart markers out of order"}


def probe(jpeg):
    """(H, W, components, sampling) of one JPEG file the decoder accepts (vbt_jpeg_probe: host only); VbtError with the reason otherwise"""
    buf = np.frombuffer(jpeg, np.uint8)
    v = [ctypes.c_int() for _ in range(4)]
    _lib.check(_lib.lib().vbt_jpeg_probe(buf.ctypes.data, buf.nbytes, *(ctypes.byref(x) for x in v)))
    return tuple(x.value for x in v)


ENTROPY_MODES = {"auto": 0, "interval": 1, "sync": 2}


class Decoder:
    """vbt_mjpeg_decoder (include/vbt_hip.h): one frame size; batches of up to max_batch JPEG files -> RGB24 frames in device memory.
    `entropy` ("auto", "interval", "sync") and `subseq_bytes` (0: the default): how the scans are entropy-decoded - set_entropy."""

    def __init__(self, H, W, max_batch=64, device=0, entropy="auto", subseq_bytes=0):
        self.H, self.W, self.max_batch = int(H), int(W), int(max_batch)
        mode = self._mode(entropy)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().vbt_mjpeg_decoder_create(int(device), self.H, self.W, self.max_batch, ctypes.byref(h)))
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

    def set_entropy(self, mode, subseq_bytes=0):
        """"auto": by interval length; "interval": one lane per restart interval; "sync": subsequences of subseq_bytes (0: the default,
        else a power of two in 4..4096) that synchronise.  The frames and the status are the same; it holds from the next decode on."""
        _lib.check(_lib.lib().vbt_mjpeg_decoder_set_entropy(self._h, self._mode(mode), int(subseq_bytes)))

    @property
    def entropy(self):
        """(mode, subseq_bytes, auto_min_interval_bytes): the mode's name, the subsequence size "sync" uses, and the scan bytes per
        restart interval from which "auto" takes the "sync" path"""
        v = [ctypes.c_int() for _ in range(3)]
        _lib.check(_lib.lib().vbt_mjpeg_decoder_get_entropy(self._h, *(ctypes.byref(x) for x in v)))
        return {n: k for k, n in ENTROPY_MODES.items()}[v[0].value], v[1].value, v[2].value

    def entropy_info(self):
        """how the entropy stage of the last batch ran: {"path": 1 (interval) or 2 (sync), "subseq_bytes", "rounds": the most rounds
        any chunk of subsequences took, "single": intervals that one lane finished}; one synchronisation of its stream"""
        info = np.zeros(4, np.int32)
        _lib.check(_lib.lib().vbt_mjpeg_decode_entropy_info(self._h, info.ctypes.data, self._stream))
        return dict(zip(("path", "subseq_bytes", "rounds", "single"), (int(x) for x in info)))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and getattr(_lib, "_lib", None) is not None:
            _lib._lib.vbt_mjpeg_decoder_destroy(h)

    def decode(self, jpegs, frames_ptr, stream=None):
        """jpegs: a sequence of bytes-likes, one complete JPEG file each; the frames go to device pointer `frames_ptr`
        ([len(jpegs), H, W, 3] uint8).  Enqueue only, on `stream`; the bytes may be dropped as soon as the call returns."""
        off = np.zeros(len(jpegs) + 1, np.uint64)
        off[1:] = np.cumsum([len(j) for j in jpegs])
        data = np.frombuffer(b"".join(bytes(j) for j in jpegs) or b"\0", np.uint8)
        _lib.check(_lib.lib().vbt_mjpeg_decode(self._h, data.ctypes.data, off.ctypes.data, len(jpegs), int(frames_ptr), stream))
        self._B, self._stream = len(jpegs), stream

    def status(self):
        """int32 [B]: the scan status of every frame of the last batch (0 = fine; STATUS_TEXT); one synchronisation of its stream"""
        st = np.zeros(max(self._B, 1), np.int32)
        _lib.check(_lib.lib().vbt_mjpeg_decode_status(self._h, st.ctypes.data, self._stream))
        return st[:self._B]


class AviReader:
    """The video frames of a Motion-JPEG AVI 1.0 file: RIFF 'AVI ' -> LIST hdrl (avih; the first LIST strl whose strh is 'vids': its
    strf must say MJPG) and LIST movi; frame k is the k-th 'NNdc' / 'NNdb' chunk of that stream - listed by idx1 when the file has
    one that points at such chunks, found by walking movi ('rec ' lists included) otherwise.  A zero-length chunk repeats the frame
    before it.  Other streams (audio) are skipped.  Refused with the reason (ValueError): anything that is not RIFF / AVI / MJPG, a
    chunk that runs past the file, a file above 2 GiB - 1 (OpenDML is not read)."""

    def __init__(self, path):
        self.path = str(path)
        size = os.path.getsize(self.path)
        if size > AVI_MAX_BYTES:
            raise ValueError(f"{self.path}: {size} bytes, above the AVI 1.0 limit of {AVI_MAX_BYTES} bytes (2 GiB - 1); OpenDML files are not read")
        if size < 12:
            raise ValueError(f"{self.path}: not a RIFF file ({size} bytes)")
        self._f = open(self.path, "rb")
        self._m = m = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ)
        if m[:4] != b"RIFF" or m[8:12] != b"AVI ":
            raise ValueError(f"{self.path}: not a RIFF / AVI file (it starts with {bytes(m[:12])!r})")
        end = min(size, 8 + struct.unpack("<I", m[4:8])[0])
        self.width = self.height = self.rate = self.scale = None
        self.total_frames, stream, movi, idx, n_strl = 0, None, None, None, 0
        for cc, p, n in self._chunks(12, end):
            if cc == b"LIST" and m[p + 8:p + 12] == b"hdrl":
                for c2, p2, n2 in self._chunks(p + 12, p + 8 + n):
                    if c2 == b"avih" and n2 >= 40:
                        self.total_frames = struct.unpack("<I", m[p2 + 24:p2 + 28])[0]
                    if c2 == b"LIST" and m[p2 + 8:p2 + 12] == b"strl":
                        kind = handler = comp = None
                        for c3, p3, n3 in self._chunks(p2 + 12, p2 + 8 + n2):
                            if c3 == b"strh" and n3 >= 36:
                                kind, handler = bytes(m[p3 + 8:p3 + 12]), bytes(m[p3 + 12:p3 + 16])
                                scale, rate = struct.unpack("<II", m[p3 + 28:p3 + 36])
                            if c3 == b"strf" and n3 >= 20:
                                w, h = struct.unpack("<ii", m[p3 + 12:p3 + 20])
                                comp = bytes(m[p3 + 24:p3 + 28])
                        if kind == b"vids" and stream is None:
                            if (comp or handler or b"").upper() not in (b"MJPG",):
                                raise ValueError(f"{self.path}: the video stream is {comp or handler!r}, not MJPG (Motion-JPEG only; mp4 / H.264 are not read)")
                            if rate < 1 or scale < 1:
                                raise ValueError(f"{self.path}: frame rate {rate} / {scale}")
                            stream, self.width, self.height, self.rate, self.scale = n_strl, w, abs(h), rate, scale
                        n_strl += 1
            elif cc == b"LIST" and m[p + 8:p + 12] == b"movi" and movi is None:
                movi = (p + 8, p + 8 + n)
            elif cc == b"idx1":
                idx = (p + 8, n)
        if stream is None:
            raise ValueError(f"{self.path}: no video stream (strh 'vids') in the AVI headers")
        if movi is None:
            raise ValueError(f"{self.path}: no LIST movi")
        tags = (b"%02ddc" % stream, b"%02ddb" % stream)
        found = self._from_index(idx, movi, tags) if idx is not None else None
        if found is None:
            found = [(p + 8, n) for cc, p, n in self._walk_movi(movi[0] + 4, movi[1]) if cc in tags]
        self.chunks = []                                               # (offset, size) of every frame's JPEG file
        for k, (p, n) in enumerate(found):
            if n == 0:
                if not self.chunks:
                    raise ValueError(f"{self.path}: the first frame chunk is empty (nothing to repeat)")
                self.chunks.append(self.chunks[-1])
            else:
                self.chunks.append((p, n))
        self.fps = self.rate / self.scale

    def _chunks(self, start, end):
        """(fourcc, offset of the chunk header, payload size) of the chunks in [start, end)"""
        m, p = self._m, start
        end = min(end, len(m))
        while p + 8 <= end:
            cc, n = bytes(m[p:p + 4]), struct.unpack("<I", m[p + 4:p + 8])[0]
            if p + 8 + n > end:
                raise ValueError(f"{self.path}: chunk {cc!r} at byte {p} says {n} bytes, {end - p - 8} are left")
            yield cc, p, n
            p += 8 + n + (n & 1)

    def _walk_movi(self, start, end):
        for cc, p, n in self._chunks(start, end):
            if cc == b"LIST":
                if n >= 4:
                    yield from self._walk_movi(p + 12, p + 8 + n)
            else:
                yield cc, p, n

    def _from_index(self, idx, movi, tags):
        """the frame chunks by idx1 (offsets from the 'movi' fourcc or from the file's start), or None when it does not point at them"""
        m = self._m
        ent = [struct.unpack("<4sIII", m[idx[0] + 16 * k:idx[0] + 16 * k + 16]) for k in range(idx[1] // 16)]
        ent = [e for e in ent if e[0] in tags]
        if not ent:
            return None
        for base in (movi[0], 0):
            ok = all(base + off + 8 + n <= movi[1] and off + base >= movi[0] and bytes(m[base + off:base + off + 4]) == cc and
                     struct.unpack("<I", m[base + off + 4:base + off + 8])[0] == n for cc, _, off, n in ent)
            if ok:
                return [(base + off + 8, n) for _, _, off, n in ent]
        return None

    def __len__(self):
        return len(self.chunks)

    def frame(self, k):
        """the bytes of frame k: one JPEG file"""
        p, n = self.chunks[k]
        return bytes(self._m[p:p + n])

    def close(self):
        m, self._m = getattr(self, "_m", None), None
        if m is not None:
            m.close()
            self._f.close()

    def __del__(self):
        self.close()


class AviClip:
    """A Motion-JPEG AVI as the clip array [T, H, W, 3] uint8 that track_frames, track_many and overlay.render take: ints and slices
    are decoded on the GPU and read back; decode_into() leaves the frames in device memory.  The frame size is the first frame's (every
    frame must have it); `entropy` is Decoder's; `fps` is the file's rate / scale.  `damaged` collects the indices of frames whose scan status was not 0."""

    dtype = np.dtype(np.uint8)
    ndim = 4

    def __init__(self, path, batch=64, device=0, entropy="auto"):
        self.reader = path if isinstance(path, AviReader) else AviReader(path)
        self.path, self.fps, self.device, self.batch = self.reader.path, self.reader.fps, int(device), max(int(batch), 1)
        self.entropy = entropy
        Decoder._mode(entropy)
        T = len(self.reader)
        if T:
            H, W, _, _ = probe(self.reader.frame(0))
        else:
            H, W = self.reader.height, self.reader.width
        self.shape = (T, int(H), int(W), 3)
        self.damaged = set()
        self._dec = self._buf = None

    def __len__(self):
        return self.shape[0]

    def _decoder(self):
        if self._dec is None:
            self._dec = Decoder(self.shape[1], self.shape[2], max_batch=self.batch, device=self.device, entropy=self.entropy)
        return self._dec

    def decode_into(self, indices, dev_ptr, stream=None):
        """frames `indices` -> [len(indices), H, W, 3] at device pointer dev_ptr, in batches of at most `batch`; enqueue only, on `stream`"""
        dec, fb = self._decoder(), self.shape[1] * self.shape[2] * 3
        indices = [int(i) for i in indices]
        for i0 in range(0, len(indices), self.batch):
            part = indices[i0:i0 + self.batch]
            try:
                dec.decode([self.reader.frame(k) for k in part], int(dev_ptr) + i0 * fb, stream)
            except _lib.VbtError as e:
                raise _lib.VbtError(f"{self.path}: frames {part[0]}..{part[-1]}: {e}") from None

    def __getitem__(self, key):
        from .mem import DeviceBuffer
        T = self.shape[0]
        if isinstance(key, (int, np.integer)):
            k = int(key) + (T if key < 0 else 0)
            if not 0 <= k < T:
                raise IndexError(f"frame {key} of {T}")
            return self[k:k + 1][0]
        if not isinstance(key, slice):
            raise TypeError("AviClip: an int or a slice of frames")
        idx = list(range(*key.indices(T)))
        out = np.empty((len(idx),) + self.shape[1:], np.uint8)
        fb = self.shape[1] * self.shape[2] * 3
        if self._buf is None:
            self._buf = DeviceBuffer(self.batch * fb, self.device)
        for i0 in range(0, len(idx), self.batch):
            part = idx[i0:i0 + self.batch]
            self.decode_into(part, self._buf.ptr)
            self.damaged.update(part[j] for j in np.flatnonzero(self._dec.status()))
            _lib.check(_lib.lib().vbt_memcpy(out[i0:].ctypes.data, self._buf.ptr, len(part) * fb, 1))
        return out
