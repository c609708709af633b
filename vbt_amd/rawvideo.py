"""Pixel formats of frame sources and headerless raw video files (include/vbt_hip.h, "pixel formats").

A decoder emits YUV 4:2:0, not packed RGB (the reference's cv2.VideoCapture converts inside the decoder, track.py:135,160).  The
library takes NV12 and I420 as they come - conversion and resize run fused on the device - so a clip written with
`ffmpeg -i clip.mp4 -pix_fmt nv12 -f rawvideo clip.yuv` is tracked without a colour conversion on the CPU.  Nothing here decodes:
the file is the decoder's output, mapped with numpy.  A YUV clip is `uint8 [T, H*3//2, W]`, the usual 2-D view of a 4:2:0 frame.

Webcams and capture cards deliver packed 4:2:2 (`yuyv422`, `uyvy422`: a clip is `uint8 [T, H, 2W]`), 10-bit decoders `p010le` (the NV12
layout in 16-bit words: a clip is little-endian `uint16 [T, H*3//2, W]`).  Every YUV format has a colour description, a matrix
(`bt601` / `bt709`) and a range (`limited` / `full`); (bt601, limited) is the default."""
import os
import re

import numpy as np

# VBT_PIX_RGB24 / VBT_PIX_NV12 / VBT_PIX_I420 / VBT_PIX_YUYV422 / VBT_PIX_UYVY422 / VBT_PIX_P010
PIX_FMTS = {"rgb24": 0, "nv12": 1, "i420": 2, "yuyv422": 16, "uyvy422": 17, "p010le": 18}
COLOR_MATRICES = {"bt601": 0, "bt709": 1}              # VBT_CS_*
COLOR_RANGES = {"limited": 0, "full": 1}               # VBT_RANGE_*
_PLANAR = ("nv12", "i420", "p010le")                   # a luma plane, then H/2 rows of chroma
_PACKED422 = ("yuyv422", "uyvy422")


def pix_fmt_code(pix_fmt):
    try:
        return PIX_FMTS[str(pix_fmt).lower()]
    except KeyError:
        raise ValueError(f"unknown pixel format {pix_fmt!r}: one of {', '.join(PIX_FMTS)}") from None


def colour_codes(matrix="bt601", range="limited"):
    """(VBT_CS_*, VBT_RANGE_*) of a colour description given by name"""
    try:
        m = COLOR_MATRICES[str(matrix).lower()]
    except KeyError:
        raise ValueError(f"unknown colour matrix {matrix!r}: one of {', '.join(COLOR_MATRICES)}") from None
    try:
        return m, COLOR_RANGES[str(range).lower()]
    except KeyError:
        raise ValueError(f"unknown colour range {range!r}: one of {', '.join(COLOR_RANGES)}") from None


def is_yuv(pix_fmt):
    return pix_fmt_code(pix_fmt) != 0


def is_new_format(pix_fmt):
    """the formats the ingest takes but drawing, scaling and JPEG encoding do not (yet)"""
    return pix_fmt_code(pix_fmt) >= 16


def frame_dtype(pix_fmt):
    return np.dtype("<u2") if str(pix_fmt).lower() == "p010le" else np.dtype(np.uint8)


def parse_size(text):
    """'1920x1080' -> (W, H) = (1920, 1080), the order ffmpeg's -s / -video_size uses."""
    m = re.fullmatch(r"\s*(\d+)\s*[xX]\s*(\d+)\s*", str(text))
    if not m or int(m.group(1)) < 1 or int(m.group(2)) < 1:
        raise ValueError(f"size must be WIDTHxHEIGHT, e.g. 1920x1080, got {text!r}")
    return int(m.group(1)), int(m.group(2))


def frame_shape(pix_fmt, H, W):
    """shape of ONE frame of H x W pixels as the pipeline takes it (elements of frame_dtype: bytes, 16-bit words for p010le)"""
    if not is_yuv(pix_fmt):
        return (int(H), int(W), 3)
    fmt = str(pix_fmt).lower()
    if fmt in _PACKED422:
        if H < 1 or W < 2 or W % 2 or H > 16384 or W > 16384:
            raise ValueError(f"YUV 4:2:2 frames have an even width, no side above 16384, got {W}x{H}")
        return (int(H), 2 * int(W))
    if H < 2 or W < 2 or H % 2 or W % 2 or (fmt == "p010le" and (H > 16384 or W > 16384)):
        raise ValueError(f"YUV 4:2:0 frames have even height and width{', no side above 16384' if fmt == 'p010le' else ''}, got {W}x{H}")
    return (int(H) * 3 // 2, int(W))


def source_hw(frames, pix_fmt):
    """(H, W) in pixels of a clip array: [T,H,W,3] for rgb24, [T,H*3//2,W] for nv12 / i420 / p010le (uint16), [T,H,2W] for yuyv422 / uyvy422"""
    shp = tuple(int(v) for v in frames.shape)
    if not is_yuv(pix_fmt):
        return shp[1], shp[2]
    fmt = str(pix_fmt).lower()
    if fmt in _PACKED422:
        if len(shp) != 3 or shp[2] % 4 or shp[2] < 4:
            raise ValueError(f"{pix_fmt} frames must be uint8 [T, H, 2W] with even W, got {shp}")
        return shp[1], shp[2] // 2
    if len(shp) != 3 or shp[1] % 3 or shp[2] % 2:
        raise ValueError(f"{pix_fmt} frames must be {frame_dtype(fmt).name} [T, H*3//2, W] with even H and W, got {shp}")
    return shp[1] * 2 // 3, shp[2]


def open_raw(path, pix_fmt, size):
    """Read-only map of a headerless raw video file (what `ffmpeg -pix_fmt {rgb24,nv12,yuv420p,yuyv422,uyvy422,p010le} -f rawvideo`
    writes) as the clip array of its format.  size = (W, H).  ValueError: the file's length is not a whole number of frames."""
    W, H = size
    shape = frame_shape(pix_fmt, H, W)
    dtype = frame_dtype(pix_fmt)
    fb = int(np.prod(shape)) * dtype.itemsize
    nbytes = os.path.getsize(path)
    if nbytes == 0 or nbytes % fb:
        raise ValueError(f"{path}: {nbytes} bytes is not a whole number of {pix_fmt} frames of {W}x{H} ({fb} bytes each)")
    return np.memmap(path, dtype=dtype, mode="r", shape=(nbytes // fb,) + shape)
