"""Pixel formats of frame sources and headerless raw video files (include/vbt_hip.h, "pixel formats").

A decoder emits YUV 4:2:0, not packed RGB (the reference's cv2.VideoCapture converts inside the decoder, track.py:135,160).  The
library takes NV12 and I420 as they come - conversion and resize run fused on the device - so a clip written with
`ffmpeg -i clip.mp4 -pix_fmt nv12 -f rawvideo clip.yuv` is tracked without a colour conversion on the CPU.  Nothing here decodes:
the file is the decoder's output, mapped with numpy.  A YUV clip is `uint8 [T, H*3//2, W]`, the usual 2-D view of a 4:2:0 frame."""
import os
import re

import numpy as np

PIX_FMTS = {"rgb24": 0, "nv12": 1, "i420": 2}          # VBT_PIX_RGB24 / VBT_PIX_NV12 / VBT_PIX_I420


def pix_fmt_code(pix_fmt):
    try:
        return PIX_FMTS[str(pix_fmt).lower()]
    except KeyError:
        raise ValueError(f"unknown pixel format {pix_fmt!r}: one of {', '.join(PIX_FMTS)}") from None


def is_yuv(pix_fmt):
    return pix_fmt_code(pix_fmt) != 0


def parse_size(text):
    """'1920x1080' -> (W, H) = (1920, 1080), the order ffmpeg's -s / -video_size uses."""
    m = re.fullmatch(r"\s*(\d+)\s*[xX]\s*(\d+)\s*", str(text))
    if not m or int(m.group(1)) < 1 or int(m.group(2)) < 1:
        raise ValueError(f"size must be WIDTHxHEIGHT, e.g. 1920x1080, got {text!r}")
    return int(m.group(1)), int(m.group(2))


def frame_shape(pix_fmt, H, W):
    """shape of ONE frame of H x W pixels as the pipeline takes it"""
    if not is_yuv(pix_fmt):
        return (int(H), int(W), 3)
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"YUV 4:2:0 frames have even height and width, got {W}x{H}")
    return (int(H) * 3 // 2, int(W))


def source_hw(frames, pix_fmt):
    """(H, W) in pixels of a clip array: [T,H,W,3] for rgb24, [T,H*3//2,W] for nv12 / i420"""
    shp = tuple(int(v) for v in frames.shape)
    if not is_yuv(pix_fmt):
        return shp[1], shp[2]
    if len(shp) != 3 or shp[1] % 3 or shp[2] % 2:
        raise ValueError(f"{pix_fmt} frames must be uint8 [T, H*3//2, W] with even H and W, got {shp}")
    return shp[1] * 2 // 3, shp[2]


def open_raw(path, pix_fmt, size):
    """Read-only map of a headerless raw video file (what `ffmpeg -pix_fmt {rgb24,nv12,yuv420p} -f rawvideo` writes) as the clip
    array of its format.  size = (W, H).  ValueError: the file's length is not a whole number of frames."""
    W, H = size
    shape = frame_shape(pix_fmt, H, W)
    fb = int(np.prod(shape))
    nbytes = os.path.getsize(path)
    if nbytes == 0 or nbytes % fb:
        raise ValueError(f"{path}: {nbytes} bytes is not a whole number of {pix_fmt} frames of {W}x{H} ({fb} bytes each)")
    return np.memmap(path, dtype=np.uint8, mode="r", shape=(nbytes // fb,) + shape)
