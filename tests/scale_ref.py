"""The numpy statement of the scaled export (include/vbt_hip.h, "Scaled export"): the size rule, the axis table and the sample, for
rgb24, nv12 and i420 frames in the layouts the library takes, and the shapes the host and GPU tests share."""
import numpy as np

MAX_SIDE = 16384
ONE = 2048

# (H, W, h, w)
RGB_CASES = [(30, 46, 20, 30),        # plain downscaling
             (33, 47, 7, 11),         # a ratio above 4, odd sides
             (9, 13, 31, 40),         # upscaling
             (1, 5, 4, 3),            # one source row: i1 clamps
             (27, 795, 18, 530),      # 1590 bytes a row: seven tiles of 256 bytes along x, the last one partial
             (16, 16, 16, 16)]        # a copy
YUV_CASES = [(36, 52, 24, 34),
             (2, 2, 36, 36),          # a single chroma sample
             (6, 1590, 4, 1060)]      # interleaved chroma across tile boundaries
ENC_CASES = [(30, 46, 20, 30),        # partial MCUs on both axes
             (27, 795, 18, 530),      # 34 MCUs wide: the transform kernel's second workgroup holds two MCUs, the last one partial
             (2, 2, 36, 36)]
TORCH_CASES = [(30, 46, 20, 30), (33, 47, 7, 11), (9, 13, 31, 40), (1, 5, 4, 3), (2, 2, 36, 36), (40, 1, 6, 2), (1080, 1920, 720, 1280)]


def is_yuv(pix_fmt):
    return pix_fmt in ("nv12", "i420")


def display_size(H, W, pix_fmt, display_height):
    """(h, w): the reference's int(h * (float(W) / float(H))) (track.py:139-140); ValueError for what the contract refuses"""
    h = int(display_height)
    if not 1 <= h <= MAX_SIDE:
        raise ValueError(f"display_height {h} outside 1..{MAX_SIDE}")
    if is_yuv(pix_fmt) and h % 2:
        raise ValueError(f"display_height {h} is odd")
    w = int(h * (float(W) / float(H)))
    if is_yuv(pix_fmt):
        w -= w % 2
    if not (2 if is_yuv(pix_fmt) else 1) <= w <= MAX_SIDE:
        raise ValueError(f"width {w} outside 1..{MAX_SIDE}")
    return h, w


def axis_table(n_src, n_dst):
    """(i0, i1, a) of every destination index, int64"""
    o = np.arange(n_dst, dtype=np.float64)
    f = np.maximum((o + 0.5) * (np.float64(n_src) / np.float64(n_dst)) - 0.5, 0.0)
    i0 = np.minimum(np.floor(f).astype(np.int64), n_src - 1)
    i1 = np.minimum(i0 + 1, n_src - 1)
    a = np.rint((f - i0) * float(ONE)).astype(np.int64)
    return i0, i1, a


def scale_plane(p, h, w):
    """p uint8 [B, H, W, C] -> uint8 [B, h, w, C]"""
    H, W = p.shape[1:3]
    y0, y1, ay = axis_table(H, h)
    x0, x1, ax = axis_table(W, w)
    q = p.astype(np.int64)
    ay, ax = ay[None, :, None, None], ax[None, None, :, None]
    r0, r1 = q[:, y0], q[:, y1]
    top = r0[:, :, x0] * (ONE - ax) + r0[:, :, x1] * ax
    bot = r1[:, :, x0] * (ONE - ax) + r1[:, :, x1] * ax
    s = top * (ONE - ay) + bot * ay + (1 << 21)
    assert s.max() < 2 ** 31
    return (s >> 22).astype(np.uint8)


def scale_frames(frames, pix_fmt, h, w):
    """frames uint8 [B, H, W, 3] (rgb24) or [B, H * 3 // 2, W] (nv12 / i420) -> the same layout at h x w"""
    frames = np.asarray(frames)
    if pix_fmt == "rgb24":
        return scale_plane(frames, h, w)
    B, H, W = frames.shape[0], frames.shape[1] * 2 // 3, frames.shape[2]
    luma = scale_plane(frames[:, :H, :, None], h, w)[..., 0]
    if pix_fmt == "nv12":
        uv = scale_plane(frames[:, H:].reshape(B, H // 2, W // 2, 2), h // 2, w // 2)
        return np.concatenate([luma.reshape(B, -1), uv.reshape(B, -1)], axis=1).reshape(B, h * 3 // 2, w)
    flat = frames[:, H:].reshape(B, 2, H // 2, W // 2, 1)
    u, v = scale_plane(flat[:, 0], h // 2, w // 2), scale_plane(flat[:, 1], h // 2, w // 2)
    return np.concatenate([luma.reshape(B, -1), u.reshape(B, -1), v.reshape(B, -1)], axis=1).reshape(B, h * 3 // 2, w)


def frame_shape(pix_fmt, H, W):
    return (H, W, 3) if pix_fmt == "rgb24" else (H * 3 // 2, W)


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def enc_cases():
    """(pix_fmt, H, W, h, w) of every Encoder(out_hw=) case of the GPU test.  YUV 4:2:0 frames have even sides, so the 27 x 795 source
    is 28 x 796 there: the output, and with it the MCU geometry, is the same 18 x 530"""
    return [(f, H + (H & 1 if f != "rgb24" else 0), W + (W & 1 if f != "rgb24" else 0), h, w) for f in ("rgb24", "nv12", "i420") for H, W, h, w in ENC_CASES]


def cases():
    """(pix_fmt, H, W, h, w) of every Scaler case of the GPU test"""
    return [("rgb24",) + c for c in RGB_CASES] + [(f,) + c for f in ("nv12", "i420") for c in YUV_CASES]
