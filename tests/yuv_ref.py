"""TEST INFRASTRUCTURE ONLY (numpy): the YUV 4:2:0 -> RGB contract of include/vbt_hip.h ("pixel formats"), written from the formula,
and a test-only RGB -> NV12 / I420 encoder that manufactures inputs (its exact arithmetic does not matter: what the tests compare
is the RGB this module decodes from the encoded frames).

A frame is uint8 [H*3//2, W]: H rows of luma, then H/2 rows of chroma - NV12: interleaved U,V, W bytes per row; I420: the
H/2 x W/2 U plane followed by the H/2 x W/2 V plane (H*W/4 bytes each, i.e. H/4 rows of the 2-D view each).
Parity with cv2.cvtColor(COLOR_YUV2RGB_NV12 / _I420) is unpinned (OpenCV is not installed); the formula is the contract."""
import numpy as np


def _planes(frame, fmt):
    f = np.asarray(frame, np.uint8)
    H, W = f.shape[-2] * 2 // 3, f.shape[-1]
    assert f.shape[-2] * 2 == H * 3 and H % 2 == 0 and W % 2 == 0, f.shape
    lead = f.shape[:-2]
    y = f[..., :H, :]
    c = f[..., H:, :].reshape(lead + (H * W // 2,))
    if fmt == "nv12":
        uv = c.reshape(lead + (H // 2, W // 2, 2))
        return y, uv[..., 0], uv[..., 1]
    assert fmt == "i420", fmt
    q = H * W // 4
    return y, c[..., :q].reshape(lead + (H // 2, W // 2)), c[..., q:].reshape(lead + (H // 2, W // 2))


def yuv_to_rgb(Y, U, V):
    """the integer formula, elementwise (int32; >> arithmetic; clip8 saturates)"""
    yp = np.maximum(np.asarray(Y, np.int32) - 16, 0) * np.int32(1220542) + np.int32(1 << 19)
    u = np.asarray(U, np.int32) - 128
    v = np.asarray(V, np.int32) - 128
    r = (yp + 1673527 * v) >> 20
    g = (yp - 409993 * u - 852492 * v) >> 20
    b = (yp + 2116026 * u) >> 20
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def rgb_from_yuv(frame, fmt):
    """uint8 [..., H*3//2, W] -> uint8 [..., H, W, 3]: chroma sample (y >> 1, x >> 1), nearest"""
    y, u, v = _planes(frame, fmt)
    up = lambda p: np.repeat(np.repeat(p, 2, axis=-2), 2, axis=-1)
    return yuv_to_rgb(y, up(u), up(v))


def rgb_from_nv12(frame):
    return rgb_from_yuv(frame, "nv12")


def rgb_from_i420(frame):
    return rgb_from_yuv(frame, "i420")


def encode(rgb, fmt):
    """test-only encoder: uint8 [..., H, W, 3] -> uint8 [..., H*3//2, W] (BT.601 limited range, chroma = mean of the 2x2 block)"""
    a = np.asarray(rgb, np.uint8).astype(np.int32)
    H, W = a.shape[-3], a.shape[-2]
    assert H % 2 == 0 and W % 2 == 0
    lead = a.shape[:-3]
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    y = np.clip(((66 * r + 129 * g + 25 * b + 128) >> 8) + 16, 0, 255)
    blk = lambda p: p.reshape(lead + (H // 2, 2, W // 2, 2)).sum(axis=(-3, -1))
    rs, gs, bs = blk(r), blk(g), blk(b)
    u = np.clip(((-38 * rs - 74 * gs + 112 * bs + 512) >> 10) + 128, 0, 255)
    v = np.clip(((112 * rs - 94 * gs - 18 * bs + 512) >> 10) + 128, 0, 255)
    if fmt == "nv12":
        c = np.stack([u, v], axis=-1).reshape(lead + (H // 2, W))
    else:
        assert fmt == "i420", fmt
        c = np.concatenate([u.reshape(lead + (H * W // 4,)), v.reshape(lead + (H * W // 4,))], axis=-1).reshape(lead + (H // 2, W))
    return np.concatenate([y, c], axis=-2).astype(np.uint8)
