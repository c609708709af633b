"""TEST INFRASTRUCTURE ONLY (numpy): the YUV -> RGB contract of include/vbt_hip.h ("more source formats") for all five YUV formats
under a colour description, written from the header's formula and derivation, and a test-only encoder that manufactures inputs (its
exact arithmetic does not matter: every comparison is against decode(encode(...))).

Frames: nv12 / i420 uint8 [..., H*3//2, W]; yuyv422 / uyvy422 uint8 [..., H, 2W]; p010le uint16 [..., H*3//2, W] (sample = word >> 6)."""
import math

import numpy as np

FMTS = ("nv12", "i420", "yuyv422", "uyvy422", "p010le")
MATRICES = ("bt601", "bt709")
RANGES = ("limited", "full")
KRKB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
SCALES = {(8, "limited"): (219, 224), (8, "full"): (255, 255), (10, "limited"): (876, 896), (10, "full"): (1023, 1023)}   # (ys, cs)
# the header's table: (matrix, depth, range) -> CY, CRV, CGU, CGV, CBU
TABLE = {("bt601", 8, "limited"): (1220542, 1673527, 409993, 852492, 2116026),
         ("bt601", 8, "full"): (1048576, 1470104, 360853, 748826, 1858077),
         ("bt601", 10, "limited"): (305236, 418389, 102698, 213115, 528805),
         ("bt601", 10, "full"): (261375, 366448, 89949, 186658, 463157),
         ("bt709", 8, "limited"): (1220945, 1879825, 223607, 558796, 2215014),
         ("bt709", 8, "full"): (1048576, 1651297, 196424, 490864, 1945738),
         ("bt709", 10, "limited"): (305236, 469956, 55902, 139699, 553753),
         ("bt709", 10, "full"): (261375, 411614, 48962, 122356, 485008)}


def depth(fmt):
    return 10 if fmt == "p010le" else 8


def derive(matrix, bits, rng):
    """C = floor(x * 2^20 + 0.5) in double precision, as the header derives every row but (bt601, 8, limited)"""
    kr, kb = KRKB[matrix]
    kg = 1 - kr - kb
    ys, cs = SCALES[(bits, rng)]
    xs = (255 / ys, 2 * (1 - kr) * 255 / cs, 2 * (1 - kb) * kb / kg * 255 / cs, 2 * (1 - kr) * kr / kg * 255 / cs, 2 * (1 - kb) * 255 / cs)
    return tuple(int(math.floor(x * 2 ** 20 + 0.5)) for x in xs)


def offsets(bits, rng):
    """YOFF, COFF"""
    return (0 if rng == "full" else 16 << (bits - 8)), 128 << (bits - 8)


def yuv_to_rgb(Y, U, V, matrix="bt601", rng="limited", bits=8):
    """the integer formula, elementwise (int32; >> arithmetic; clip8 saturates)"""
    cy, crv, cgu, cgv, cbu = (np.int32(c) for c in TABLE[(matrix, bits, rng)])
    yoff, coff = offsets(bits, rng)
    yp = np.maximum(np.asarray(Y, np.int32) - yoff, 0) * cy + np.int32(1 << 19)
    u = np.asarray(U, np.int32) - coff
    v = np.asarray(V, np.int32) - coff
    r = (yp + crv * v) >> 20
    g = (yp - cgu * u - cgv * v) >> 20
    b = (yp + cbu * u) >> 20
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def planes(frame, fmt):
    """(Y [..., H, W], U, V [..., H/cy, W/2], cy): the samples of a frame, chroma not yet upsampled; cy = luma rows per chroma row"""
    f = np.asarray(frame)
    lead = f.shape[:-2]
    if fmt in ("yuyv422", "uyvy422"):
        assert f.dtype == np.uint8 and f.shape[-1] % 4 == 0, (f.dtype, f.shape)
        q = f.reshape(lead + (f.shape[-2], f.shape[-1] // 4, 4))
        if fmt == "yuyv422":
            y, u, v = q[..., 0::2], q[..., 1], q[..., 3]
        else:
            y, u, v = q[..., 1::2], q[..., 0], q[..., 2]
        return y.reshape(lead + (f.shape[-2], f.shape[-1] // 2)), u, v, 1
    H, W = f.shape[-2] * 2 // 3, f.shape[-1]
    assert f.shape[-2] * 2 == H * 3 and H % 2 == 0 and W % 2 == 0, f.shape
    if fmt == "p010le":
        assert f.dtype == np.uint16, f.dtype
        f = f >> 6                                                       # the low 6 bits are ignored
    else:
        assert f.dtype == np.uint8, f.dtype
    y = f[..., :H, :]
    c = f[..., H:, :].reshape(lead + (H * W // 2,))
    if fmt in ("nv12", "p010le"):
        uv = c.reshape(lead + (H // 2, W // 2, 2))
        return y, uv[..., 0], uv[..., 1], 2
    assert fmt == "i420", fmt
    q = H * W // 4
    return y, c[..., :q].reshape(lead + (H // 2, W // 2)), c[..., q:].reshape(lead + (H // 2, W // 2)), 2


def decode(frame, fmt, matrix="bt601", rng="limited"):
    """-> uint8 [..., H, W, 3]: 4:2:2 pixel (y, x) takes the chroma of (y, x >> 1), the others (y >> 1, x >> 1); nearest"""
    y, u, v, cy = planes(frame, fmt)
    up = lambda p: np.repeat(np.repeat(p, cy, axis=-2), 2, axis=-1)
    return yuv_to_rgb(y, up(u), up(v), matrix, rng, depth(fmt))


def encode(rgb, fmt, matrix="bt601", rng="limited"):
    """test-only encoder: uint8 [..., H, W, 3] -> a frame of fmt (float64, rounded; chroma = mean of the pixels that share it)"""
    return pack(*samples(rgb, fmt, matrix, rng), fmt)


def samples(rgb, fmt, matrix="bt601", rng="limited"):
    """the encoder's samples before they are packed: Y [..., H, W], U and V [..., H or H/2, W/2]"""
    a = np.asarray(rgb, np.uint8).astype(np.float64)
    H, W = a.shape[-3], a.shape[-2]
    lead = a.shape[:-3]
    bits = depth(fmt)
    kr, kb = KRKB[matrix]
    ys, cs = SCALES[(bits, rng)]
    yoff, coff = offsets(bits, rng)
    top = (1 << bits) - 1
    luma = kr * a[..., 0] + (1 - kr - kb) * a[..., 1] + kb * a[..., 2]
    cb = (a[..., 2] - luma) / (2 * (1 - kb))
    cr = (a[..., 0] - luma) / (2 * (1 - kr))
    cy = 1 if fmt in ("yuyv422", "uyvy422") else 2
    assert W % 2 == 0 and H % cy == 0
    blk = lambda p: p.reshape(lead + (H // cy, cy, W // 2, 2)).mean(axis=(-3, -1))
    q = lambda p: np.clip(np.floor(p + 0.5), 0, top).astype(np.uint16)
    return q(luma * ys / 255 + yoff), q(blk(cb) * cs / 255 + coff), q(blk(cr) * cs / 255 + coff)


def pack(y, u, v, fmt):
    """samples Y [..., H, W], U and V [..., H or H/2, W/2] (8-bit, 10-bit for p010le) -> a frame of fmt; the inverse of planes()"""
    y, u, v = (np.asarray(p).astype(np.uint16) for p in (y, u, v))
    H, W = y.shape[-2:]
    lead = y.shape[:-2]
    cy = 1 if fmt in ("yuyv422", "uyvy422") else 2
    assert u.shape == v.shape == lead + (H // cy, W // 2) and W % 2 == 0 and H % cy == 0, (y.shape, u.shape, v.shape)
    if cy == 1:
        y2 = y.reshape(lead + (H, W // 2, 2))
        order = (y2[..., 0], u, y2[..., 1], v) if fmt == "yuyv422" else (u, y2[..., 0], v, y2[..., 1])
        return np.stack(order, axis=-1).reshape(lead + (H, 2 * W)).astype(np.uint8)
    if fmt == "i420":
        c = np.concatenate([u.reshape(lead + (H * W // 4,)), v.reshape(lead + (H * W // 4,))], axis=-1).reshape(lead + (H // 2, W))
    else:
        c = np.stack([u, v], axis=-1).reshape(lead + (H // 2, W))
    out = np.concatenate([y, c], axis=-2)
    return (out << 6).astype(np.uint16) if fmt == "p010le" else out.astype(np.uint8)
