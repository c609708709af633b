"""TEST INFRASTRUCTURE ONLY (numpy): the raster contract of the tracking overlay, written from the text of include/vbt_hip.h
("tracking overlay"), not from the kernel.  It is a gather: for every pixel of a frame, every primitive of every row of that frame
is tested.  It includes the YUV colour and the chroma rule.  Slow and small on purpose."""
import numpy as np

COLUMNS = ("id", "time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width")
DEFAULTS = dict(trail=120, thickness=2, radius=10, label_scale=3, rgb=(255, 255, 255), label=True, box=True)
GEOMETRY = ("frame", "cx", "cy", "xmin", "ymin", "xmax", "ymax", "trail")

GLYPHS = {
    "0": "01110 10001 10011 10101 11001 10001 01110", "6": "00110 01000 10000 11110 10001 10001 01110",
    "1": "00100 01100 00100 00100 00100 00100 01110", "7": "11111 00001 00010 00100 01000 01000 01000",
    "2": "01110 10001 00001 00010 00100 01000 11111", "8": "01110 10001 10001 01110 10001 10001 01110",
    "3": "11111 00010 00100 00010 00001 10001 01110", "9": "01110 10001 10001 01111 00001 00010 01100",
    "4": "00010 00110 01010 10010 11111 00010 00010", "i": "00100 00000 01100 00100 00100 00100 01110",
    "5": "11111 10000 11110 00001 00001 10001 01110", "d": "00001 00001 01101 10011 10001 10001 01111",
}


def glyph(ch):
    """bool [7, 5]: rows top to bottom, columns left to right"""
    return np.array([[b == "1" for b in row] for row in GLYPHS[ch].split()], bool)


def sorted_rows(data):
    """dict of lists / DataFrame -> dict of numpy columns sorted by (id, time), stable"""
    cols = {k: np.asarray(data[k], np.int64 if k == "id" else np.float64) for k in COLUMNS}
    order = np.lexsort((cols["time"], cols["id"]))
    return {k: v[order] for k, v in cols.items()}


def _trunc(v):
    return np.trunc(np.clip(v, -2.0 ** 20, 2.0 ** 20)).astype(np.int64)


def geometry(rows, fps, H, W, trail=120):
    """int64 [n, 8] = frame, cx, cy, xmin, ymin, xmax, ymax, trail length, for rows sorted by (id, time)"""
    x, y, w, h = rows["x"], rows["y"], rows["norm_plate_width"], rows["norm_plate_height"]
    n = len(x)
    g = np.zeros((n, 8), np.int64)
    g[:, 0] = np.rint(np.clip(rows["time"] * np.float64(fps), -2.0 ** 30, 2.0 ** 30)).astype(np.int64)     # llrint: ties to even
    g[:, 1], g[:, 2] = _trunc(x * W), _trunc(y * H)
    g[:, 3], g[:, 5] = _trunc((x - w / 2) * W), _trunc((x + w / 2) * W)
    g[:, 4], g[:, 6] = _trunc((y - h / 2) * H), _trunc((y + h / 2) * H)
    ids = rows["id"]
    for i in range(n):
        k = 1
        while k < trail and i - k >= 0 and ids[i - k] == ids[i]:
            k += 1
        g[i, 7] = k
    return g


def segment_mask(px, py, p0, p1, t):
    """rule 2 for pixel grids px, py (int64) and end points p0, p1 (before the +-32768 clamp)"""
    (x0, y0), (x1, y1) = (tuple(int(np.clip(v, -32768, 32768)) for v in p) for p in (p0, p1))
    dx, dy = x1 - x0, y1 - y0
    qx, qy = px - x0, py - y0
    L2 = dx * dx + dy * dy
    u = qx * dx + qy * dy
    c = qx * dy - qy * dx
    m = 2 * np.abs(c)
    small = m <= 3037000499                                     # m * m fits int64; above it, m^2 > t^2 L2 anyway
    inside = small & (np.where(small, m, 0) ** 2 <= t * t * L2)
    ex, ey = np.where(u <= 0, qx, px - x1), np.where(u <= 0, qy, py - y1)
    ends = 4 * (ex * ex + ey * ey) <= t * t
    return np.where((u > 0) & (u < L2), inside, ends)


def box_mask(px, py, xmin, ymin, xmax, ymax, t):
    a, b = t // 2, (t + 1) // 2
    outer = (px >= xmin - a) & (px <= xmax + a) & (py >= ymin - a) & (py <= ymax + a)
    inner = (px >= xmin + b) & (px <= xmax - b) & (py >= ymin + b) & (py <= ymax - b)      # empty rectangle: all False
    return outer & ~inner


def marker_mask(px, py, cx, cy, R):
    return (px - cx) ** 2 + (py - cy) ** 2 <= R * R


def label_mask(px, py, tid, xmin, ymin, s):
    yb = ymin - 15 if ymin - 15 > 15 else ymin + 15
    m = np.zeros(px.shape, bool)
    for k, ch in enumerate("id" + str(int(tid))):
        bits = glyph(ch)
        for r in range(7):
            for c in range(5):
                if bits[r, c]:
                    left, top = xmin + 6 * s * k + s * c, yb - 7 * s + 1 + s * r
                    m |= (px >= left) & (px < left + s) & (py >= top) & (py < top + s)
    return m


def coverage(rows, g, frame, H, W, **params):
    """bool [H, W]: the pixels of frame number `frame` that are covered"""
    p = dict(DEFAULTS, **params)
    py, px = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    m = np.zeros((H, W), bool)
    for i in np.nonzero(g[:, 0] == frame)[0]:
        _, cx, cy, xmin, ymin, xmax, ymax, tl = (int(v) for v in g[i])
        if p["box"]:
            m |= box_mask(px, py, xmin, ymin, xmax, ymax, p["thickness"])
        for j in range(i - tl + 1, i):
            m |= segment_mask(px, py, g[j, 1:3], g[j + 1, 1:3], p["thickness"])
        m |= marker_mask(px, py, cx, cy, p["radius"])
        if p["label"]:
            m |= label_mask(px, py, rows["id"][i], xmin, ymin, p["label_scale"])
    return m


def yuv_colour(rgb):
    r, g, b = (int(v) for v in rgb)
    return (((66 * r + 129 * g + 25 * b + 128) >> 8) + 16, ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128,
            ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128)


def paint(frame, mask, pix_fmt, rgb):
    """one frame (rgb24: [H, W, 3]; nv12 / i420: [H*3//2, W]) with the covered pixels written, as a copy"""
    out = np.array(frame, np.uint8, copy=True)
    if pix_fmt == "rgb24":
        out[mask] = np.asarray(rgb, np.uint8)
        return out
    H, W = mask.shape
    Y, U, V = yuv_colour(rgb)
    flat = out.reshape(-1)
    flat[:H * W][mask.reshape(-1)] = Y
    cm = mask.reshape(H // 2, 2, W // 2, 2).any(axis=(1, 3))       # chroma sample (py >> 1, px >> 1)
    chroma = flat[H * W:]
    if pix_fmt == "nv12":
        uv = chroma.reshape(H // 2, W // 2, 2)
        uv[cm, 0], uv[cm, 1] = U, V
    else:
        assert pix_fmt == "i420", pix_fmt
        q = (H // 2) * (W // 2)
        chroma[:q].reshape(H // 2, W // 2)[cm] = U
        chroma[q:].reshape(H // 2, W // 2)[cm] = V
    return out


def frame_hw(frames, pix_fmt):
    return (frames.shape[1], frames.shape[2]) if pix_fmt == "rgb24" else (frames.shape[1] * 2 // 3, frames.shape[2])


def draw(frames, data, fps, frame0=1, frame_step=1, pix_fmt="rgb24", **params):
    """frames[i] = frame number frame0 + i * frame_step; returns the drawn copy"""
    p = dict(DEFAULTS, **params)
    rows = sorted_rows(data)
    H, W = frame_hw(frames, pix_fmt)
    g = geometry(rows, fps, H, W, p["trail"])
    if len(frames) == 0:
        return np.array(frames, np.uint8, copy=True)
    return np.stack([paint(frames[i], coverage(rows, g, frame0 + i * frame_step, H, W, **p), pix_fmt, p["rgb"]) for i in range(len(frames))])


def render(frames, data, fps, frame_stride=1, pix_fmt="rgb24", **params):
    """the kept frames of a clip (1-based number a multiple of frame_stride), drawn"""
    kept = np.asarray(frames)[frame_stride - 1::frame_stride]
    return draw(kept, data, fps, frame0=frame_stride, frame_step=frame_stride, pix_fmt=pix_fmt, **params)
