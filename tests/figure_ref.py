"""TEST INFRASTRUCTURE ONLY (numpy): the rep figure, written from the text of include/vbt_hip.h ("Rep figure"), not from the kernels.
prepare() gives the tables vbt_figure_table returns (head, points, records), render() is a per-pixel gather over the whole frame:
every pixel is tested against every record and both curves of its rectangle.  Slow and small on purpose."""
import math

import numpy as np

import overlay_hud_ref as HR
import overlay_ref as R

DEFAULTS = dict(width=1280, height=800, scale=2, thickness=2, max_figures=64, max_rows=16384, max_phases=512)
CELLS = dict(left=40, right=4, top=11, mid=13, bottom=14)
MIN_PLOT = 16
STAGE_POINTS, STAGE_RECORDS = 512, 96
TILE_W, TILE_H = 256, 32
SPAN, LINE, SWATCH, TEXT = 0, 1, 2, 3
RECORD = ("kind", "x0", "y0", "x1", "y1", "ox", "oy", "chars0", "chars1", "chars2", "value", "aux")
WHITE, INK = (255, 255, 255), (0, 0, 0)
TINT = {0: (247, 212, 212), 1: (255, 229, 207)}
CURVE = {4: (53, 25, 62), 5: (226, 75, 64), 6: (112, 31, 87), 7: (243, 118, 81)}          # x, y, dx, dy

# character codes: the digits, then the rep panel's 12..21, then the figure's own
CODES = {**{str(d): d for d in range(10)}, "R": 12, "E": 13, "P": 14, "O": 15, "M": 16, "A": 17, "C": 18, "V": 19, ".": 20, " ": 21,
         "-": 22, "/": 23, "S": 24, "X": 25, "Y": 26, "D": 27}
GLYPHS = {**{CODES[ch]: bits for ch, bits in HR.GLYPHS.items() if ch in CODES and ch != "d"},
          22: "00000 00000 00000 11111 00000 00000 00000", 25: "10001 10001 01010 00100 01010 10001 10001",
          23: "00001 00001 00010 00100 01000 10000 10000", 26: "10001 10001 01010 00100 00100 00100 00100",
          24: "01111 10000 10000 01110 00001 00001 11110", 27: "11110 10001 10001 10001 10001 10001 11110"}


def glyph(code):
    """bool [7, 5]: rows top to bottom, columns left to right"""
    return np.array([[b == "1" for b in row] for row in GLYPHS[code].split()], bool)


def geom(width, height, scale, thickness=2, **_):
    s = scale
    PW = width - (CELLS["left"] + CELLS["right"]) * s
    rest = height - (CELLS["top"] + CELLS["mid"] + CELLS["bottom"]) * s
    PH = rest // 2 if rest >= 0 else -1
    X0, Y0 = CELLS["left"] * s, CELLS["top"] * s
    return dict(W=width, H=height, s=s, t=thickness, X0=X0, Y0=Y0, Y1=Y0 + PH + CELLS["mid"] * s, PW=PW, PH=PH)


def clamp_round(v):
    v = np.float64(v)
    if not v >= -32768.0:
        return -32768
    if v > 32768.0:
        return 32768
    return int(np.rint(v))


def col(t, t0, t1, PW):
    if not t1 > t0:
        return 0
    with np.errstate(all="ignore"):
        return clamp_round((np.float64(t) - t0) / (t1 - t0) * np.float64(PW - 1))


def row(v, lo, hi, PH):
    with np.errstate(all="ignore"):
        return clamp_round((hi - np.float64(v)) / (hi - lo) * np.float64(PH - 1))


def smooth(rows):
    """float64 [T, 4]: pandas' own rolling(5, min_periods=1) means of x, y, dx, dy"""
    import pandas as pd
    rows = np.asarray(rows, np.float64).reshape(-1, 7)
    return pd.DataFrame(rows[:, 1:5]).rolling(window=5, center=False, min_periods=1).mean().to_numpy(np.float64).reshape(-1, 4)


def head(rows, sm):
    """t0, t1, position lo, hi, velocity lo, hi"""
    if len(rows) == 0:
        return np.array([0, 0, 0, 1, 0, 1], np.float64)
    m, M = sm[:, :2].min(), sm[:, :2].max()
    lo, hi = max(m - np.float64(0.2), np.float64(0.0)), min(M + np.float64(0.2), np.float64(1.0))
    if hi <= lo:
        lo, hi = m - np.float64(0.2), M + np.float64(0.2)
    vm, vM = sm[:, 2:].min(), sm[:, 2:].max()
    pad = (vM - vm) * np.float64(0.05)
    if pad == 0:
        pad = np.float64(0.5)
    return np.array([rows[0, 0], rows[-1, 0], lo, hi, vm - pad, vM + pad], np.float64)


def value_step(lo, hi):
    for decade in range(1, 8):
        for mult in (1, 2, 5):
            step = 10 ** decade * mult
            if step > 10 ** 7:
                return 0
            if (hi - lo) * np.float64(1000.0) / np.float64(step) <= 6.0:
                return step
    return 0


def centi_text(c):
    return ("-" if c < 0 else "") + f"{abs(c) // 100}.{abs(c) % 100:02d}"


def _box(kind, x0, y0, x1, y1, clip, value=0, aux=0):
    cx0, cy0, cx1, cy1 = clip
    return [kind, max(x0, cx0), max(y0, cy0), min(x1, cx1), min(y1, cy1), x0, y0, 0, 0, 0, value, aux]


def _text(s, ox, oy, text, rot, clip, value=0):
    n = len(text)
    wu, hu = (6 * n - 1) * s, 7 * s
    x1, y1 = ox + (hu if rot else wu) - 1, oy + (wu if rot else hu) - 1
    chars = [0, 0, 0]
    for k, ch in enumerate(text):
        chars[k // 4] |= CODES[ch] << (8 * (k % 4))
    cx0, cy0, cx1, cy1 = clip
    return [TEXT, max(ox, cx0), max(oy, cy0), min(x1, cx1), min(y1, cy1), ox, oy] + chars + [value, n | (rot << 8)]


def records(G, hd, phases):
    """int64 [n, 12] in table order"""
    s, W, H, X0, PW, PH = G["s"], G["W"], G["H"], G["X0"], G["PW"], G["PH"]
    t0, t1 = hd[0], hd[1]
    frame = (0, 0, W - 1, H - 1)
    Ys = (G["Y0"], G["Y1"])
    ph = np.asarray(phases, np.float64).reshape(-1, 6)
    out = []
    for i, p in enumerate(ph):
        if int(p[5]) == 2:
            continue
        c0, c1 = col(p[0], t0, t1, PW), col(p[1], t0, t1, PW)
        for Y in Ys:
            rect = (X0, Y, X0 + PW - 1, Y + PH - 1)
            out.append(_box(SPAN, X0 + c0, Y, X0 + c1, Y + PH - 1, rect, i, int(p[5])))
    for p in ph:
        if int(p[5]) != 0:
            continue
        dur = p[1] - p[0]
        with np.errstate(all="ignore"):
            cc = col((p[0] + p[1]) / np.float64(2.0), t0, t1, PW)
            vals = (HR.centi(p[4]), HR.centi(p[4] / dur) if dur > 0 else 0)
        for Y, v in zip(Ys, vals):
            out.append(_text(s, X0 + cc - 3 * s, Y + 2 * s, centi_text(v), 1, (X0, Y, X0 + PW - 1, Y + PH - 1), v))
    for k, Y in enumerate(Ys):
        out.append(_box(LINE, X0 - s, Y - s, X0 + PW + s - 1, Y - 1, frame))
        out.append(_box(LINE, X0 - s, Y + PH, X0 + PW + s - 1, Y + PH + s - 1, frame))
        out.append(_box(LINE, X0 - s, Y, X0 - 1, Y + PH - 1, frame))
        out.append(_box(LINE, X0 + PW, Y, X0 + PW + s - 1, Y + PH - 1, frame))
        out.append(_text(s, X0, Y - 9 * s, "ACV M/S" if k else "ROM M", 0, frame))
        for j, kc in enumerate((48, 70)):
            kx = X0 + kc * s
            out.append(_box(SWATCH, kx, Y - 7 * s, kx + 6 * s - 1, Y - 4 * s - 1, frame, 0, 4 + 2 * k + j))
            out.append(_text(s, kx + 7 * s, Y - 9 * s, ("X", "Y", "DX", "DY")[2 * k + j], 0, frame))
        lo, hi = hd[2 + 2 * k], hd[3 + 2 * k]
        step = value_step(lo, hi) if lo >= -1e9 and hi <= 1e9 else 0
        if step:
            k0 = math.floor(lo * np.float64(1000.0) / np.float64(step)) - 1
            for kk in range(k0, k0 + 10):
                milli = kk * step
                v = np.float64(milli) / np.float64(1000.0)
                if not lo <= v <= hi:
                    continue
                r = row(v, lo, hi, PH)
                c = max(-9999, min(9999, milli // 10))                  # (milli is a multiple of 10)
                out.append(_box(LINE, X0 - 3 * s, Y + r - s // 2, X0 - s - 1, Y + r - s // 2 + s - 1, frame, c))
                txt = centi_text(c)
                out.append(_text(s, X0 - 4 * s - (6 * len(txt) - 1) * s, Y + r - 3 * s, txt, 0, frame, c))
    if t0 >= -1e9 and t1 <= 1e9:
        u = 1
        while np.float64(u) * 256.0 < t1 - t0:
            u *= 10
        i0 = math.floor(t0)
        base = i0 - i0 % (5 * u)
        top = G["Y1"] + PH + s
        for k in range(264):
            sec = base + k * u
            if sec > t1:
                break
            if sec < t0:
                continue
            major = (sec - base) % (5 * u) == 0
            c = col(np.float64(sec), t0, t1, PW)
            out.append(_box(LINE, X0 + c - s // 2, top, X0 + c - s // 2 + s - 1, top + (3 if major else 2) * s - 1, frame, sec, int(major)))
            if major:
                txt = str(sec)
                out.append(_text(s, X0 + c - ((6 * len(txt) - 1) * s) // 2, top + 4 * s, txt, 0, frame, sec))
    return np.array(out, np.int64).reshape(-1, 12)


def prepare(rows, phases, **params):
    """(head float64 [6], points int64 [T, 5], records int64 [n, 12]) of one figure"""
    G = geom(**dict(DEFAULTS, **params))
    rows = np.asarray(rows, np.float64).reshape(-1, 7)
    sm = smooth(rows)
    hd = head(rows, sm)
    pts = np.zeros((len(rows), 5), np.int64)
    for i in range(len(rows)):
        pts[i, 0] = col(rows[i, 0], hd[0], hd[1], G["PW"])
        for k in range(4):
            pts[i, 1 + k] = row(sm[i, k], hd[2 + 2 * (k // 2)], hd[3 + 2 * (k // 2)], G["PH"])
    return hd, pts, records(G, hd, phases)


def text_mask(px, py, r, s):
    n, rot = int(r[11]) & 255, int(r[11]) >> 8
    wu = (6 * n - 1) * s
    m = np.zeros(px.shape, bool)
    for k in range(n):
        bits = glyph((int(r[7 + k // 4]) >> (8 * (k % 4))) & 255)
        for rr in range(7):
            for c in range(5):
                if not bits[rr, c]:
                    continue
                ux, uy = 6 * s * k + s * c, s * rr                    # the block in the text not turned
                if rot:                                               # (ux, uy) -> (uy, wu - 1 - ux): the block's columns become rows
                    m |= (px >= r[5] + uy) & (px < r[5] + uy + s) & (py > r[6] + wu - 1 - ux - s) & (py <= r[6] + wu - 1 - ux)
                else:
                    m |= (px >= r[5] + ux) & (px < r[5] + ux + s) & (py >= r[6] + uy) & (py < r[6] + uy + s)
    return m & (px >= r[1]) & (px <= r[3]) & (py >= r[2]) & (py <= r[4])


def curve_mask(qx, qy, pts, which, t):
    """rule 2 over every segment of a series, rectangle coordinates"""
    m = np.zeros(qx.shape, bool)
    T = len(pts)
    for i in range(max(T - 1, 1) if T else 0):
        j = min(i + 1, T - 1)
        m |= R.segment_mask(qx, qy, (pts[i, 0], pts[i, which]), (pts[j, 0], pts[j, which]), t)
    return m


def render_one(hd, pts, recs, **params):
    """uint8 [H, W, 3] from the tables"""
    G = geom(**dict(DEFAULTS, **params))
    W, H, s = G["W"], G["H"], G["s"]
    py, px = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    out = np.empty((H, W, 3), np.uint8)
    out[:] = WHITE
    for r in recs:                                                    # spans in table order: the later phase overwrites
        if r[0] == SPAN:
            out[(px >= r[1]) & (px <= r[3]) & (py >= r[2]) & (py <= r[4])] = TINT[int(r[11])]
    for r in recs:
        if r[0] in (LINE, SWATCH):
            out[(px >= r[1]) & (px <= r[3]) & (py >= r[2]) & (py <= r[4])] = INK if r[0] == LINE else CURVE[int(r[11])]
    for k, Y in enumerate((G["Y0"], G["Y1"])):
        inside = (px >= G["X0"]) & (px < G["X0"] + G["PW"]) & (py >= Y) & (py < Y + G["PH"])
        for which in (1 + 2 * k, 2 + 2 * k):                          # the first curve, then the second over it
            out[inside & curve_mask(px - G["X0"], py - Y, pts, which, G["t"])] = CURVE[3 + which]
    for r in recs:
        if r[0] == TEXT:
            out[text_mask(px, py, r, s)] = INK
    return out


def render(figures, **params):
    """uint8 [N, H, W, 3]: figures = [(rows [T, 7], phases [P, 6]), ...]"""
    return np.stack([render_one(*prepare(rows, phases, **params), **params) for rows, phases in figures])


def staged(pts, recs, **params):
    """does every tile of the figure keep its points / its records in LDS (the header's "Staging")"""
    G = geom(**dict(DEFAULTS, **params))
    h = (G["t"] + 1) // 2
    pts_ok = recs_ok = True
    for x_lo in range(0, G["W"], TILE_W):
        x_hi = min(x_lo + TILE_W, G["W"]) - 1
        if len(pts):
            c = pts[:, 0]
            k0, k1 = int(np.searchsorted(c, x_lo - G["X0"] - h, "left")), int(np.searchsorted(c, x_hi - G["X0"] + h + 1, "left"))
            seg0, seg1 = max(k0 - 1, 0), min(k1 - 1, max(len(c) - 1, 1) - 1)
            if seg0 <= seg1 and min(seg1 + 1, len(c) - 1) - seg0 + 1 > STAGE_POINTS:
                pts_ok = False
        for y_lo in range(0, G["H"], TILE_H):
            y_hi = min(y_lo + TILE_H, G["H"]) - 1
            n = sum(1 for r in recs if r[1] <= r[3] and r[2] <= r[4] and r[1] <= x_hi and r[3] >= x_lo and r[2] <= y_hi and r[4] >= y_lo)
            if n > STAGE_RECORDS:
                recs_ok = False
    return pts_ok, recs_ok
