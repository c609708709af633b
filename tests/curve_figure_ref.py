"""TEST INFRASTRUCTURE ONLY (numpy): the curve figure, written from the text of include/vbt_hip.h ("Curve figure"), not from the kernels.
A figure is a dict: series = [(xy float64 [n, 2], legend text, palette index), ...], marks = [(series, point, text), ...], x_title,
y_title, corner (0 lower left, 1 lower right), minor_x, minor_y (thousandths, 0 none).  prepare() gives the tables
vbt_curve_figure_table returns (counts, MERGED points, records); render_one() paints the UNMERGED polyline: every finite point a dot,
every two consecutive finite points a segment.  Slow and small on purpose."""
import numpy as np

import overlay_ref as R

DEFAULTS = dict(width=1120, height=640, scale=2, thickness=2, max_figures=16, max_series=8, max_points=131072, max_marks=8)
CELLS = dict(left=30, right=4, top=4, bottom=22)
MIN_PLOT = 16
STAGE_POINTS, STAGE_RECORDS = 384, 64
TILE_W, TILE_H = 256, 8
LEGEND_TEXT, SWATCH, LEGEND_BOX, MARK_TEXT, MARKER, LEADER, CURVES, LINE, TEXT, GRID_MAJOR, GRID_MINOR = range(11)
RECORD = ("kind", "x0", "y0", "x1", "y1", "ox", "oy", "value", "aux", "n", "pad0", "pad1") + tuple(f"chars{k}" for k in range(16))
WHITE, INK, MAJOR, MINOR, BORDER = (255, 255, 255), (0, 0, 0), (176, 176, 176), (204, 204, 204), (128, 128, 128)
PALETTE = ((31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194), (127, 127, 127),
           (188, 189, 34), (23, 190, 207))
LOWER_LEFT, LOWER_RIGHT = 0, 1

FONT = {ch: bits for ch, bits in (line.split(" ", 1) for line in """\
! 00100 00100 00100 00100 00100 00000 00100
" 01010 01010 01010 00000 00000 00000 00000
# 01010 01010 11111 01010 11111 01010 01010
$ 00100 01111 10100 01110 00101 11110 00100
% 11000 11001 00010 00100 01000 10011 00011
& 01100 10010 10100 01000 10101 10010 01101
' 00100 00100 01000 00000 00000 00000 00000
( 00010 00100 01000 01000 01000 00100 00010
) 01000 00100 00010 00010 00010 00100 01000
* 00000 00100 10101 01110 10101 00100 00000
+ 00000 00100 00100 11111 00100 00100 00000
, 00000 00000 00000 00000 01100 00100 01000
- 00000 00000 00000 11111 00000 00000 00000
. 00000 00000 00000 00000 00000 01100 01100
/ 00001 00001 00010 00100 01000 10000 10000
0 01110 10001 10011 10101 11001 10001 01110
1 00100 01100 00100 00100 00100 00100 01110
2 01110 10001 00001 00010 00100 01000 11111
3 11111 00010 00100 00010 00001 10001 01110
4 00010 00110 01010 10010 11111 00010 00010
5 11111 10000 11110 00001 00001 10001 01110
6 00110 01000 10000 11110 10001 10001 01110
7 11111 00001 00010 00100 01000 01000 01000
8 01110 10001 10001 01110 10001 10001 01110
9 01110 10001 10001 01111 00001 00010 01100
: 00000 01100 01100 00000 01100 01100 00000
; 00000 01100 01100 00000 01100 00100 01000
< 00010 00100 01000 10000 01000 00100 00010
= 00000 00000 11111 00000 11111 00000 00000
> 01000 00100 00010 00001 00010 00100 01000
? 01110 10001 00001 00010 00100 00000 00100
@ 01110 10001 00001 01101 10101 10101 01110
A 01110 10001 10001 11111 10001 10001 10001
B 11110 10001 10001 11110 10001 10001 11110
C 01110 10001 10000 10000 10000 10001 01110
D 11110 10001 10001 10001 10001 10001 11110
E 11111 10000 10000 11110 10000 10000 11111
F 11111 10000 10000 11110 10000 10000 10000
G 01110 10001 10000 10111 10001 10001 01111
H 10001 10001 10001 11111 10001 10001 10001
I 01110 00100 00100 00100 00100 00100 01110
J 00111 00010 00010 00010 00010 10010 01100
K 10001 10010 10100 11000 10100 10010 10001
L 10000 10000 10000 10000 10000 10000 11111
M 10001 11011 10101 10101 10001 10001 10001
N 10001 10001 11001 10101 10011 10001 10001
O 01110 10001 10001 10001 10001 10001 01110
P 11110 10001 10001 11110 10000 10000 10000
Q 01110 10001 10001 10001 10101 10010 01101
R 11110 10001 10001 11110 10100 10010 10001
S 01111 10000 10000 01110 00001 00001 11110
T 11111 00100 00100 00100 00100 00100 00100
U 10001 10001 10001 10001 10001 10001 01110
V 10001 10001 10001 10001 10001 01010 00100
W 10001 10001 10001 10101 10101 10101 01010
X 10001 10001 01010 00100 01010 10001 10001
Y 10001 10001 01010 00100 00100 00100 00100
Z 11111 00001 00010 00100 01000 10000 11111
[ 01110 01000 01000 01000 01000 01000 01110
\\ 10000 10000 01000 00100 00010 00001 00001
] 01110 00010 00010 00010 00010 00010 01110
^ 00100 01010 10001 00000 00000 00000 00000
_ 00000 00000 00000 00000 00000 00000 11111
` 01000 00100 00010 00000 00000 00000 00000
a 00000 00000 01110 00001 01111 10001 01111
b 10000 10000 10110 11001 10001 10001 11110
c 00000 00000 01110 10000 10000 10001 01110
d 00001 00001 01101 10011 10001 10001 01111
e 00000 00000 01110 10001 11111 10000 01110
f 00110 01001 01000 11100 01000 01000 01000
g 00000 01111 10001 10001 01111 00001 01110
h 10000 10000 10110 11001 10001 10001 10001
i 00100 00000 01100 00100 00100 00100 01110
j 00010 00000 00110 00010 00010 10010 01100
k 10000 10000 10010 10100 11000 10100 10010
l 01100 00100 00100 00100 00100 00100 01110
m 00000 00000 11010 10101 10101 10001 10001
n 00000 00000 10110 11001 10001 10001 10001
o 00000 00000 01110 10001 10001 10001 01110
p 00000 00000 11110 10001 11110 10000 10000
q 00000 00000 01101 10011 01111 00001 00001
r 00000 00000 10110 11001 10000 10000 10000
s 00000 00000 01110 10000 01110 00001 11110
t 01000 01000 11100 01000 01000 01001 00110
u 00000 00000 10001 10001 10001 10011 01101
v 00000 00000 10001 10001 10001 01010 00100
w 00000 00000 10001 10001 10101 10101 01010
x 00000 00000 10001 01010 00100 01010 10001
y 00000 00000 10001 10001 01111 00001 01110
z 00000 00000 11111 00010 00100 01000 11111
{ 00010 00100 00100 01000 00100 00100 00010
| 00100 00100 00100 00100 00100 00100 00100
} 01000 00100 00100 00010 00100 00100 01000
~ 00000 00000 01000 10101 00010 00000 00000""".split("\n"))}
FONT[" "] = "00000 00000 00000 00000 00000 00000 00000"


def glyph(ch):
    """bool [7, 5]: rows top to bottom, columns left to right"""
    return np.array([[b == "1" for b in row] for row in FONT[ch].split()], bool)


def figure(series=(), marks=(), x_title="", y_title="", corner=LOWER_LEFT, minor_x=0, minor_y=0):
    return dict(series=[(np.asarray(xy, np.float64).reshape(-1, 2), str(text), int(colour)) for xy, text, colour in series],
                marks=[(int(s), int(p), str(t)) for s, p, t in marks], x_title=x_title, y_title=y_title, corner=int(corner),
                minor_x=int(minor_x), minor_y=int(minor_y))


def geom(width, height, scale, thickness=2, **_):
    s = scale
    return dict(W=width, H=height, s=s, t=thickness, X0=CELLS["left"] * s, Y0=CELLS["top"] * s,
                PW=width - (CELLS["left"] + CELLS["right"]) * s, PH=height - (CELLS["top"] + CELLS["bottom"]) * s)


def clamp_round(v):
    v = np.float64(v)
    if not v >= -32768.0:
        return -32768
    if v > 32768.0:
        return 32768
    return int(np.rint(v))


def col(x, PW):
    with np.errstate(all="ignore"):
        return clamp_round(np.float64(x) / np.float64(1.01) * np.float64(PW - 1))


def row(y, PH):
    with np.errstate(all="ignore"):
        return clamp_round((np.float64(1.01) - np.float64(y)) / np.float64(1.01) * np.float64(PH - 1))


def ordered(xy):
    """the points in drawing order: as given when x over the finite points never decreases, reversed when it never increases;
    ValueError("point i") for a series that is neither"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    fin = np.isfinite(xy).all(axis=1)
    idx = np.nonzero(fin)[0]
    direction = 0
    for a, b in zip(idx[:-1], idx[1:]):
        if xy[b, 0] == xy[a, 0]:
            continue
        d = 1 if xy[b, 0] > xy[a, 0] else -1
        if direction == 0:
            direction = d
        elif d != direction:
            raise ValueError(f"point {b}: x is not monotone")
    return xy[::-1] if direction < 0 else xy


def polyline(xy, G):
    """int64 [m, 3]: the UNMERGED points of a series - (column, row, join) of every finite point, join = the point before it is finite"""
    xy = ordered(xy)
    fin = np.isfinite(xy).all(axis=1)
    out = []
    for i in range(len(xy)):
        if fin[i]:
            out.append((col(xy[i, 0], G["PW"]), row(xy[i, 1], G["PH"]), int(i > 0 and fin[i - 1])))
    return np.array(out, np.int64).reshape(-1, 3)


def merge(poly):
    """the run merge on an unmerged table: of every maximal stretch of joined points of one column keep the first, the last, the first
    of the lowest rows and the first of the highest rows, in order"""
    out, i, m = [], 0, len(poly)
    while i < m:
        j = i + 1
        while j < m and poly[j, 2] == 1 and poly[j, 0] == poly[i, 0]:
            j += 1
        rows = poly[i:j, 1]
        keep = sorted({i, j - 1, i + int(np.argmin(rows)), i + int(np.argmax(rows))})
        out += [tuple(poly[k]) for k in keep]
        i = j
    return np.array(out, np.int64).reshape(-1, 3)


def _box(kind, x0, y0, x1, y1, clip, value=0, aux=0):
    cx0, cy0, cx1, cy1 = clip
    return [kind, max(x0, cx0), max(y0, cy0), min(x1, cx1), min(y1, cy1), x0, y0, value, aux, 0, 0, 0] + [0] * 16


def _text(kind, s, ox, oy, text, rot, clip, value=0):
    n = len(text)
    wu, hu = (6 * n - 1) * s, 7 * s
    x1, y1 = ox + (hu if rot else wu) - 1, oy + (wu if rot else hu) - 1
    chars = [0] * 16
    for k, ch in enumerate(text):
        chars[k // 4] |= ord(ch) << (8 * (k % 4))
    chars = [c - (1 << 32) if c >= 1 << 31 else c for c in chars]
    cx0, cy0, cx1, cy1 = clip
    return [kind, max(ox, cx0), max(oy, cy0), min(x1, cx1), min(y1, cy1), ox, oy, value, rot, n, 0, 0] + chars


def records(G, fig):
    """int64 [n, 28] in table order"""
    s, W, H, X0, Y0, PW, PH = G["s"], G["W"], G["H"], G["X0"], G["Y0"], G["PW"], G["PH"]
    b = (s + 1) // 2
    frame, plot = (0, 0, W - 1, H - 1), (X0, Y0, X0 + PW - 1, Y0 + PH - 1)
    out = [_box(LINE, X0 - s, Y0, X0 - 1, Y0 + PH + s - 1, frame), _box(LINE, X0, Y0 + PH, X0 + PW - 1, Y0 + PH + s - 1, frame)]

    def grid(kind, axis, milli):
        v = np.float64(milli) / np.float64(1000.0)
        if axis == 0:
            x = X0 + col(v, PW)
            return _box(kind, x, Y0, x + b - 1, Y0 + PH - 1, plot, milli, 0)
        y = Y0 + row(v, PH)
        return _box(kind, X0, y, X0 + PW - 1, y + b - 1, plot, milli, 1)
    for axis in (0, 1):
        for k in range(6):
            milli = 200 * k
            v = np.float64(milli) / np.float64(1000.0)
            label = f"{k // 5}.{2 * k % 10}"
            if axis == 0:
                x = X0 + col(v, PW)
                out.append(_box(LINE, x - s // 2, Y0 + PH + s, x - s // 2 + s - 1, Y0 + PH + 4 * s - 1, frame, milli, 0))
                out.append(_text(TEXT, s, x - (17 * s) // 2, Y0 + PH + 5 * s, label, 0, frame, milli))
            else:
                y = Y0 + row(v, PH)
                out.append(_box(LINE, X0 - 4 * s, y - s // 2, X0 - s - 1, y - s // 2 + s - 1, frame, milli, 1))
                out.append(_text(TEXT, s, X0 - 22 * s, y - 3 * s, label, 0, frame, milli))
            out.append(grid(GRID_MAJOR, axis, milli))
    for axis, step in ((0, fig["minor_x"]), (1, fig["minor_y"])):
        if step > 0:
            out += [grid(GRID_MINOR, axis, m) for m in range(step, 1001, step) if m % 200]
    nx, ny = len(fig["x_title"]), len(fig["y_title"])
    if nx:
        out.append(_text(TEXT, s, X0 + (PW - (6 * nx - 1) * s) // 2, Y0 + PH + 14 * s, fig["x_title"], 0, frame))
    if ny:
        out.append(_text(TEXT, s, s, Y0 + (PH - (6 * ny - 1) * s) // 2, fig["y_title"], 1, frame))
    K = len(fig["series"])
    if K:
        L = max(len(t) for _, t, _ in fig["series"])
        BW, BH = ((6 * L - 1) * s if L else 0) + 16 * s, 9 * s * K + 4 * s
        bx = X0 + PW - 3 * s - BW if fig["corner"] == LOWER_RIGHT else X0 + 3 * s
        by = Y0 + PH - 3 * s - BH
        out.append(_box(LEGEND_BOX, bx, by, bx + BW - 1, by + BH - 1, frame, BW, BH))
        for k, (_, text, colour) in enumerate(fig["series"]):
            ty = by + 3 * s + 9 * s * k
            out.append(_box(SWATCH, bx + 3 * s, ty + 2 * s, bx + 11 * s - 1, ty + 5 * s - 1, frame, k, colour))
            out.append(_text(LEGEND_TEXT, s, bx + 13 * s, ty, text, 0, frame, k))
    M = len(fig["marks"])
    for i, (sr, pt, text) in enumerate(fig["marks"]):
        p = fig["series"][sr][0][pt]
        if not np.isfinite(p).all():
            none = (0, 0, -1, -1)
            out += [_text(MARK_TEXT, s, 0, 0, text, 0, none, i), _box(MARKER, 0, 0, -1, -1, none), _box(LEADER, 0, 0, -1, -1, none)]
            continue
        px, py, wu, rad = X0 + col(p[0], PW), Y0 + row(p[1], PH), (6 * len(text) - 1) * s, 2 * s
        if fig["corner"] == LOWER_RIGHT:
            ax, ay = px + (M - i) * 6 * s, py + (i + 1) * 10 * s
            ox = ax
        else:
            ax, ay = px - 8 * s, py + (min(i, 3) + 1) * 10 * s
            ox = ax - wu + 1
        out.append(_text(MARK_TEXT, s, ox, ay, text, 0, frame, i))
        out.append(_box(MARKER, px - rad, py - rad, px + rad, py + rad, frame, px, py))
        out.append([LEADER, max(min(ax, px) - 1, 0), max(min(ay, py) - 1, 0), min(max(ax, px) + 1, W - 1), min(max(ay, py) + 1, H - 1), ax, ay, px, py,
                    0, 0, 0] + [0] * 16)
    return np.array(out, np.int64).reshape(-1, 28)


def prepare(fig, **params):
    """(counts int64 [K], merged points int64 [sum, 3], records int64 [n, 28]) of one figure"""
    G = geom(**dict(DEFAULTS, **params))
    merged = [merge(polyline(xy, G)) for xy, _, _ in fig["series"]]
    pts = np.concatenate(merged) if merged else np.zeros((0, 3), np.int64)
    return np.array([len(m) for m in merged], np.int64), pts.reshape(-1, 3), records(G, fig)


def text_mask(px, py, r, s):
    n, rot = int(r[9]), int(r[8])
    wu = (6 * n - 1) * s
    m = np.zeros(px.shape, bool)
    for k in range(n):
        bits = glyph(chr((int(r[12 + k // 4]) >> (8 * (k % 4))) & 255))
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


def curve_mask(G, table):
    """bool [PH, PW]: rule 2 over a point table (merged or not) in rectangle coordinates - every point a dot, every joined point a segment
    from the point before it.  Each test runs on the segment's box widened by (t + 1) / 2 only: nothing outside it is within t / 2."""
    PW, PH, t = G["PW"], G["PH"], G["t"]
    h = (t + 1) // 2
    m = np.zeros((PH, PW), bool)
    for i in range(len(table)):
        a = table[i - 1] if table[i, 2] else table[i]
        b = table[i]
        x0, x1 = max(min(a[0], b[0]) - h, 0), min(max(a[0], b[0]) + h, PW - 1)
        y0, y1 = max(min(a[1], b[1]) - h, 0), min(max(a[1], b[1]) + h, PH - 1)
        if x0 > x1 or y0 > y1:
            continue
        qy, qx = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
        m[y0:y1 + 1, x0:x1 + 1] |= R.segment_mask(qx, qy, (int(a[0]), int(a[1])), (int(b[0]), int(b[1])), t)
    return m


def render_one(fig, merged=False, **params):
    """uint8 [H, W, 3]: the records by rising priority, the curves (UNMERGED unless merged=True) in their place"""
    G = geom(**dict(DEFAULTS, **params))
    W, H, s = G["W"], G["H"], G["s"]
    b = (s + 1) // 2
    recs = records(G, fig)
    py, px = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    out = np.empty((H, W, 3), np.uint8)
    out[:] = WHITE

    def box(r):
        return (px >= r[1]) & (px <= r[3]) & (py >= r[2]) & (py <= r[4])
    for kind in (GRID_MINOR, GRID_MAJOR, TEXT, LINE, CURVES, LEADER, MARKER, MARK_TEXT, LEGEND_BOX, SWATCH, LEGEND_TEXT):
        if kind == CURVES:
            for xy, _, colour in fig["series"]:                        # the later series over the earlier
                table = polyline(xy, G)
                out[G["Y0"]:G["Y0"] + G["PH"], G["X0"]:G["X0"] + G["PW"]][curve_mask(G, merge(table) if merged else table)] = PALETTE[colour]
            continue
        for r in recs[recs[:, 0] == kind]:
            if kind in (TEXT, MARK_TEXT, LEGEND_TEXT):
                out[text_mask(px, py, r, s)] = INK
            elif kind == LINE:
                out[box(r)] = INK
            elif kind == GRID_MAJOR:
                out[box(r)] = MAJOR
            elif kind == GRID_MINOR:
                along = px - r[5] if r[8] else py - r[6]
                out[box(r) & ((along // b) % 3 == 0)] = MINOR
            elif kind == LEADER:
                out[box(r) & R.segment_mask(px, py, (int(r[5]), int(r[6])), (int(r[7]), int(r[8])), 1)] = INK
            elif kind == MARKER:
                out[box(r) & ((px - r[7]) ** 2 + (py - r[8]) ** 2 <= (2 * s) ** 2)] = INK
            elif kind == LEGEND_BOX:
                rx, ry = px - r[5], py - r[6]
                edge = (rx < b) | (ry < b) | (rx >= r[7] - b) | (ry >= r[8] - b)
                out[box(r) & edge] = BORDER
                out[box(r) & ~edge] = WHITE
            elif kind == SWATCH:
                out[box(r)] = PALETTE[int(r[8])]
    return out


def staged(counts, pts, recs, **params):
    """does every tile of the figure keep its merged points / its records in LDS (the header's "Staging"); the render reads LDS only
    when both hold"""
    G = geom(**dict(DEFAULTS, **params))
    h = (G["t"] + 1) // 2
    pts_ok = recs_ok = True
    for x_lo in range(0, G["W"], TILE_W):
        x_hi = min(x_lo + TILE_W, G["W"]) - 1
        total, at = 0, 0
        for m in counts:
            c = pts[at:at + m, 0]
            at += m
            if m == 0:
                continue
            k0, k1 = int(np.searchsorted(c, x_lo - G["X0"] - h, "left")), int(np.searchsorted(c, x_hi - G["X0"] + h + 1, "left"))
            i0, i1 = k0, min(k1, m - 1)
            if i0 <= i1:
                total += i1 - max(i0 - 1, 0) + 1
        if total > STAGE_POINTS:
            pts_ok = False
        for y_lo in range(0, G["H"], TILE_H):
            y_hi = min(y_lo + TILE_H, G["H"]) - 1
            n = sum(1 for r in recs if r[1] <= r[3] and r[2] <= r[4] and r[1] <= x_hi and r[3] >= x_lo and r[2] <= y_hi and r[4] >= y_lo)
            if n > STAGE_RECORDS:
                recs_ok = False
    return pts_ok, recs_ok
