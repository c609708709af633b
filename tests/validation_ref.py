"""TEST INFRASTRUCTURE ONLY (numpy): the validation figure, written from the text of include/vbt_hip.h ("Validation figure"), not from
the kernels.  A pair is (ref float64 [N, 3] time, x, y; rows float64 [T, 5] time, x, y, norm_plate_height, norm_plate_width; kind
"kinovea" | "qualisys").  numbers() gives what vbt_validation_stats and the double tables of vbt_validation_table return - every sum
in the header's fixed order (fsum) -, prepare() all tables, render_one() paints the UNMERGED polylines.  Slow and small on purpose."""
import numpy as np

import curve_figure_ref as CR
import figure_ref as FR
import overlay_ref as R

DEFAULTS = dict(width=1280, height=640, scale=2, thickness=2, max_pairs=64, max_rows=4096, max_ref_rows=4096, max_grid=4096)
CELLS = dict(left=50, right=4, top=17, mid=6, bottom=23)
MIN_PLOT = 16
STAGE_POINTS, STAGE_RECORDS = 768, 64
TILE_W, TILE_H = 256, 8
LANES = 256
KINDS = {"kinovea": 0, "qualisys": 1}
STATS = ("mse_x", "mse_y", "r_x", "r_y", "n", "t_min", "t_max", "flags")
TRUTH, TRACKER = (53, 25, 62), (243, 118, 81)
LEGEND_TEXT, SWATCH, LEGEND_BOX, LINE, TEXT = CR.LEGEND_TEXT, CR.SWATCH, CR.LEGEND_BOX, CR.LINE, CR.TEXT
RECORD = CR.RECORD
F = np.float64


def fsum(v):
    """the header's sum: 256 partial sums over l, l + 256, ... in rising order, then a halving tree over the 256"""
    v = np.asarray(v, F).reshape(-1)
    k = -(-len(v) // LANES)
    a = np.zeros(k * LANES, F)
    a[:len(v)] = v
    p = np.zeros(LANES, F)
    for r in a.reshape(k, LANES):
        p = p + r
    h = LANES // 2
    while h:
        p[:h] = p[:h] + p[h:2 * h]
        h //= 2
    return p[0]


def window_means(rows, kind):
    """float64 [T, 4]: x, y, height, width through pandas' own windows - kinovea (5, 5, expanding, expanding), qualisys (copy, copy, 30, 30)"""
    import pandas as pd
    out = np.empty((len(rows), 4), F)
    for c in range(4):
        s = pd.Series(rows[:, 1 + c])
        if kind == "kinovea":
            out[:, c] = (s.rolling(window=5, center=False, min_periods=1) if c < 2 else s.expanding(min_periods=1)).mean().to_numpy()
        else:
            out[:, c] = rows[:, 1 + c] if c < 2 else s.rolling(window=30, center=False, min_periods=1).mean().to_numpy()
    return out


def interp(t, v, ts):
    hi = np.clip(np.searchsorted(t, ts, "left"), 1, len(t) - 1)
    lo = hi - 1
    slope = (v[hi] - v[lo]) / (t[hi] - t[lo])
    return slope * (ts - t[lo]) + v[lo]


def numbers(ref, rows, kind, plate=0.45, rate=30.0):
    """(aligned trajectory [T, 3], grid [n, 5], stats [8])"""
    ref, rows = np.asarray(ref, F).reshape(-1, 3), np.asarray(rows, F).reshape(-1, 5)
    plate, rate = F(plate), F(rate)
    sm = window_means(rows, kind)
    x = sm[:, 0] * plate / sm[:, 3]
    y = -sm[:, 1] * plate / sm[:, 2]
    y = y + (fsum(ref[:, 2]) / F(len(ref)) - fsum(y) / F(len(y)))
    x = x + (fsum(ref[:, 1]) / F(len(ref)) - fsum(x) / F(len(x)))
    traj = np.stack([rows[:, 0], x, y], axis=1)
    t_max, t_min = min(ref[-1, 0], rows[-1, 0]), max(ref[0, 0], rows[0, 0])
    n = int(t_max * rate)
    step = (t_max - t_min) / F(n - 1)
    ts = np.arange(n).astype(F) * step + t_min
    ts[-1] = t_max
    grid = np.stack([ts, interp(ref[:, 0], ref[:, 1], ts), interp(traj[:, 0], traj[:, 1], ts), interp(ref[:, 0], ref[:, 2], ts),
                     interp(traj[:, 0], traj[:, 2], ts)], axis=1)
    stats = np.zeros(8, F)
    flags = 0
    with np.errstate(all="ignore"):
        for a in range(2):
            ga, gb = grid[:, 1 + 2 * a], grid[:, 2 + 2 * a]
            stats[a] = fsum((ga - gb) * (ga - gb)) / F(n)
            ma, mb = fsum(ga) / F(n), fsum(gb) / F(n)
            na, nb = np.sqrt(fsum((ga - ma) * (ga - ma))), np.sqrt(fsum((gb - mb) * (gb - mb)))
            dot = fsum(((ga - ma) / na) * ((gb - mb) / nb))
            if np.isnan(dot):
                flags |= 1 << a
            else:
                dot = max(min(dot, F(1.0)), F(-1.0))
            stats[2 + a] = dot
    stats[4:] = [n, t_min, t_max, flags]
    return traj, grid, stats


def geom(width, height, scale, thickness=2, **_):
    s = scale
    PH = (height - (CELLS["top"] + CELLS["mid"] + CELLS["bottom"]) * s) // 2 if height >= (CELLS["top"] + CELLS["mid"] + CELLS["bottom"]) * s else -1
    Y0 = CELLS["top"] * s
    return dict(W=width, H=height, s=s, t=thickness, X0=CELLS["left"] * s, Y0=Y0, Y1=Y0 + PH + CELLS["mid"] * s,
                PW=width - (CELLS["left"] + CELLS["right"]) * s, PH=PH)


def head(kind, ref, traj):
    """time lo, hi, X lo, hi, Y lo, hi"""
    lim = []
    for a in (1, 2):
        m, M = min(ref[:, a].min(), traj[:, a].min()), max(ref[:, a].max(), traj[:, a].max())
        d = M - m
        e = F(0.05) * d if d != 0 else F(0.05)
        lim.append([m - e, M + e])
    (loX, hiX), (loY, hiY) = lim
    dX, dY = hiX - loX, hiY - loY
    if (dX < dY) if kind == "kinovea" else not dX > dY:
        loX, hiX = loX - dY / F(2.0), hiX + dY / F(2.0)
    elif kind == "qualisys":
        loY, hiY = loY - dX / F(2.0), hiY + dX / F(2.0)
    return np.array([0.0, max(ref[-1, 0], traj[-1, 0]), loX, hiX, loY, hiY], F)


def series(ref, traj):
    """the four series as (times, values, panel): ref x, tracker x, ref y, tracker y"""
    return [(ref[:, 0], ref[:, 1], 0), (traj[:, 0], traj[:, 1], 0), (ref[:, 0], ref[:, 2], 1), (traj[:, 0], traj[:, 2], 1)]


def polyline(t, v, hd, panel, G):
    """int64 [n, 3]: the UNMERGED points of a series - (column, row, join) of every point"""
    lo, hi = hd[2 + 2 * panel], hd[3 + 2 * panel]
    return np.array([(FR.col(t[i], F(0.0), hd[1], G["PW"]), FR.row(v[i], lo, hi, G["PH"]), int(i > 0)) for i in range(len(t))], np.int64).reshape(-1, 3)


def records(G, kind, hd):
    """int64 [n, 28] in table order"""
    s, W, H, X0, PW, PH = G["s"], G["W"], G["H"], G["X0"], G["PW"], G["PH"]
    frame = (0, 0, W - 1, H - 1)
    out = []
    for k, Y in enumerate((G["Y0"], G["Y1"])):
        out += [CR._box(LINE, X0 - s, Y - s, X0 + PW + s - 1, Y - 1, frame), CR._box(LINE, X0 - s, Y + PH, X0 + PW + s - 1, Y + PH + s - 1, frame),
                CR._box(LINE, X0 - s, Y, X0 - 1, Y + PH - 1, frame), CR._box(LINE, X0 + PW, Y, X0 + PW + s - 1, Y + PH - 1, frame)]
        lo, hi = hd[2 + 2 * k], hd[3 + 2 * k]
        step = FR.value_step(lo, hi) if lo >= -1e9 and hi <= 1e9 else 0
        if step:
            k0 = int(np.floor(lo * F(1000.0) / F(step))) - 1
            for kk in range(k0, k0 + 10):
                milli = kk * step
                v = F(milli) / F(1000.0)
                if not (lo <= v <= hi):
                    continue
                row = FR.row(v, lo, hi, PH)
                c = max(min(int(abs(milli) // 10) * (1 if milli >= 0 else -1), 9999), -9999)
                text = FR.centi_text(c)
                out.append(CR._box(LINE, X0 - 3 * s, Y + row - s // 2, X0 - s - 1, Y + row - s // 2 + s - 1, frame, c, 1))
                out.append(CR._text(TEXT, s, X0 - 4 * s - (6 * len(text) - 1) * s, Y + row - 3 * s, text, 0, frame, c))
        text = "Y [m]" if k else "X [m]"
        out.append(CR._text(TEXT, s, s, Y + (PH - (6 * len(text) - 1) * s) // 2, text, 1, frame, k))
    t1 = hd[1]
    top = G["Y1"] + PH + s
    if t1 <= 1e9:
        u = 1
        while F(u) * F(128.0) < t1:
            u *= 10
        for k in range(140):
            sec = k * u
            if F(sec) > t1:
                break
            major = k % 5 == 0
            c = FR.col(F(sec), F(0.0), t1, PW)
            out.append(CR._box(LINE, X0 + c - s // 2, top, X0 + c - s // 2 + s - 1, top + (3 if major else 2) * s - 1, frame, sec, 0))
            if major:
                text = str(sec)
                out.append(CR._text(TEXT, s, X0 + c - ((6 * len(text) - 1) * s) // 2, top + 4 * s, text, 0, frame, sec))
    text = "Time [s]"
    out.append(CR._text(TEXT, s, X0 + (PW - (6 * len(text) - 1) * s) // 2, G["Y1"] + PH + 14 * s, text, 0, frame))
    names = ("Kinovea" if kind == "kinovea" else "Qualisys", "Velocity Tracker")
    BW, BH = 3 * s + 10 * s + (6 * len(names[0]) - 1) * s + 6 * s + 10 * s + (6 * len(names[1]) - 1) * s + 3 * s, 13 * s
    bx, by = X0 + PW + s - BW, 2 * s
    out.append(CR._box(LEGEND_BOX, bx, by, bx + BW - 1, by + BH - 1, frame, BW, BH))
    x = bx + 3 * s
    for k, name in enumerate(names):
        out.append(CR._box(SWATCH, x, by + 5 * s, x + 8 * s - 1, by + 8 * s - 1, frame, k, k))
        out.append(CR._text(LEGEND_TEXT, s, x + 10 * s, by + 3 * s, name, 0, frame, k))
        x += 10 * s + (6 * len(name) - 1) * s + 6 * s
    return np.array(out, np.int64).reshape(-1, 28)


def prepare(ref, rows, kind, plate=0.45, rate=30.0, **params):
    """dict(traj, grid, stats, head, counts int64 [4], pts int64 [sum, 3] (MERGED), recs int64 [n, 28], polys: the four UNMERGED tables)"""
    G = geom(**dict(DEFAULTS, **params))
    ref = np.asarray(ref, F).reshape(-1, 3)
    traj, grid, stats = numbers(ref, rows, kind, plate, rate)
    hd = head(kind, ref, traj)
    polys = [polyline(t, v, hd, panel, G) for t, v, panel in series(ref, traj)]
    merged = [CR.merge(p) for p in polys]
    return dict(traj=traj, grid=grid, stats=stats, head=hd, counts=np.array([len(m) for m in merged], np.int64), pts=np.concatenate(merged).reshape(-1, 3),
                recs=records(G, kind, hd), polys=polys)


def render_one(prep, merged=False, **params):
    """uint8 [H, W, 3] from prepare()'s dict: the records by rising priority, the curves (UNMERGED unless merged=True) in their place"""
    G = geom(**dict(DEFAULTS, **params))
    W, H, s = G["W"], G["H"], G["s"]
    b = (s + 1) // 2
    recs = prep["recs"]
    py, px = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    out = np.empty((H, W, 3), np.uint8)
    out[:] = CR.WHITE

    def box(r):
        return (px >= r[1]) & (px <= r[3]) & (py >= r[2]) & (py <= r[4])
    tables = prep["polys"]
    if merged:
        ends = np.cumsum(prep["counts"])
        tables = [prep["pts"][e - c:e] for c, e in zip(prep["counts"], ends)]
    for kind in (TEXT, LINE, CR.CURVES, LEGEND_BOX, SWATCH, LEGEND_TEXT):
        if kind == CR.CURVES:
            for k, table in enumerate(tables):                                     # the tracker's over the ground truth's
                Y = G["Y1"] if k >= 2 else G["Y0"]
                out[Y:Y + G["PH"], G["X0"]:G["X0"] + G["PW"]][CR.curve_mask(G, table)] = TRACKER if k & 1 else TRUTH
            continue
        for r in recs[recs[:, 0] == kind]:
            if kind in (TEXT, LEGEND_TEXT):
                out[CR.text_mask(px, py, r, s)] = CR.INK
            elif kind == LINE:
                out[box(r)] = CR.INK
            elif kind == LEGEND_BOX:
                rx, ry = px - r[5], py - r[6]
                edge = (rx < b) | (ry < b) | (rx >= r[7] - b) | (ry >= r[8] - b)
                out[box(r) & edge] = CR.BORDER
                out[box(r) & ~edge] = CR.WHITE
            elif kind == SWATCH:
                out[box(r)] = TRACKER if int(r[8]) else TRUTH
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
