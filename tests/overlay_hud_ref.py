"""TEST INFRASTRUCTURE ONLY (numpy): the rep panel of the tracking overlay, written from the text of include/vbt_hip.h ("Rep panel"),
not from the kernel.  A gather over the panel rectangle: every pixel is tested against the text, the bars and the timeline and gets
one of the two colours.  The rows-only picture (tests/overlay_ref.py) is painted first, then the panel.  Slow and small on purpose."""
import numpy as np

import overlay_ref as R

HUD_DEFAULTS = dict(x=16, y=16, scale=3, full_scale_cm=200, bg=(0, 0, 0))
TABLE = ("fs", "fe", "rom_cm", "acv_cm", "type", "count")
CONCENTRIC, ECCENTRIC, HOLD = 0, 1, 2

GLYPHS = dict(R.GLYPHS, **{
    "R": "11110 10001 10001 11110 10100 10010 10001", "A": "01110 10001 10001 11111 10001 10001 10001",
    "E": "11111 10000 10000 11110 10000 10000 11111", "C": "01110 10001 10000 10000 10000 10001 01110",
    "P": "11110 10001 10001 11110 10000 10000 10000", "V": "10001 10001 10001 10001 10001 01010 00100",
    "O": "01110 10001 10001 10001 10001 10001 01110", ".": "00000 00000 00000 00000 00000 01100 01100",
    "M": "10001 11011 10101 10101 10001 10001 10001", " ": "00000 00000 00000 00000 00000 00000 00000",
})


def glyph(ch):
    """bool [7, 5]: rows top to bottom, columns left to right"""
    return np.array([[b == "1" for b in row] for row in GLYPHS[ch].split()], bool)


def phases6(phases):
    """[P,6] array or list of objects with time_start, time_end, y_start, y_end, rom, type -> float64 [P,6]"""
    if len(phases) and hasattr(phases[0], "time_start"):
        phases = [(p.time_start, p.time_end, p.y_start, p.y_end, p.rom, p.type) for p in phases]
    return np.asarray(phases, np.float64).reshape(-1, 6)


def frame_number(t, fps):
    return int(np.rint(np.clip(np.float64(t) * np.float64(fps), -2.0 ** 30, 2.0 ** 30)))          # llrint: ties to even


def centi(v):
    v = np.float64(v)
    if np.isnan(v) or v <= 0:
        return 0
    return int(np.rint(min(v * np.float64(100.0), np.float64(9999.0))))


def table(phases, fps):
    """int64 [P, 6] = fs, fe, rom_cm, acv_cm, type, concentric phases among phases 0..i"""
    ph = phases6(phases)
    t = np.zeros((len(ph), 6), np.int64)
    count = 0
    for i, (ts, te, _, _, rom, typ) in enumerate(ph):
        dur = te - ts
        count += int(typ) == CONCENTRIC
        with np.errstate(over="ignore"):
            t[i] = (frame_number(ts, fps), frame_number(te, fps), centi(rom), centi(rom / dur) if dur > 0 else 0, int(typ), count)
    return t


def completed(tab, f):
    """table indices of the completed reps of frame f, in table order"""
    return [i for i in range(len(tab)) if tab[i, 4] == CONCENTRIC and tab[i, 1] <= f]


def field(n, v):
    return "     " if n == 0 else f"{v // 100}.{v % 100:02d}".rjust(5)


def text_lines(tab, f):
    done = completed(tab, f)
    n = len(done)
    rom, acv = (int(tab[done[-1], 2]), int(tab[done[-1], 3])) if n else (0, 0)
    return ["REP" + str(min(n, 99999)).rjust(5), "ROM" + field(n, rom), "ACV" + field(n, acv)]


def bar_heights(tab, f, s, full_scale_cm):
    """hb of the eight slots; 0 = empty"""
    done = completed(tab, f)
    n = len(done)
    out = []
    for j in range(8):
        m = max(n - 8, 0) + j
        out.append(min(max(int(tab[done[m], 3]) * 12 * s // full_scale_cm, 1), 12 * s) if m < n else 0)
    return out


def timeline_phase(tab, fc):
    """index of the first phase with fs < fc <= fe, or None"""
    for i in range(len(tab)):
        if tab[i, 0] < fc <= tab[i, 1]:
            return i
    return None


def panel_mask(tab, f, frame_step, s, full_scale_cm):
    """bool [50 s, 52 s]: the covered pixels of the panel of frame number f, counted from the panel's origin"""
    py, px = np.meshgrid(np.arange(50 * s, dtype=np.int64), np.arange(52 * s, dtype=np.int64), indexing="ij")
    m = np.zeros(px.shape, bool)
    for l, line in enumerate(text_lines(tab, f)):
        assert len(line) == 8, line
        for k, ch in enumerate(line):
            bits = glyph(ch)
            for r in range(7):
                for c in range(5):
                    if bits[r, c]:
                        left, top = 2 * s + 6 * s * k + s * c, 2 * s + 9 * s * l + s * r
                        m |= (px >= left) & (px < left + s) & (py >= top) & (py < top + s)
    for j, hb in enumerate(bar_heights(tab, f, s, full_scale_cm)):
        if hb:
            left = 2 * s + 6 * s * j
            m |= (px >= left) & (px < left + 5 * s) & (py >= 41 * s - hb) & (py < 41 * s)
    for c in range(47 * s):
        fc = int(f) - (47 * s - 1 - c) * int(frame_step)
        i = timeline_phase(tab, fc) if fc >= 1 else None
        if i is None or tab[i, 4] == HOLD:
            continue
        top = 43 * s if tab[i, 4] == CONCENTRIC else 45 * s
        m |= (px == 2 * s + c) & (py >= top) & (py < 47 * s)
    return m


def paint_panel(frame, mask, x, y, pix_fmt, fg, bg):
    """one frame with every pixel of the panel rectangle at (x, y) written: fg where mask, bg elsewhere; as a copy"""
    out = np.array(frame, np.uint8, copy=True)
    ph, pw = mask.shape
    if pix_fmt == "rgb24":
        out[y:y + ph, x:x + pw] = np.where(mask[:, :, None], np.asarray(fg, np.uint8), np.asarray(bg, np.uint8))
        return out
    assert x % 2 == 0 and y % 2 == 0, (x, y)
    H, W = out.shape[0] * 2 // 3, out.shape[1]
    (Yf, Uf, Vf), (Yb, Ub, Vb) = R.yuv_colour(fg), R.yuv_colour(bg)
    flat = out.reshape(-1)
    flat[:H * W].reshape(H, W)[y:y + ph, x:x + pw] = np.where(mask, Yf, Yb)
    cm = mask.reshape(ph // 2, 2, pw // 2, 2).any(axis=(1, 3))         # chroma sample (py >> 1, px >> 1): any of its four pixels
    U, V = np.where(cm, Uf, Ub), np.where(cm, Vf, Vb)
    cy, cx = y // 2, x // 2
    chroma = flat[H * W:]
    if pix_fmt == "nv12":
        uv = chroma.reshape(H // 2, W // 2, 2)
        uv[cy:cy + ph // 2, cx:cx + pw // 2, 0], uv[cy:cy + ph // 2, cx:cx + pw // 2, 1] = U, V
    else:
        assert pix_fmt == "i420", pix_fmt
        q = (H // 2) * (W // 2)
        chroma[:q].reshape(H // 2, W // 2)[cy:cy + ph // 2, cx:cx + pw // 2] = U
        chroma[q:].reshape(H // 2, W // 2)[cy:cy + ph // 2, cx:cx + pw // 2] = V
    return out


NO_ROWS = {k: [] for k in R.COLUMNS}


def draw(frames, data, fps, phases, frame0=1, frame_step=1, pix_fmt="rgb24", hud_params=None, **params):
    """frames[i] = frame number frame0 + i * frame_step: the rows-only overlay of `data` (None: no rows), then the panel of `phases`"""
    hp = dict(HUD_DEFAULTS, **(hud_params or {}))
    fg = dict(R.DEFAULTS, **params)["rgb"]
    out = R.draw(frames, NO_ROWS if data is None else data, fps, frame0=frame0, frame_step=frame_step, pix_fmt=pix_fmt, **params)
    tab = table(phases, fps)
    H, W = R.frame_hw(frames, pix_fmt)
    assert hp["x"] >= 0 and hp["y"] >= 0 and hp["x"] + 52 * hp["scale"] <= W and hp["y"] + 50 * hp["scale"] <= H
    for i in range(len(out)):
        mask = panel_mask(tab, frame0 + i * frame_step, frame_step, hp["scale"], hp["full_scale_cm"])
        out[i] = paint_panel(out[i], mask, hp["x"], hp["y"], pix_fmt, fg, hp["bg"])
    return out


def render(frames, data, fps, phases, frame_stride=1, pix_fmt="rgb24", hud_params=None, **params):
    """the kept frames of a clip (1-based number a multiple of frame_stride), drawn with the panel"""
    kept = np.asarray(frames)[frame_stride - 1::frame_stride]
    return draw(kept, data, fps, phases, frame0=frame_stride, frame_step=frame_stride, pix_fmt=pix_fmt, hud_params=hud_params, **params)
