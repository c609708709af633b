"""Curve figure without a GPU (include/vbt_hip.h, "Curve figure"): the entry points of the C ABI and their bindings, the refusals made
before the handle is looked at, the numpy statement (tests/curve_figure_ref.py) against two cases worked out by hand, the font, the
reversed series, the run merge against the unmerged polyline, the shared core (vbt_amd/csrc/curve_figure_core.h) as a stand-alone host
program under -fsanitize=address,undefined (tests/fuzz/curve_figure_check.cc, run as a program, never loaded into Python) against the
numpy statement for the GPU test's cases, and the CLI's options."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from click.testing import CliRunner

import curve_figure_cases as CC
import curve_figure_ref as CR
import figure_ref as FR
import overlay_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vbt_curve_figure_default_params", "vbt_curve_figure_create", "vbt_curve_figure_destroy", "vbt_curve_figure_set",
                "vbt_curve_figure_render", "vbt_curve_figure_table")
ARG, CAPACITY, STATE = -1, -4, -5


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib
    return _lib, _lib.lib()


def test_entry_points_are_exported_declared_and_bound():
    _lib_mod, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "vbt_hip.h")).read()
    assert "Curve figure" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in _lib_mod.declared_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert ctypes.sizeof(_lib_mod.CurveFigureParams) == 32 and ctypes.sizeof(_lib_mod.CurveFigureDesc) == 96
    assert ctypes.sizeof(_lib_mod.CurveSeries) == 72 and ctypes.sizeof(_lib_mod.CurveMark) == 24
    p = _lib_mod.CurveFigureParams()
    L.vbt_curve_figure_default_params(ctypes.byref(p))
    assert {k: getattr(p, k) for k in CR.DEFAULTS} == CR.DEFAULTS
    assert CR.DEFAULTS["max_series"] >= 8 and (CR.DEFAULTS["width"], CR.DEFAULTS["height"]) == (1120, 640)
    assert re.search(r"#define\s+VBT_CURVE_FIGURE_STAGE_POINTS\s+%d\b" % CR.STAGE_POINTS, code)
    assert re.search(r"#define\s+VBT_CURVE_FIGURE_STAGE_RECORDS\s+%d\b" % CR.STAGE_RECORDS, code)
    from vbt_amd import curve_figure, evaluate
    assert curve_figure.default_params() == CR.DEFAULTS and curve_figure.RECORD == CR.RECORD
    for name in ("set", "render", "table", "device_frames", "frames"):
        assert callable(getattr(curve_figure.CurveFigure, name))
    assert callable(evaluate.plot_precision_recall) and callable(evaluate.plot_roc)
    assert "without the figures" not in evaluate.__doc__


def test_create_refuses_bad_sizes_before_any_device_call():
    _lib_mod, L = _lib()

    def create(**kw):
        p = _lib_mod.CurveFigureParams()
        L.vbt_curve_figure_default_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        h = ctypes.c_void_p()
        return L.vbt_curve_figure_create(0, ctypes.byref(p), ctypes.byref(h)), L.vbt_last_error().decode(), h.value
    for kw, word in ((dict(width=0), "16384"), (dict(height=16385), "16384"), (dict(scale=0), "scale"), (dict(scale=65), "scale"),
                     (dict(thickness=0), "thickness"), (dict(max_figures=0), "max_figures"), (dict(max_figures=1025), "max_figures"),
                     (dict(max_series=0), "max_series"), (dict(max_series=17), "max_series"), (dict(max_points=0), "max_points"),
                     (dict(max_marks=-1), "max_marks"), (dict(max_marks=65), "max_marks"), (dict(max_figures=1024, max_points=1 << 17), "2^26"),
                     (dict(width=49, height=42, scale=1), "plot rectangle"), (dict(width=50, height=41, scale=1), "plot rectangle"),
                     (dict(width=160, height=60, scale=2), "plot rectangle")):
        rc, msg, h = create(**kw)
        assert rc == ARG and word in msg and "vbt_curve_figure_create" in msg and not h, (kw, msg)
    assert L.vbt_curve_figure_create(0, None, None) == ARG and "out" in L.vbt_last_error().decode()
    with pytest.raises(_lib_mod.VbtArgError):
        _lib_mod.check(create(width=0)[0])


def test_set_render_and_table_refuse_before_the_handle_is_looked_at():
    _lib_mod, L = _lib()
    from vbt_amd import curve_figure
    up = np.array([[0.0, 0.1], [0.5, 0.6], [1.0, 0.9]])
    good = CR.figure([(up, "a", 0), (up[::-1], "b", 1)], [(1, 2, "0.5000")], "x", "y", CR.LOWER_LEFT, 50, 100)

    def fset(figs, n=None, edit=None, null=()):
        descs, series, xy, marks = curve_figure.pack(figs)
        if edit:
            edit(descs, series, xy, marks)
        args = dict(descs=ctypes.addressof(descs), series=ctypes.addressof(series), xy=xy.ctypes.data, marks=ctypes.addressof(marks))
        args.update({k: None for k in null})
        rc = L.vbt_curve_figure_set(None, len(figs) if n is None else n, args["descs"], args["series"], args["xy"], args["marks"], None)
        return rc, L.vbt_last_error().decode()
    assert fset([good]) == (ARG, "vbt_curve_figure_set: handle is NULL")          # good arguments get as far as the (missing) handle
    assert fset([good, good]) == (ARG, "vbt_curve_figure_set: handle is NULL")
    for rc_msg, code, words in (
            (fset([good], n=-1), ARG, ("n -1",)),
            (fset([good], null=("descs",)), ARG, ("figs",)),
            (fset([good], n=1025), CAPACITY, ("1025 figures",)),
            (fset([good], edit=lambda d, s, x, m: setattr(d[0], "n_series", -1)), ARG, ("figure 0", "negative")),
            (fset([good], edit=lambda d, s, x, m: setattr(d[0], "n_marks", -2)), ARG, ("figure 0", "negative")),
            (fset([good], edit=lambda d, s, x, m: setattr(d[0], "legend_corner", 2)), ARG, ("figure 0", "legend_corner 2")),
            (fset([good], edit=lambda d, s, x, m: setattr(d[0], "minor_x", 19)), ARG, ("figure 0", "minor_x 19")),
            (fset([good], edit=lambda d, s, x, m: setattr(d[0], "minor_y", 1001)), ARG, ("figure 0", "minor_y 1001")),
            (fset([good], edit=lambda d, s, x, m: setattr(d[0], "n_series", 17)), CAPACITY, ("figure 0", "17 series")),
            (fset([good], edit=lambda d, s, x, m: setattr(d[0], "n_marks", 65)), CAPACITY, ("figure 0", "65 marks")),
            (fset([good], null=("series",)), ARG, ("NULL series",)),
            (fset([good], null=("marks",)), ARG, ("NULL series or marks",)),
            (fset([good], null=("xy",)), ARG, ("NULL xy",)),
            (fset([good, good], edit=lambda d, s, x, m: setattr(s[3], "n_points", -1)), ARG, ("figure 1, series 1", "negative")),
            (fset([good], edit=lambda d, s, x, m: setattr(s[1], "colour", 10)), ARG, ("figure 0, series 1", "colour 10")),
            (fset([good], edit=lambda d, s, x, m: setattr(s[0], "text", b"x" * 64)), ARG, ("figure 0, series 0", "NUL")),
            (fset([good], edit=lambda d, s, x, m: setattr(s[0], "text", b"ab\x7f")), ARG, ("figure 0, series 0", "0x7f at 2")),
            (fset([good], edit=lambda d, s, x, m: setattr(s[1], "text", b"\x1f")), ARG, ("figure 0, series 1", "0x1f at 0")),
            (fset([good], edit=lambda d, s, x, m: setattr(d[0], "y_title", b"a\tb")), ARG, ("figure 0", "y_title", "0x09 at 1")),
            (fset([good], edit=lambda d, s, x, m: setattr(d[0], "x_title", b"t" * 32)), ARG, ("figure 0", "x_title", "NUL")),
            (fset([good], edit=lambda d, s, x, m: setattr(m[0], "series", 2)), ARG, ("figure 0, mark 0", "series 2")),
            (fset([good], edit=lambda d, s, x, m: setattr(m[0], "point", 3)), ARG, ("figure 0, mark 0", "point 3")),
            (fset([good], edit=lambda d, s, x, m: setattr(m[0], "point", -1)), ARG, ("figure 0, mark 0", "point -1")),
            (fset([good], edit=lambda d, s, x, m: setattr(m[0], "text", b"\x80")), ARG, ("figure 0, mark 0", "0x80")),
            (fset([good], edit=lambda d, s, x, m: setattr(m[0], "text", b"m" * 16)), ARG, ("figure 0, mark 0", "NUL"))):
        assert rc_msg[0] == code and all(w in rc_msg[1] for w in words) and "handle" not in rc_msg[1], (rc_msg, words)
    # x that turns back: the figure, the series and the index of the first point that does are named; non-finite points are passed over
    zig = np.array([[0.0, 0.1], [0.5, 0.6], [np.nan, 0.2], [0.4, 0.9], [0.6, 0.9]])
    bad = CR.figure([(up, "a", 0), (zig, "b", 1)])
    rc, msg = fset([good, bad])
    assert rc == ARG and "figure 1, series 1, point 3" in msg and "monotone" in msg
    with pytest.raises(ValueError, match="point 3"):
        CR.ordered(zig)
    flat = np.array([[0.5, 0.1], [0.5, 0.6], [np.nan, np.nan], [0.5, 0.2]])           # never moves: both directions hold
    assert fset([CR.figure([(flat, "flat", 0)])])[1] == "vbt_curve_figure_set: handle is NULL"
    with pytest.raises(ValueError, match="at most 63"):
        curve_figure.pack([CR.figure([(up, "x" * 64, 0)])])
    with pytest.raises(ValueError, match="at most 15"):
        curve_figure.pack([CR.figure([(up, "x", 0)], [(0, 0, "y" * 16)])])
    with pytest.raises(ValueError, match="ASCII"):
        curve_figure.pack([CR.figure([(up, "café", 0)])])
    assert L.vbt_curve_figure_render(None, None, 0, 1, None) == ARG and "NULL" in L.vbt_last_error().decode()
    n = ctypes.c_int()
    assert L.vbt_curve_figure_table(None, 0, None, 0, ctypes.byref(n), None, 0, ctypes.byref(n), None, 0, ctypes.byref(n)) == ARG
    L.vbt_curve_figure_destroy(None)


# ---- the numpy statement against two cases worked out by hand ----

SMALLEST = dict(width=50, height=42, scale=1, thickness=1)                         # the smallest legal figure at scale 1: a 16 x 16 rectangle


def _pixels(frame, colour, x0, y0, w, h):
    return {(int(c), int(r)) for r, c in zip(*np.nonzero((frame[y0:y0 + h, x0:x0 + w] == colour).all(axis=2)))}


def test_a_two_point_curve_on_the_smallest_figure_by_hand():
    """col(x) = x / 1.01 * 15, row(y) = (1.01 - y) / 1.01 * 15.  The points (0, 1.01 / 3) and (1.01 / 3, 0.404) are (0, 10) and (5, 9).
    Rule 2 at thickness 1 on (0, 10) - (5, 9): L2 = 26, a pixel between the ends is covered when 4 c^2 <= 26, c = -qx - 5 qy:
    row 10 columns 0..2, row 9 columns 3..5.  No legend text: the box is 16 wide and 13 high at (33, 4) and hides the curve's
    columns 3..5 of row 9 (frame (33..35, 13)), which is what priority 2 over 6 says."""
    G = CR.geom(**SMALLEST)
    assert (G["X0"], G["Y0"], G["PW"], G["PH"]) == (30, 4, 16, 16)
    xy = np.array([[0.0, 1.01 / 3], [1.01 / 3, 0.404]])
    assert CR.polyline(xy, G).tolist() == [[0, 10, 0], [5, 9, 1]]
    mask = CR.curve_mask(G, CR.polyline(xy, G))
    assert {(int(c), int(r)) for r, c in zip(*np.nonzero(mask))} == {(0, 10), (1, 10), (2, 10), (3, 9), (4, 9), (5, 9)}
    fig = CR.figure([(xy, "", 3)])
    counts, pts, recs = CR.prepare(fig, **SMALLEST)
    assert counts.tolist() == [2] and pts.tolist() == [[0, 10, 0], [5, 9, 1]]
    box = recs[recs[:, 0] == CR.LEGEND_BOX]
    assert box[:, 1:9].tolist() == [[33, 4, 48, 16, 33, 4, 16, 13]]                 # bx = 30 + 3, by = 4 + 16 - 3 - 13, BW = 16, BH = 9 + 4
    frame = CR.render_one(fig, **SMALLEST)
    assert _pixels(frame, CR.PALETTE[3], 30, 4, 16, 16) == {(0, 10), (1, 10), (2, 10)} | {(c, r) for c in range(6, 14) for r in (5, 6, 7)}   # and the swatch: frame [36, 44) x [9, 12)
    assert (frame[4:17, 33] == CR.BORDER).all() and (frame[4, 33:49] == CR.BORDER).all() and (frame[16, 33:49] == CR.BORDER).all()
    assert (frame[13, 34:36] == CR.WHITE).all()                                     # the box is opaque: no curve inside it
    assert (frame[4:21, 29] == CR.INK).all() and (frame[20, 30:46] == CR.INK).all()  # the two spines
    assert (frame[3, 29:] == CR.WHITE).all() and (frame[4:20, 46] != CR.INK).any()   # no top spine, no right spine


def test_one_text_record_by_hand():
    """The x title "Hi" on the smallest figure: 2 bytes, 11 pixels wide, centred under the rectangle at ox = 30 + (16 - 11) / 2 = 32,
    oy = 4 + 16 + 14 = 34; 'H' covers columns 32..36, column 37 is the gap, 'i' covers 38..42."""
    fig = CR.figure(x_title="Hi")
    _, pts, recs = CR.prepare(fig, **SMALLEST)
    assert len(pts) == 0
    want = [CR.TEXT, 32, 34, 42, 40, 32, 34, 0, 0, 2, 0, 0, ord("H") | ord("i") << 8] + [0] * 15
    assert recs[-1].tolist() == want and len(recs) == 2 + 12 * 3 + 1                 # spines, 12 ticks with label and grid line, the title
    frame = CR.render_one(fig, **SMALLEST)
    ink = (frame == 0).all(axis=2)
    assert np.array_equal(ink[34:41, 32:37], CR.glyph("H")) and np.array_equal(ink[34:41, 38:43], CR.glyph("i")) and not ink[34:41, 37].any()
    assert not ink[41].any() and not ink[34:41, 43:].any()
    # the y axis label "1.0": v = 1 is row rint(0.01 / 1.01 * 15) = 0; the label's box starts at (30 - 22, 4 - 3)
    label = [r for r in recs if r[0] == CR.TEXT and r[7] == 1000 and r[5] == 8]
    assert len(label) == 1 and label[0][1:7].tolist() == [8, 1, 24, 7, 8, 1]
    assert label[0][9] == 3 and label[0][12] == ord("1") | ord(".") << 8 | ord("0") << 16 and not label[0][13:].any()
    assert np.array_equal(ink[1:4, 8:13], CR.glyph("1")[:3])                        # (the label of 0.8 begins three rows lower on a rectangle this small)


# ---- the font ----

def _header_font():
    hdr = open(os.path.join(ROOT, "include", "vbt_hip.h")).read()
    sect = hdr[hdr.index("Curve figure ----"):hdr.index("MJPEG export ----")]
    return dict(re.findall(r"'(.)' ((?:[01]{5} ){6}[01]{5})", sect))


def _core_font():
    src = open(os.path.join(ROOT, "vbt_amd", "csrc", "curve_font.h")).read()
    lits = re.findall(r"0b([01']{41})ull", src)
    return {chr(0x20 + i): lit.replace("'", " ") for i, lit in enumerate(lits)}


def test_the_font_covers_printable_ascii_and_reuses_the_existing_glyphs():
    chars = [chr(c) for c in range(0x20, 0x7F)]
    assert sorted(CR.FONT) == chars
    assert all(re.fullmatch(r"(?:[01]{5} ){6}[01]{5}", CR.FONT[c]) for c in chars)
    assert len(set(CR.FONT.values())) == 95                                         # no two glyphs are equal
    assert _core_font() == CR.FONT and _header_font() == CR.FONT                    # the header writes the table out; the core holds it
    # the characters the rep panel and the rep figure already draw keep their bits
    old = {ch: FR.GLYPHS[code] for ch, code in FR.CODES.items()}
    assert sorted(old) == sorted("0123456789REPOMACV. -/SXYD")
    for ch, bits in old.items():
        assert CR.FONT[ch] == bits, ch
    for ch in "id":                                                                 # the tracking overlay's label
        assert CR.FONT[ch] == R.GLYPHS[ch], ch
    assert FR.CODES["D"] == 27 and max(FR.CODES.values()) == 27                     # the old codes are what they were


# ---- reversed series, and the run merge ----

def test_a_decreasing_series_equals_the_same_points_reversed():
    p = CC.params(CC.CONFIGS[1])
    a = CC.figure_a()
    flipped = dict(a, series=[(xy[::-1].copy(), t, c) for xy, t, c in a["series"]])
    for got, want in zip(CR.prepare(flipped, **p), CR.prepare(a, **p)):
        assert np.array_equal(got, want)
    assert np.array_equal(CR.render_one(flipped, **p), CR.render_one(a, **p))
    with_marks = CC.figure_e()
    xy, t, c = with_marks["series"][0]
    n = len(xy)
    back = dict(with_marks, series=[(xy[::-1].copy(), t, c)], marks=[(s, n - 1 - i, txt) for s, i, txt in with_marks["marks"]])
    assert np.array_equal(CR.render_one(back, **p), CR.render_one(with_marks, **p))


def test_merged_and_unmerged_polylines_cover_the_same_pixels():
    """the CPU side of the capsule-union argument: figures (a) and (d) at every configuration and 200 seeded random tables"""
    for cfg in CC.CONFIGS:
        G = CR.geom(**CC.params(cfg))
        for fig in (CC.figure_a(), CC.figure_d()):
            for xy, _, _ in fig["series"]:
                table = CR.polyline(xy, G)
                merged = CR.merge(table)
                assert len(merged) <= len(table) and np.array_equal(CR.curve_mask(G, merged), CR.curve_mask(G, table))
        d = CR.polyline(CC.figure_d()["series"][0][0], G)
        assert len(d) == 3000 and len(CR.merge(d)) <= 400
    rng = np.random.default_rng(20251019)
    shrunk = 0
    for k in range(200):
        G = dict(PW=int(rng.integers(16, 48)), PH=int(rng.integers(16, 48)), t=int(rng.integers(1, 5)))
        n = int(rng.integers(1, 60))
        cols = np.sort(rng.integers(-3, G["PW"] + 3, n) // int(rng.integers(1, 6)) * int(rng.integers(1, 3)))
        rows = rng.integers(-3, G["PH"] + 3, n)
        if k % 3 == 0:
            rows = np.round(rows / 4).astype(np.int64) * 4                           # equal rows in a run: the FIRST lowest / highest is kept
        join = (rng.random(n) < 0.9).astype(np.int64)
        join[0] = 0
        table = np.stack([cols, rows, join], axis=1).astype(np.int64)
        merged = CR.merge(table)
        shrunk += len(merged) < len(table)
        assert np.array_equal(CR.curve_mask(G, merged), CR.curve_mask(G, table)), (k, table.tolist())
    assert shrunk > 100                                                             # the merge did something in most of them


# ---- the shared core under sanitizers ----

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("curve_figure") / "curve_figure_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "fuzz", "curve_figure_check.cc"), "-o", exe])
    return exe


def case_bytes(fig, cfg):
    b = np.array(list(cfg) + [fig["corner"], fig["minor_x"], fig["minor_y"], len(fig["series"]), len(fig["marks"])], np.int32).tobytes()
    b += fig["x_title"].encode().ljust(32, b"\0") + fig["y_title"].encode().ljust(32, b"\0")
    for xy, text, colour in fig["series"]:
        b += np.array([len(xy), colour], np.int32).tobytes() + text.encode().ljust(64, b"\0")
    for s, p, text in fig["marks"]:
        b += np.array([s, p], np.int32).tobytes() + text.encode().ljust(16, b"\0")
    return b + b"".join(np.ascontiguousarray(xy, np.float64).tobytes() for xy, _, _ in fig["series"])


def run(harness, tmp_path, fig, cfg, expect=0):
    """the program's output parsed: (counts, points, records, frame)"""
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        f.write(case_bytes(fig, cfg))
    p = subprocess.run([harness, case, out], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert p.returncode == expect and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, (p.stdout[-1000:], p.stderr[-3000:])
    if expect:
        return p.stdout
    b = open(out, "rb").read()
    K = int(np.frombuffer(b, np.int32, 1)[0])
    counts = np.frombuffer(b, np.int32, K, 4)
    o = 4 + 4 * K
    T = int(np.frombuffer(b, np.int32, 1, o)[0])
    pts = np.frombuffer(b, np.int32, T * 3, o + 4).reshape(T, 3)
    o += 4 + T * 12
    n = int(np.frombuffer(b, np.int32, 1, o)[0])
    recs = np.frombuffer(b, np.int32, n * 28, o + 4).reshape(n, 28)
    o += 4 + n * 112
    frame = np.frombuffer(b, np.uint8, cfg[0] * cfg[1] * 3, o).reshape(cfg[1], cfg[0], 3)
    assert len(b) == o + cfg[0] * cfg[1] * 3
    return counts, pts, recs, frame


@pytest.mark.parametrize("cfg", CC.CONFIGS, ids=lambda c: "%dx%d-s%d-t%d" % c)
def test_host_program_equals_the_numpy_statement(harness, tmp_path, cfg):
    """the program renders the MERGED tables, numpy the unmerged polyline"""
    for name, fig, (counts, pts, recs, frame) in zip(CC.NAMES, CC.figures(), CC.reference(cfg)):
        gcounts, gpts, grecs, gframe = run(harness, tmp_path, fig, cfg)
        assert np.array_equal(gcounts, counts), (name, gcounts, counts)
        assert np.array_equal(gpts, pts), (name, np.argwhere(gpts != pts)[:5])
        assert grecs.shape == recs.shape and np.array_equal(grecs, recs), name
        assert np.array_equal(gframe, frame), (name, np.argwhere((gframe != frame).any(axis=2))[:10])


def test_host_program_refuses_a_series_that_turns_back(harness, tmp_path):
    fig = CR.figure([(np.array([[0.0, 0.0], [0.5, 0.5], [0.4, 0.6]]), "zig", 0)])
    assert "series 0, point 2" in run(harness, tmp_path, fig, CC.CONFIGS[1], expect=3)


def test_the_cases_hold_what_they_are_meant_to():
    for cfg in CC.CONFIGS:
        p, G = CC.params(cfg), CR.geom(**CC.params(cfg))
        ref = dict(zip(CC.NAMES, CC.reference(cfg)))
        st = {k: CR.staged(v[0], v[1], v[2], **p) for k, v in ref.items()}
        # which path: (d) reads global memory where its 100 stretches have a column each (the module's docstring); the six real curves of
        # (g) hold 400 merged points, which one tile of the narrow figures sees all of
        wide = cfg[0] == 320
        assert st["d"] == (not wide, True) and st["g"] == (wide, True), (cfg, st)
        assert all(v == (True, True) for k, v in st.items() if k not in "dg"), (cfg, st)
        assert ref["d"][0].tolist() == ([400] if wide else [len(ref["d"][1])]) and len(ref["d"][1]) <= 400
        assert ref["b"][0].tolist() == [1, 0] and ref["c"][0].tolist() == [3, 0, 5, 3]
        assert ref["c"][1][3:8, 2].tolist() == [0, 1, 0, 0, 1]                       # the hole breaks the polyline; an isolated point behind it
        box = ref["f"][2][ref["f"][2][:, 0] == CR.LEGEND_BOX][0]
        assert box[7] == (6 * 63 - 1 + 16) * cfg[2] and (box[5] < 0) == (cfg[0] < 320 * cfg[2]) and box[1] == max(box[5], 0)   # wider than the narrow figures: clipped
        texts = ref["e"][2][ref["e"][2][:, 0] == CR.MARK_TEXT]
        assert len(texts) == 5 and texts[4][5] < 0 and texts[4][1] == 0 and (texts[2][5:7] != texts[3][5:7]).any()
    xy = CC.figure_a()["series"]
    assert (np.diff(xy[1][0][:, 0]) <= 0).all() and (np.diff(xy[0][0][:, 0]) >= 0).all() and (xy[0][0][11] == xy[0][0][10]).all()


# ---- CLI ----

def test_eval_help_lists_the_figure_options_and_a_bad_size_is_refused(tmp_path):
    from vbt_amd.cli import main
    res = CliRunner().invoke(main, ["eval", "--help"])
    assert res.exit_code == 0
    for opt in ("--fig_dir", "--fig_size", "--fig_scale", "--fig_format", "--fig_quality", "--curve_dir", "--score_thresholds"):
        assert opt in res.output, opt
    res = CliRunner().invoke(main, ["eval", "--detections_df", str(tmp_path / "none.pkl.gz"), "--fig_dir", str(tmp_path / "o"), "--fig_size", "wide"])
    assert res.exit_code == 2 and "--fig_size" in res.output and not (tmp_path / "o").exists()
    res = CliRunner().invoke(main, ["eval", "--fig_format", "png"])
    assert res.exit_code == 2 and "--fig_format" in res.output
    from vbt_amd import cli
    assert "--fig_dir DIR" in cli.__doc__ and "without the figures: VOC" not in cli.__doc__
