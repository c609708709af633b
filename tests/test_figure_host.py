"""Rep figure without a GPU (include/vbt_hip.h, "Rep figure"): the entry points of the C ABI and their bindings, the refusals made
before the handle is looked at, the numpy statement (tests/figure_ref.py) against two cases worked out by hand, the shared core
(vbt_amd/csrc/figure_core.h) as a stand-alone host program under -fsanitize=address,undefined (tests/fuzz/figure_check.cc, run as a
program, never loaded into Python) against the numpy statement for the GPU test's cases, and the CLI's options."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from click.testing import CliRunner

import figure_cases as FC
import figure_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vbt_figure_default_params", "vbt_figure_create", "vbt_figure_destroy", "vbt_figure_set", "vbt_figure_render", "vbt_figure_table")
ARG, CAPACITY, STATE = -1, -4, -5


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib
    return _lib, _lib.lib()


def test_entry_points_are_exported_declared_and_bound():
    _lib_mod, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "vbt_hip.h")).read()
    assert "Rep figure" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in _lib_mod.declared_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert ctypes.sizeof(_lib_mod.FigureParams) == 32
    p = _lib_mod.FigureParams()
    L.vbt_figure_default_params(ctypes.byref(p))
    assert {k: getattr(p, k) for k in FR.DEFAULTS} == FR.DEFAULTS and p.reserved == 0
    assert re.search(r"#define\s+VBT_FIGURE_STAGE_POINTS\s+%d\b" % FR.STAGE_POINTS, code)
    assert re.search(r"#define\s+VBT_FIGURE_STAGE_RECORDS\s+%d\b" % FR.STAGE_RECORDS, code)
    from vbt_amd import figure
    assert figure.default_params() == FR.DEFAULTS and figure.RECORD == FR.RECORD
    for name in ("set", "render", "table", "frames"):
        assert callable(getattr(figure.Figure, name))
    assert callable(figure.plot) and callable(figure.plot_many)


def test_create_refuses_bad_sizes_before_any_device_call():
    _lib_mod, L = _lib()

    def create(**kw):
        p = _lib_mod.FigureParams()
        L.vbt_figure_default_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        h = ctypes.c_void_p()
        return L.vbt_figure_create(0, ctypes.byref(p), ctypes.byref(h)), L.vbt_last_error().decode(), h.value
    for kw, word in ((dict(width=0), "16384"), (dict(height=16385), "16384"), (dict(scale=0), "scale"), (dict(scale=65), "scale"),
                     (dict(thickness=0), "thickness"), (dict(max_figures=0), "max_figures"), (dict(max_figures=4097), "max_figures"),
                     (dict(max_rows=0), "max_rows"), (dict(max_phases=-1), "max_phases"), (dict(max_figures=4096, max_rows=1 << 20), "2^26"),
                     (dict(width=59, height=70, scale=1), "plot rectangle"), (dict(width=60, height=69, scale=1), "plot rectangle"),
                     (dict(width=160, height=100, scale=2), "plot rectangle")):
        rc, msg, h = create(**kw)
        assert rc == ARG and word in msg and "vbt_figure_create" in msg and not h, (kw, msg)
    assert L.vbt_figure_create(0, None, None) == ARG and "out" in L.vbt_last_error().decode()
    with pytest.raises(_lib_mod.VbtArgError):
        _lib_mod.check(create(width=0)[0])


def test_set_render_and_table_refuse_before_the_handle_is_looked_at():
    _lib_mod, L = _lib()
    rows = np.array([[0, .5, .5, 0, 0, .2, .2], [1, .5, .4, 0, -.1, .2, .2], [2, .5, .3, 0, -.1, .2, .2]], np.float64)
    ph = np.array([[0.0, 1.0, 0.5, 0.4, 0.3, 0.0], [1.0, 2.0, 0.4, 0.3, 0.3, 1.0]], np.float64)

    def fset(rows, ph, n=1, rc=None, pc=None):
        rows, ph = np.ascontiguousarray(rows, np.float64), np.ascontiguousarray(ph, np.float64)
        rc = np.array([len(rows)] if rc is None else rc, np.int32)
        pc = np.array([len(ph)] if pc is None else pc, np.int32)
        return L.vbt_figure_set(None, n, rows.ctypes.data, rc.ctypes.data, ph.ctypes.data, pc.ctypes.data, None), L.vbt_last_error().decode()
    assert fset(rows, ph) == (ARG, "vbt_figure_set: handle is NULL")             # good arguments get as far as the (missing) handle
    rc, msg = fset(rows, ph, n=-1)
    assert rc == ARG and "handle" not in msg
    rc, msg = fset(rows, ph, n=4097, rc=[0] * 4097, pc=[0] * 4097)
    assert rc == CAPACITY and "4097 figures" in msg
    rc, msg = fset(rows, ph, rc=[-1])
    assert rc == ARG and "negative" in msg
    rc, msg = fset(rows, ph, rc=[(1 << 20) + 1])
    assert rc == CAPACITY and "rows" in msg
    rc, msg = fset(rows, ph, pc=[65537])
    assert rc == CAPACITY and "phases" in msg
    for value in (np.nan, np.inf, -np.inf):
        bad = rows.copy()
        bad[1, 4] = value
        assert fset(bad, ph) == (ARG, "vbt_figure_set: figure 0, row 1 holds a non-finite value")
    bad = rows.copy()
    bad[2, 0] = 0.5
    assert fset(bad, ph) == (ARG, "vbt_figure_set: figure 0, row 2: time decreases")
    two = np.concatenate([rows, bad])                                              # the second figure's row is named as its own
    assert fset(two, np.concatenate([ph, ph]), n=2, rc=[3, 3], pc=[2, 2]) == (ARG, "vbt_figure_set: figure 1, row 2: time decreases")
    bad = ph.copy()
    bad[1, 5] = 3.0
    assert fset(rows, bad) == (ARG, "vbt_figure_set: figure 0, phase 1 has type 3, not 0, 1 or 2")
    bad = ph.copy()
    bad[1, 1] = 0.5
    assert fset(rows, bad) == (ARG, "vbt_figure_set: figure 0, phase 1 ends before it starts (time_end < time_start)")
    bad = ph.copy()
    bad[1, 0] = -1.0
    assert fset(rows, bad) == (ARG, "vbt_figure_set: figure 0: phases are not ordered in time at phase 1")
    bad = ph.copy()
    bad[0, 4] = np.nan
    assert fset(rows, bad) == (ARG, "vbt_figure_set: figure 0, phase 0 holds a non-finite value")
    assert L.vbt_figure_render(None, None, 0, 1, None) == ARG and "NULL" in L.vbt_last_error().decode()
    n = ctypes.c_int()
    assert L.vbt_figure_table(None, 0, None, None, 0, ctypes.byref(n), None, 0, ctypes.byref(n)) == ARG
    L.vbt_figure_destroy(None)


# ---- the numpy statement against two cases worked out by hand ----

SMALLEST = dict(width=60, height=70, scale=1, thickness=1)                         # the smallest legal figure at scale 1: 16 x 16 rectangles


def test_three_rows_on_the_smallest_figure_by_hand():
    """times 0, 1, 3; x = 0.6; y = 0.4, 0.48, 0.56, whose rolling means are 0.4, 0.44, 0.48; dy = -0.2.
    Position range [0.4 - 0.2, 0.6 + 0.2] = [0.2, 0.8]: row(v) = (0.8 - v) * 25, so x is row 5 and y rows 10, 9, 8.
    Velocity: m = -0.2, M = 0, pad = 0.01, range [-0.21, 0.01]: row(0) = rint(0.68) = 1, row(-0.2) = rint(14.3) = 14.
    Columns: t / 3 * 15 = 0, 5, 15."""
    rows = np.array([[0, .6, .4, 0, -.2, .2, .2], [1, .6, .48, 0, -.2, .2, .2], [3, .6, .56, 0, -.2, .2, .2]], np.float64)
    G = FR.geom(**SMALLEST)
    assert (G["X0"], G["Y0"], G["Y1"], G["PW"], G["PH"]) == (40, 11, 40, 16, 16)
    hd, pts, recs = FR.prepare(rows, np.zeros((0, 6)), **SMALLEST)
    assert hd[0] == 0 and hd[1] == 3 and abs(hd[2] - 0.2) < 1e-12 and abs(hd[3] - 0.8) < 1e-12 and abs(hd[4] + 0.21) < 1e-12 and abs(hd[5] - 0.01) < 1e-12
    assert pts.tolist() == [[0, 5, 10, 1, 14], [5, 5, 9, 1, 14], [15, 5, 8, 1, 14]]
    frame = FR.render_one(hd, pts, recs, **SMALLEST)
    # the y curve at thickness 1, rule 2 by hand.  Segment (0,10)-(5,9): L2 = 26, a pixel between the ends is covered when
    # 4 c^2 <= 26, c = -qx - 5 qy: row 10 columns 0..2, row 9 columns 3..5.  Segment (5,9)-(15,8): L2 = 101, 4 c^2 <= 101,
    # c = -qx - 10 qy from (5, 9): row 9 columns 5..10, row 8 columns 10..15.
    want = {(c, 10) for c in (0, 1, 2)} | {(c, 9) for c in range(3, 11)} | {(c, 8) for c in range(10, 16)}
    upper = frame[11:27, 40:56]
    got = {(int(c), int(r)) for r, c in zip(*np.nonzero((upper == FR.CURVE[5]).all(axis=2)))}
    assert got == want
    gotx = {(int(c), int(r)) for r, c in zip(*np.nonzero((upper == FR.CURVE[4]).all(axis=2)))}
    assert gotx == {(c, 5) for c in range(16)}                                     # x: a horizontal line
    lower = frame[40:56, 40:56]
    assert {(int(c), int(r)) for r, c in zip(*np.nonzero((lower == FR.CURVE[7]).all(axis=2)))} == {(c, 14) for c in range(16)}
    assert {(int(c), int(r)) for r, c in zip(*np.nonzero((lower == FR.CURVE[6]).all(axis=2)))} == {(c, 1) for c in range(16)}
    assert (frame[10, 39:57] == 0).all() and (frame[27, 39:57] == 0).all() and (frame[11:27, 39] == 0).all() and (frame[11:27, 56] == 0).all()   # frame lines


def test_the_empty_figure_by_hand():
    """T = 0: ranges [0, 1], time [0, 0].  Value step: 1000 / 200 = 5 <= 6, so ticks at 0, 0.2 .. 1.0 in rows (1 - v) * 15 = 15, 12, 9,
    6, 3, 0; one time tick, second 0, a major one with its label.  Per rectangle 4 lines, the title, 2 swatches, 2 key texts, 6 ticks
    and 6 labels: 21; and 2 for the time tick."""
    hd, pts, recs = FR.prepare(np.zeros((0, 7)), np.zeros((0, 6)), **SMALLEST)
    assert hd.tolist() == [0, 0, 0, 1, 0, 1] and pts.shape == (0, 5) and len(recs) == 44
    ticks = [r for r in recs[:21] if r[0] == FR.LINE and r[1] == 37]
    assert [(int(r[2]) - 11, int(r[10])) for r in ticks] == [(15, 0), (12, 20), (9, 40), (6, 60), (3, 80), (0, 100)]
    assert all((r[1], r[3], r[4] - r[2]) == (37, 38, 0) for r in ticks)             # [X0 - 3, X0 - 1) and one pixel high
    t = recs[-2:]
    assert t[0].tolist() == [FR.LINE, 40, 57, 40, 59, 40, 57, 0, 0, 0, 0, 1]        # under the lower rectangle: Y1 + PH + 1, three long
    assert t[1].tolist() == [FR.TEXT, 38, 61, 42, 67, 38, 61, 0, 0, 0, 0, 1]        # "0", centred on column 40
    frame = FR.render_one(hd, pts, recs, **SMALLEST)
    assert (frame[11:27, 40:56] == 255).all() and (frame[40:56, 40:56] == 255).all()
    zero = FR.glyph(0)
    assert np.array_equal((frame[61:68, 38:43] == 0).all(axis=2), zero)
    assert frame.shape == (70, 60, 3) and set(map(tuple, frame.reshape(-1, 3).tolist())) == {FR.WHITE, FR.INK}   # the swatches lie right of the frame


# ---- the shared core under sanitizers ----

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("figure") / "figure_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "fuzz", "figure_check.cc"), "-o", exe])
    return exe


def run(harness, tmp_path, rows, phases, width, height, scale, thickness):
    """the program's output parsed: (head, points, records, frame)"""
    rows, phases = np.ascontiguousarray(rows, np.float64).reshape(-1, 7), np.ascontiguousarray(phases, np.float64).reshape(-1, 6)
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        f.write(np.array([width, height, scale, thickness, len(rows), len(phases)], np.int32).tobytes() + rows.tobytes() + phases.tobytes())
    p = subprocess.run([harness, case, out], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, (p.stdout[-1000:], p.stderr[-3000:])
    b = open(out, "rb").read()
    hd = np.frombuffer(b, np.float64, 6)
    T = int(np.frombuffer(b, np.int32, 1, 48)[0])
    pts = np.frombuffer(b, np.int32, T * 5, 52).reshape(T, 5)
    o = 52 + T * 20
    n = int(np.frombuffer(b, np.int32, 1, o)[0])
    recs = np.frombuffer(b, np.int32, n * 12, o + 4).reshape(n, 12)
    frame = np.frombuffer(b, np.uint8, height * width * 3, o + 4 + n * 48).reshape(height, width, 3)
    assert len(b) == o + 4 + n * 48 + height * width * 3
    return hd, pts, recs, frame


@pytest.mark.parametrize("cfg", FC.CONFIGS, ids=lambda c: "%dx%d-s%d-t%d" % c)
def test_host_program_equals_the_numpy_statement(harness, tmp_path, cfg):
    for i, ((rows, phases), (hd, pts, recs, frame)) in enumerate(zip(FC.figures(), FC.reference(cfg))):
        ghd, gpts, grecs, gframe = run(harness, tmp_path, rows, phases, *cfg)
        assert np.array_equal(ghd, hd), (i, ghd, hd)                               # doubles with ==
        assert np.array_equal(gpts, pts), i
        assert grecs.shape == recs.shape and np.array_equal(grecs, recs), i
        assert np.array_equal(gframe, frame), (i, np.argwhere((gframe != frame).any(axis=2))[:10])


def test_the_cases_hold_what_they_are_meant_to():
    cfg = FC.CONFIGS[1]
    ref = FC.reference(cfg)
    G = FR.geom(**FC.params(cfg))
    (_, _, ra, fa), (_, pb, rb, _), (hc, pc, rc, _), (_, pd_, rd, _) = ref
    spans = ra[ra[:, 0] == FR.SPAN]
    assert len(spans) == 8 and spans[0, 5] < G["X0"] and spans[-1, 3] == G["X0"] + G["PW"] - 1        # one starts before t0, one is cut at t1
    assert spans[0, 3] == spans[2, 1] and spans[2, 3] == spans[4, 1]                # shared boundary columns
    labels = ra[(ra[:, 0] == FR.TEXT) & (ra[:, 11] >> 8 == 1)]
    assert len(labels) == 4 and labels[-1, 5] + 6 > labels[-1, 3] >= labels[-1, 1]  # the last label is cut by the right edge, not gone
    assert any(r[0] == FR.TEXT and r[10] < 0 for r in ra)                           # a minus glyph on the velocity axis
    lb = rb[(rb[:, 0] == FR.TEXT) & (rb[:, 11] >> 8 == 1)]
    assert len(pb) == 1 and lb[:, 10].tolist() == [30, 0] and (lb[:, 5] < G["X0"]).all()      # ACV 0.00, cut by the left edge
    assert len(pc) == 0 and hc.tolist() == [0, 0, 0, 1, 0, 1]
    ld = rd[(rd[:, 0] == FR.TEXT) & (rd[:, 11] >> 8 == 1)]
    assert ld[0, 10] == 9999 and len(pd_) == 700
    assert np.bincount(pd_[:, 0]).max() >= 6 and np.abs(np.diff(pd_[:, 4])).max() >= 10     # many points per column; a segment 10 rows high and at most a column wide
    assert FR.staged(pd_, rd, **FC.params(cfg))[0] is False and FR.staged(ref[0][1], ra, **FC.params(cfg)) == (True, True)


# ---- CLI ----

def test_plot_help_lists_the_options_and_fig_dir_is_required(tmp_path):
    from vbt_amd.cli import main
    res = CliRunner().invoke(main, ["plot", "--help"])
    assert res.exit_code == 0
    for opt in ("--fig_dir", "--plate_diameter", "--fig_size", "--fig_scale", "--fig_format", "--fig_quality"):
        assert opt in res.output, opt
    assert "--show_fig" not in res.output
    res = CliRunner().invoke(main, ["plot", str(tmp_path / "a_id1_m.pkl.gz")])
    assert res.exit_code == 2 and "--fig_dir" in res.output
    res = CliRunner().invoke(main, ["plot", str(tmp_path / "a_id1_m.pkl.gz"), "--fig_dir", str(tmp_path / "o"), "--fig_size", "wide"])
    assert res.exit_code == 2 and "--fig_size" in res.output
    res = CliRunner().invoke(main, ["plot", str(tmp_path / "missing_id1_m.pkl.gz"), "--fig_dir", str(tmp_path / "o")])
    assert isinstance(res.exception, FileNotFoundError)                             # reference plot.py:67-68
