"""Rep panel of the tracking overlay without a GPU: the new entry points of the C ABI, the refusals vbt_overlay_set_hud makes before it
looks at the handle, the numpy statement of the panel's contract (tests/overlay_hud_ref.py) against cases worked out by hand, and
the CLI flag."""
import ctypes

import numpy as np
from click.testing import CliRunner

import overlay_hud_ref as HR
import overlay_ref as R

ENTRY_POINTS = ("vbt_overlay_hud_default_params", "vbt_overlay_set_hud", "vbt_overlay_hud_table")
FPS = 30.0


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib
    return _lib, _lib.lib()


def test_entry_points_are_exported_declared_and_bound():
    import os
    import re
    from conftest import ROOT
    _lib_mod, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "vbt_hip.h")).read() + open(os.path.join(ROOT, "include", "vbt_hip_diag.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in _lib_mod.declared_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert "vbt_overlay_hud_params" in hdr
    assert ctypes.sizeof(_lib_mod.OverlayHudParams) == 24
    assert ctypes.sizeof(_lib_mod.OverlayParams) == 24                       # the existing structure keeps its layout
    p = _lib_mod.OverlayHudParams()
    L.vbt_overlay_hud_default_params(ctypes.byref(p))
    assert (p.x, p.y, p.scale, p.full_scale_cm, list(p.bg), list(p.reserved)) == (16, 16, 3, 200, [0, 0, 0], [0] * 5)
    assert HR.HUD_DEFAULTS == dict(x=16, y=16, scale=3, full_scale_cm=200, bg=(0, 0, 0))


def _phases(n=4):
    """n phases of 10 frames each, eccentric and concentric in turn"""
    ph = np.zeros((n, 6), np.float64)
    for i in range(n):
        ph[i] = ((1 + 10 * i) / FPS, (11 + 10 * i) / FPS, 0.4, 0.6, 0.5, 1 - i % 2)
    return ph


def test_set_hud_refuses_bad_arguments_before_it_looks_at_the_handle():
    _lib_mod, L = _lib()

    def set_hud(ph, fps=FPS, P=None, **kw):
        p = _lib_mod.OverlayHudParams()
        L.vbt_overlay_hud_default_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        ph = None if ph is None else np.ascontiguousarray(ph, np.float64)
        rc = L.vbt_overlay_set_hud(None, ctypes.byref(p), None if ph is None else ph.ctypes.data, len(ph) if P is None else P, fps, None)
        return rc, L.vbt_last_error().decode()
    rc, msg = set_hud(_phases())
    assert rc == -1 and "handle" in msg                                      # good phases get as far as the (missing) handle
    rc, msg = set_hud(np.zeros((0, 6)))
    assert rc == -1 and "handle" in msg                                      # so does P = 0 with params
    assert L.vbt_overlay_set_hud(None, None, None, 0, FPS, None) == -1 and "handle" in L.vbt_last_error().decode()   # and the switch-off
    for fps in (0.0, -30.0, float("nan"), float("inf")):
        rc, msg = set_hud(_phases(), fps)
        assert rc == -1 and "fps" in msg and "handle" not in msg, (fps, msg)
    for (i, k), value, word in (((1, 4), np.nan, "non-finite"), ((2, 0), np.inf, "non-finite"), ((0, 3), -np.inf, "non-finite"),
                                ((1, 5), 3.0, "type"), ((1, 5), -1.0, "type"), ((1, 5), 0.5, "type"),
                                ((2, 1), 20.5 / FPS, "ends before"),          # time_end < time_start
                                ((2, 0), 10.5 / FPS, "not ordered"),          # time_start decreasing
                                ((1, 1), 31.5 / FPS, "not ordered")):         # time_end decreasing (phase 2 ends at 31 / fps)
        ph = _phases()
        ph[i, k] = value
        rc, msg = set_hud(ph)
        assert rc == -1 and word in msg and "handle" not in msg, ((i, k), value, msg)
    rc, msg = set_hud(_phases(), P=-1)
    assert rc == -1 and "bad argument" in msg
    rc, msg = set_hud(None, P=3)
    assert rc == -1 and "bad argument" in msg
    ph = _phases()
    assert L.vbt_overlay_set_hud(None, None, ph.ctypes.data, len(ph), FPS, None) == -1 and "bad argument" in L.vbt_last_error().decode()
    for kw, word in ((dict(scale=0), "scale"), (dict(scale=65), "scale"), (dict(full_scale_cm=0), "full_scale_cm"),
                     (dict(full_scale_cm=100001), "full_scale_cm"), (dict(x=-1), "negative"), (dict(y=-2), "negative")):
        rc, msg = set_hud(_phases(), **kw)
        assert rc == -1 and word in msg and "handle" not in msg, (kw, msg)
    many = np.zeros((65537, 6), np.float64)
    many[:, 0], many[:, 1], many[:, 5] = 1 / FPS, 2 / FPS, 2
    rc, msg = set_hud(many)
    assert rc == -4 and "65536" in msg, msg
    rc, msg = set_hud(many[:65536])
    assert rc == -1 and "handle" in msg                                      # 65536 phases are allowed
    ph = _phases()
    ph[3, 1] = ((1 << 24) + 1) / FPS
    rc, msg = set_hud(ph)
    assert rc == -4 and "frame" in msg, msg
    ph[3, 1] = (1 << 24) / FPS
    rc, msg = set_hud(ph)
    assert rc == -1 and "handle" in msg                                      # frame 2^24 itself is allowed
    assert L.vbt_overlay_hud_table(None, None, 0, None) == -1


def test_reference_glyph_cell_and_dot():
    s = 2
    m = HR.panel_mask(HR.table(np.zeros((0, 6)), FPS), 1, 1, s, 200)          # "REP    0" and blank fields
    assert m.shape == (50 * s, 52 * s)
    assert HR.text_lines(HR.table(np.zeros((0, 6)), FPS), 1) == ["REP    0", "ROM     ", "ACV     "]
    assert m[2 * s:3 * s, 2 * s:3 * s].all()                                  # R, row 0, column 0: the s x s block at (2 s, 2 s)
    assert m[2 * s:3 * s, 2 * s:6 * s].all() and not m[2 * s:3 * s, 6 * s:8 * s].any()     # row 0 of R is 11110, then the gap to E
    assert not m[:2 * s].any() and not m[:, :2 * s].any() and not m[11 * s:, 20 * s:].any()   # margins; no field after ROM / ACV
    zero = np.kron(R.glyph("0"), np.ones((s, s), bool))
    assert np.array_equal(m[2 * s:9 * s, (2 + 6 * 7) * s:(2 + 6 * 7 + 5) * s], zero)       # the count's last digit: character 7
    tab = np.array([[0, 3, 5, 9999, 0, 1]], np.int64)                         # one completed rep: ROM 0.05, ACV 99.99
    assert HR.text_lines(tab, 3) == ["REP    1", "ROM 0.05", "ACV99.99"] and HR.text_lines(tab, 2)[1] == "ROM     "
    m = HR.panel_mask(tab, 3, 1, 1, 200)
    cell = m[2 + 9:2 + 9 + 7, 2 + 6 * 5:2 + 6 * 5 + 5]                        # line 1, character 5: the '.'
    want = np.zeros((7, 5), bool)
    want[5:7, 1:3] = True
    assert np.array_equal(cell, want) and np.array_equal(HR.glyph("."), want)


def test_reference_field_and_centi():
    assert HR.field(1, 5) == " 0.05" and HR.field(1, 9999) == "99.99" and HR.field(0, 9999) == "     " and HR.field(3, 120) == " 1.20"
    assert HR.centi(1.115) == int(np.rint(np.float64(1.115) * np.float64(100.0)))          # the library's rounding: the double product, ties to even
    assert HR.centi(0.125) == 12 and HR.centi(0.135) == int(np.rint(0.135 * 100.0)) and HR.centi(0.5) == 50
    assert HR.centi(float("nan")) == 0 and HR.centi(0.0) == 0 and HR.centi(-1.0) == 0 and HR.centi(1e9) == 9999 and HR.centi(float("inf")) == 9999
    t = HR.table([(1 / FPS, 4 / FPS, 0.6, 0.4, 0.3, 0), (4 / FPS, 4 / FPS, 0.4, 0.4, 0.3, 2), (4 / FPS, 10 / FPS, 0.4, 0.6, 0.25, 1)], FPS)
    assert t.tolist() == [[1, 4, 30, 300, 0, 1], [4, 4, 30, 0, 2, 1], [4, 10, 25, 125, 1, 1]]      # duration 0: ACV 0


def test_reference_bars_by_hand():
    s = 2
    tab = np.array([[0, 3, 10, 1, 0, 1], [3, 6, 10, 50, 1, 1], [6, 9, 10, 201, 0, 2]], np.int64)     # ACV 1 cm/s, then 201 cm/s
    assert HR.bar_heights(tab, 9, s, 200) == [1, 12 * s, 0, 0, 0, 0, 0, 0]    # 1 * 24 / 200 = 0 -> the stub of 1; above full scale -> 12 s
    assert HR.bar_heights(tab, 8, s, 200) == [1, 0, 0, 0, 0, 0, 0, 0]
    assert HR.bar_heights(tab, 9, s, 402) == [1, 12, 0, 0, 0, 0, 0, 0]        # 201 * 24 / 402 = 12
    m = HR.panel_mask(tab, 9, 1, s, 200)
    assert m[41 * s - 1, 2 * s:7 * s].all() and not m[41 * s - 2, 2 * s:7 * s].any()
    assert m[29 * s:41 * s, 8 * s:13 * s].all() and not m[29 * s - 1, 8 * s:13 * s].any() and not m[41 * s, 8 * s:13 * s].any()
    assert not m[29 * s:41 * s, 7 * s:8 * s].any() and not m[29 * s:41 * s, 13 * s:].any()
    nine = np.array([[2 * i, 2 * i + 1, 10, 10 * (i + 1), 0, i + 1] for i in range(10)], np.int64)
    assert HR.bar_heights(nine, 19, 1, 200) == [10 * (i + 1) * 12 // 200 for i in range(2, 10)]       # ten reps: the window holds reps 2..9


def test_reference_timeline_edges_by_hand():
    tab = np.array([[10, 20, 10, 10, 0, 1], [20, 30, 10, 10, 1, 1], [30, 33, 0, 0, 2, 1]], np.int64)
    assert HR.timeline_phase(tab, 10) is None and HR.timeline_phase(tab, 11) == 0 and HR.timeline_phase(tab, 20) == 0
    assert HR.timeline_phase(tab, 21) == 1 and HR.timeline_phase(tab, 31) == 2 and HR.timeline_phase(tab, 34) is None
    m = HR.panel_mask(tab, 36, 1, 1, 200)                                     # column c is frame 36 - (46 - c) = c - 10
    col = lambda fc: m[:, 2 + fc + 10]
    assert not col(10)[43:47].any()                                           # fc = fs: not in the phase
    assert col(11)[43:47].all() and col(20)[43:47].all() and not col(11)[41:43].any() and not col(11)[47:].any()    # fc = fe: in it
    assert col(21)[45:47].all() and not col(21)[43:45].any() and col(30)[45:47].all()                 # eccentric: the lower half
    assert not col(31)[43:47].any() and not col(34)[43:47].any()              # a hold, and past the table
    early = HR.panel_mask(tab, 12, 1, 1, 200)                                 # columns with fc < 1 cover nothing
    assert not early[43:47, :2 + 46 - 1].any() and early[43:47, 2 + 45].all() and early[43:47, 2 + 46].all()
    step = HR.panel_mask(tab, 36, 4, 1, 200)                                  # frame_step 4: column c is frame 36 - 4 (46 - c)
    assert np.nonzero(step[43, :])[0].tolist() == [2 + 46 - k for k in (6, 5, 4)]             # frames 12, 16, 20: concentric
    assert np.nonzero(step[45, :])[0].tolist() == [2 + 46 - k for k in (6, 5, 4, 3, 2)]       # and 24, 28: eccentric; 32 is the hold


def test_reference_chroma_rule_and_extent():
    mask = np.zeros((50, 52), bool)
    mask[3, 5] = True
    fg, bg = (252, 3, 115), (10, 200, 30)
    (Yf, Uf, Vf), (Yb, Ub, Vb) = R.yuv_colour(fg), R.yuv_colour(bg)
    H, W, x, y = 60, 64, 6, 4
    for fmt in ("nv12", "i420"):
        out = HR.paint_panel(np.full((H * 3 // 2, W), 7, np.uint8), mask, x, y, fmt, fg, bg).reshape(-1)
        luma = out[:H * W].reshape(H, W)
        want = np.full((H, W), 7, np.uint8)
        want[y:y + 50, x:x + 52] = Yb
        want[y + 3, x + 5] = Yf
        assert np.array_equal(luma, want), fmt
        if fmt == "nv12":
            uv = out[H * W:].reshape(H // 2, W // 2, 2)
            U, V = uv[:, :, 0], uv[:, :, 1]
        else:
            q = (H // 2) * (W // 2)
            U, V = out[H * W:H * W + q].reshape(H // 2, W // 2), out[H * W + q:].reshape(H // 2, W // 2)
        for plane, f_, b_ in ((U, Uf, Ub), (V, Vf, Vb)):
            want = np.full((H // 2, W // 2), 7, np.uint8)
            want[y // 2:y // 2 + 25, x // 2:x // 2 + 26] = b_
            want[(y + 3) >> 1, (x + 5) >> 1] = f_                             # one covered pixel of the quad: the sample gets fg's chroma
            assert np.array_equal(plane, want), fmt
    rgb = HR.paint_panel(np.full((H, W, 3), 7, np.uint8), mask, 7, 5, "rgb24", fg, bg)
    want = np.full((H, W, 3), 7, np.uint8)
    want[5:55, 7:59] = bg
    want[5 + 3, 7 + 5] = fg
    assert np.array_equal(rgb, want)


def test_track_and_overlay_help_list_hud():
    from vbt_amd.cli import main
    for cmd in ("track", "overlay"):
        res = CliRunner().invoke(main, [cmd, "--help"])
        assert res.exit_code == 0, res.output
        for opt in ("--hud", "--plate_diameter", "--hud_scale", "--hud_pos"):
            assert opt in res.output, (cmd, opt)
    res = CliRunner().invoke(main, ["track", "nothing.npy", "--hud"])
    assert res.exit_code == 2 and "--video_dir" in res.output
    res = CliRunner().invoke(main, ["overlay", "nothing.npy", "frame.pkl.gz", "--hud"])
    assert res.exit_code == 2 and "file name" in res.output
