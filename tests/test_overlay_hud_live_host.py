"""Rep panel that follows the live analysis, without a GPU (include/vbt_hip.h, "Rep panel from the live analysis"): the new entry points
of the C ABI and their bindings, the refusals vbt_overlay_hud_follow makes before any device call, the per-phase record functions of
vbt_amd/csrc/overlay_core.h - shared by vbt_overlay_set_hud and the follow kernel - as a stand-alone host program under
-fsanitize=address,undefined (tests/fuzz/overlay_hud_follow_check.cc, run as a program, never loaded into Python) against the numpy
statement of the table (tests/overlay_hud_ref.py), and the CLI flag."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from click.testing import CliRunner

import overlay_hud_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vbt_overlay_hud_follow", "vbt_overlay_hud_follow_update", "vbt_overlay_hud_follow_status", "vbt_overlay_hud_follow_flush")
FLAGGED, BAD_PHASE, CAPACITY = 1, 2, 4
COLS = ["time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width"]
CLIPS = ("013", "017", "029")


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib
    return _lib, _lib.lib()


def test_entry_points_are_exported_declared_and_bound():
    _lib_mod, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "vbt_hip.h")).read()
    assert "Rep panel from the live analysis" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in _lib_mod.declared_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, code), name
    for name, bit in (("FLAGGED", FLAGGED), ("BAD_PHASE", BAD_PHASE), ("CAPACITY", CAPACITY)):
        assert re.search(r"VBT_OVERLAY_HUD_FOLLOW_%s\s*=\s*%d\b" % (name, bit), code), name
    from vbt_amd import overlay
    assert overlay.HUD_FOLLOW_FLAGS == {1: "FLAGGED", 2: "BAD_PHASE", 4: "CAPACITY"}
    assert overlay.hud_follow_flag_names(6) == ["BAD_PHASE", "CAPACITY"]
    for name in ("hud_follow", "hud_follow_update", "hud_follow_status", "hud_follow_flush", "hud_table"):
        assert callable(getattr(overlay.Overlay, name))


def test_hud_follow_refuses_bad_arguments_before_any_device_call():
    _lib_mod, L = _lib()

    def follow(fps=30.0, params=True, **kw):
        p = _lib_mod.OverlayHudParams()
        L.vbt_overlay_hud_default_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        rc = L.vbt_overlay_hud_follow(None, ctypes.byref(p) if params else None, None, 0, fps)
        return rc, L.vbt_last_error().decode()
    rc, msg = follow()
    assert rc == -1 and "vbt_overlay_hud_follow" in msg and "handle" in msg          # good arguments get as far as the (missing) handle
    rc, msg = follow(params=False)
    assert rc == -1 and "params" in msg and "handle" not in msg
    for fps in (0.0, -30.0, float("nan"), float("inf")):
        rc, msg = follow(fps)
        assert rc == -1 and "fps" in msg and "handle" not in msg, (fps, msg)
    for kw, word in ((dict(scale=0), "scale"), (dict(scale=65), "scale"), (dict(full_scale_cm=0), "full_scale_cm"),
                     (dict(full_scale_cm=100001), "full_scale_cm"), (dict(x=-1), "negative"), (dict(y=-2), "negative")):
        rc, msg = follow(**kw)
        assert rc == -1 and word in msg and "vbt_overlay_hud_follow" in msg and "handle" not in msg, (kw, msg)
    assert L.vbt_overlay_hud_follow_update(None, 0, None) == -1 and "handle" in L.vbt_last_error().decode()
    assert L.vbt_overlay_hud_follow_flush(None, 1) == -1 and "handle" in L.vbt_last_error().decode()
    leader, n, flags = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
    assert L.vbt_overlay_hud_follow_status(None, ctypes.byref(leader), ctypes.byref(n), ctypes.byref(flags), None) == -1
    assert "NULL" in L.vbt_last_error().decode()
    with pytest.raises(_lib_mod.VbtArgError):
        _lib_mod.check(follow(scale=0)[0])


def test_set_hud_keeps_its_refusals_and_messages():
    """vbt_overlay_set_hud now makes its tests through the shared functions: the same results, the same words, the same order"""
    _lib_mod, L = _lib()
    p = _lib_mod.OverlayHudParams()
    L.vbt_overlay_hud_default_params(ctypes.byref(p))
    ph = np.array([[1 / 30, 11 / 30, 0.4, 0.6, 0.5, 1.0], [11 / 30, 21 / 30, 0.6, 0.4, 0.5, 0.0]], np.float64)

    def set_hud(a):
        a = np.ascontiguousarray(a, np.float64)
        return L.vbt_overlay_set_hud(None, ctypes.byref(p), a.ctypes.data, len(a), 30.0, None), L.vbt_last_error().decode()
    assert set_hud(ph) == (-1, "vbt_overlay_set_hud: handle is NULL")
    bad = ph.copy()
    bad[1, 5], bad[1, 1] = 3.0, np.nan                                             # two faults in one phase: the first test wins
    assert set_hud(bad) == (-1, "vbt_overlay_set_hud: phase 1 holds a non-finite value")
    bad = ph.copy()
    bad[0, 5], bad[1, 1] = 0.5, 0.0                                                # two bad phases: the first phase wins
    assert set_hud(bad) == (-1, "vbt_overlay_set_hud: phase 0 has type 0.5, not 0, 1 or 2")
    bad = ph.copy()
    bad[1, 1] = 10 / 30
    assert set_hud(bad) == (-1, "vbt_overlay_set_hud: phase 1 ends before it starts (time_end < time_start)")
    bad = ph.copy()
    bad[1, 0] = 0.5 / 30
    assert set_hud(bad) == (-1, "vbt_overlay_set_hud: phases are not ordered in time at phase 1")
    bad = ph.copy()
    bad[1, 1] = ((1 << 24) + 1) / 30
    assert set_hud(bad) == (-4, "vbt_overlay_set_hud: phase 1 ends at frame 16777217, above 16777216")


# ---- the shared record arithmetic under sanitizers ----

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hud_follow") / "overlay_hud_follow_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "fuzz", "overlay_hud_follow_check.cc"), "-o", exe])
    return exe


def run(harness, tmp_path, phases, fps, cap=512):
    """the program's output parsed: (per-phase codes, table int64 [n, 6], records, flags)"""
    path = str(tmp_path / "phases.bin")
    np.ascontiguousarray(phases, np.float64).reshape(-1, 6).tofile(path)
    p = subprocess.run([harness, path, repr(float(fps)), str(cap)], capture_output=True, text=True,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, (p.stdout[-1000:], p.stderr[-3000:])
    codes, tab, status = [], [], None
    for ln in p.stdout.splitlines():
        head, _, rest = ln.partition(":")
        if head.startswith("phase"):
            assert int(head.split()[1]) == len(codes)
            codes.append([int(v) for v in rest.split()])
        elif head.startswith("rec"):
            assert int(head.split()[1]) == len(tab)
            tab.append([int(v) for v in rest.split()])
        elif head == "status":
            status = [int(v) for v in rest.split()]
    return codes, np.array(tab, np.int64).reshape(-1, 6), status[0], status[1]


def check_code(ph, i):
    """numpy statement of the tests vbt_overlay_set_hud makes on phase i, in its order: 0 ok, 1 non-finite, 2 type, 3 ends before it
    starts, 4 times decreasing along the table"""
    r = ph[i]
    if not np.isfinite(r).all():
        return 1
    if r[5] not in (0.0, 1.0, 2.0):
        return 2
    if r[1] < r[0]:
        return 3
    if i > 0 and (r[0] < ph[i - 1, 0] or r[1] < ph[i - 1, 1]):
        return 4
    return 0


def corpus_phases():
    """{clip: (float64 [P, 6], fps)}: the phases oracle/velocity.py gives for the export id of the reference clips"""
    from oracle import velocity as ov
    from test_oracle_ocsort_corpus import load_all
    corpus = load_all()
    out = {}
    for clip in CLIPS:
        g, best, fps = corpus[clip]
        m = np.asarray(g["id"]) == best
        cols = ov.preprocess(*[np.asarray(g[c])[m].tolist() for c in COLS])
        vt = ov.VelocityTracker(0.45)
        for i in range(len(cols[0])):
            vt.process_measurements(*[c[i] for c in cols])
        vt.end_processing()
        out[clip] = (np.asarray([p.as_row() for p in vt.phases], np.float64).reshape(-1, 6), float(fps))
    return out


def test_corpus_phase_lists_give_the_reference_table(harness, tmp_path):
    total = 0
    for clip, (ph, fps) in corpus_phases().items():
        assert len(ph) > 0, clip
        codes, tab, n, flags = run(harness, tmp_path, ph, fps)
        assert (n, flags) == (len(ph), 0) and all(c == [0, 0] for c in codes), clip
        assert np.array_equal(tab, HR.table(ph, fps)), clip
        for cut in (1, len(ph) // 2):                                          # a prefix - what the live panel sees - is the table's prefix
            _, part, m, fl = run(harness, tmp_path, ph[:cut], fps)
            assert (m, fl) == (cut, 0) and np.array_equal(part, tab[:cut]), (clip, cut)
        total += n
    assert total >= 10


def test_ties_zero_durations_and_the_rounding(harness, tmp_path):
    fps = 30.0
    ph = np.array([[1 / fps, 4 / fps, 0.6, 0.4, 0.125, 0],            # centi(0.125): 12.5 ties to even
                   [4 / fps, 4 / fps, 0.4, 0.4, 0.3, 2],              # time_end == time_start: ACV 0
                   [4 / fps, 10 / fps, 0.4, 0.6, 0.135, 1],
                   [10.5 / fps, 12.5 / fps, 0.6, 0.4, 1.115, 0],      # frame numbers on ties: llrint(10.5) = 10, llrint(12.5) = 12
                   [12.5 / fps, 12.5 / fps, 0.4, 0.4, 0.0, 0],        # a concentric phase of no duration still counts
                   [13 / fps, 14 / fps, 0.4, 0.6, -0.2, 1],           # a negative ROM shows as 0
                   [14 / fps, 15 / fps, 0.4, 0.6, 250.0, 0]], np.float64)   # above 99.99: clamped
    codes, tab, n, flags = run(harness, tmp_path, ph, fps)
    assert (n, flags) == (len(ph), 0) and all(c == [0, 0] for c in codes)
    want = HR.table(ph, fps)
    assert np.array_equal(tab, want)
    assert tab[0].tolist() == [1, 4, 12, 125, 0, 1] and tab[1].tolist() == [4, 4, 30, 0, 2, 1]
    assert tab[3, :2].tolist() == [HR.frame_number(10.5 / fps, fps), HR.frame_number(12.5 / fps, fps)]
    assert tab[4, 2:].tolist() == [0, 0, 0, 3] and tab[5, 2] == 0 and tab[6, 2:4].tolist() == [9999, 9999] and tab[6, 5] == 4
    for fps2 in (29.97, 59.94, 240.0):                                       # one multiply before llrint, whatever the rate
        _, t2, _, fl = run(harness, tmp_path, ph, fps2)
        assert fl == 0 and np.array_equal(t2, HR.table(ph, fps2)), fps2
    _, t0, n0, f0 = run(harness, tmp_path, np.zeros((0, 6)), fps)
    assert (n0, f0, len(t0)) == (0, 0, 0)                                     # no phase: no record, no flag


BAD = {
    "nan": ((2, 4), np.nan, 1), "inf-start": ((1, 0), np.inf, 1), "minus-inf": ((0, 3), -np.inf, 1),
    "type-3": ((1, 5), 3.0, 2), "type-negative": ((1, 5), -1.0, 2), "type-half": ((1, 5), 0.5, 2),
    "ends-before": ((2, 1), 20.5 / 30, 3), "start-decreasing": ((2, 0), 10.5 / 30, 4), "end-decreasing": ((1, 1), 31.5 / 30, 4),
}


def _phases(n=4, fps=30.0):
    ph = np.zeros((n, 6), np.float64)
    for i in range(n):
        ph[i] = ((1 + 10 * i) / fps, (11 + 10 * i) / fps, 0.4, 0.6, 0.5, 1 - i % 2)
    return ph


@pytest.mark.parametrize("case", list(BAD))
def test_each_bad_phase_is_flagged_and_blanks_the_table(harness, tmp_path, case):
    (i, k), value, code = BAD[case]
    ph = _phases()
    codes, tab, n, flags = run(harness, tmp_path, ph, 30.0)
    assert (n, flags) == (4, 0) and np.array_equal(tab, HR.table(ph, 30.0))
    ph[i, k] = value
    codes, tab, n, flags = run(harness, tmp_path, ph, 30.0)
    assert (n, flags, len(tab)) == (0, BAD_PHASE, 0), case
    want = [check_code(ph, j) for j in range(len(ph))]
    assert [c[0] for c in codes] == want and next(c for c in want if c) == code, (case, codes)        # (a decreasing end shows at the next phase)


def test_frame_above_2_24_and_capacity(harness, tmp_path):
    ph = _phases()
    ph[3, 1] = (1 << 24) / 30.0
    codes, tab, n, flags = run(harness, tmp_path, ph, 30.0)
    assert (n, flags) == (4, 0) and tab[3, 1] == 1 << 24                       # frame 2^24 itself is allowed
    ph[3, 1] = ((1 << 24) + 1) / 30.0
    codes, tab, n, flags = run(harness, tmp_path, ph, 30.0)
    assert (n, flags) == (0, BAD_PHASE) and codes[3] == [0, 5] and all(c == [0, 0] for c in codes[:3])
    ph = _phases()
    _, tab, n, flags = run(harness, tmp_path, ph, 30.0, cap=4)
    assert (n, flags) == (4, 0)
    _, tab, n, flags = run(harness, tmp_path, ph, 30.0, cap=3)                  # more phases than the table holds: nothing is written
    assert (n, flags, len(tab)) == (0, CAPACITY, 0)


# ---- CLI ----

def test_track_help_lists_live_hud_and_the_cli_refuses_what_it_cannot_do(tmp_path):
    from vbt_amd.cli import main
    res = CliRunner().invoke(main, ["track", "--help"])
    assert res.exit_code == 0 and "--live_hud" in res.output
    src = str(tmp_path / "missing.npy")                                       # never opened: the refusals come first
    out = str(tmp_path / "out")
    for extra, word in ((["--video_dir", out], "--one_pass"), (["--one_pass"], "--video_dir"), (["--one_pass", "--video_dir", out, "--hud"], "--hud"),
                        (["--one_pass", "--video_dir", out, "--concurrent", "2"], "--concurrent")):
        res = CliRunner().invoke(main, ["track", src, "--live_hud"] + extra)
        assert res.exit_code == 2 and "--live_hud" in res.output and word in res.output, (extra, res.output)
        assert not os.path.exists(out)
    res = CliRunner().invoke(main, ["track", src, "--one_pass", "--video_dir", out, "--hud"])      # the two-pass panel stays refused, as before
    assert res.exit_code == 2 and "--one_pass cannot draw --hud" in res.output and "only after its last frame" in res.output


def test_a_panel_that_does_not_fit_is_refused_before_anything_is_written(tmp_path):
    from vbt_amd.cli import main
    src = str(tmp_path / "small.npy")
    np.save(src, np.zeros((2, 120, 160, 3), np.uint8))
    out = str(tmp_path / "out")
    for extra, word in ((["--hud_scale", "3"], "does not lie inside"), (["--hud_scale", "1", "--hud_pos", "120,10"], "does not lie inside")):
        res = CliRunner().invoke(main, ["track", src, "--one_pass", "--live_hud", "--video_dir", out] + extra)
        assert res.exit_code == 2 and "--live_hud" in res.output and word in res.output, res.output
        assert not os.path.exists(out)
    raw = str(tmp_path / "small.yuv")
    np.zeros((2, 180, 160), np.uint8).tofile(raw)
    res = CliRunner().invoke(main, ["track", raw, "--pix_fmt", "nv12", "--size", "160x120", "--one_pass", "--live_hud", "--video_dir", out,
                                    "--hud_scale", "1", "--hud_pos", "7,8"])
    assert res.exit_code == 2 and "even" in res.output and not os.path.exists(out), res.output
