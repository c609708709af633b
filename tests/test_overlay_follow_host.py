"""Follow mode of the tracking overlay without a GPU (include/vbt_hip.h, "Following a device row log"): the per-row step of
vbt_amd/csrc/overlay_core.h as a stand-alone host program under -fsanitize=address,undefined (tests/fuzz/overlay_follow_check.cc, run
as a program, never loaded into Python) against the sorted-mode reference (tests/overlay_ref.py) for every way of cutting the log
into updates, the rows it must skip, the argument refusals made before any device call, the bindings and the CLI option."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from click.testing import CliRunner

import overlay_follow_util as U
import overlay_ref as R
from test_gpu_overlay import FPS, H, W, synthetic_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vbt_overlay_follow", "vbt_overlay_follow_update", "vbt_overlay_follow_status", "vbt_tracker_rows_dev", "vbt_pipeline_overlay_draw")
MAX_FRAME = 132


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("follow") / "overlay_follow_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "fuzz", "overlay_follow_check.cc"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def log():
    out = U.emission_log(synthetic_rows())
    out.setflags(write=False)
    return out


def run(harness, tmp_path, log, cut, trail=120, max_frame=MAX_FRAME, mrpf=25):
    """the program's output parsed: (geometry [n, 8], trails per row, {frame: rows}, rows consumed, flags, raw text)"""
    path = str(tmp_path / "log.bin")
    np.ascontiguousarray(log).tofile(path)
    p = subprocess.run([harness, path, str(H), str(W), repr(FPS), str(trail), str(max_frame), str(mrpf), str(cut)], capture_output=True, text=True,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, (p.stdout[-1000:], p.stderr[-3000:])
    geo, trails, frames, status = [], [], {}, None
    for ln in p.stdout.splitlines():
        head, _, rest = ln.partition(":")
        if head.startswith("row"):
            assert int(head.split()[1]) == len(geo)
            g, _, t = rest.partition("|")
            geo.append([int(v) for v in g.split()])
            trails.append(np.array([[int(c) for c in pt.split(",")] for pt in t.split()], np.int64).reshape(-1, 2))
        elif head.startswith("frame"):
            frames[int(head.split()[1])] = [int(v) for v in rest.split()]
        elif head == "status":
            status = [int(v) for v in rest.split()]
    return np.array(geo, np.int64).reshape(-1, 8), trails, frames, status[0], status[1], p.stdout


def test_the_log_interleaves_ids_and_holds_every_trail_length(log):
    """what the tests below are about, on the reference's integers: emission order, ids 1 and 12 interleaved, the trail lengths at and
    around the 16-segment chunks and the cap"""
    assert len(log) == 133 and (np.diff(log["time"]) >= 0).all()
    f = U.frames_of(log, FPS)
    at = {int(fr): log["id"][f == fr].tolist() for fr in (127, 128, 129)}
    assert at == {127: [1, 12], 128: [1], 129: [1, 12]}
    geo, trails = U.reference(log, FPS, H, W)
    one = geo[log["id"] == 1]
    assert one[:, 7].tolist() == [min(k, 120) for k in range(1, 132)]                 # depths 1..131, capped
    assert {1, 2, 16, 17, 18, 120} <= set(geo[:, 7].tolist())
    assert all(len(t) == geo[i, 7] and t[0].tolist() == geo[i, 1:3].tolist() for i, t in enumerate(trails))


def test_every_cut_gives_the_reference(harness, tmp_path, log):
    geo_ref, trails_ref = U.reference(log, FPS, H, W)
    f = U.frames_of(log, FPS)
    texts = []
    for cut in (1, -1, 64, 0):                          # one row at a time, one frame at a time, 64 rows, everything at once
        geo, trails, frames, n, flags, text = run(harness, tmp_path, log, cut)
        assert (n, flags) == (len(log), 0), cut
        for k, name in enumerate(R.GEOMETRY):
            assert np.array_equal(geo[:, k], geo_ref[:, k]), (cut, name)
        for i in range(len(log)):
            assert np.array_equal(trails[i], trails_ref[i]), (cut, i)
        assert {fr: sorted(v) for fr, v in frames.items()} == {int(fr): np.nonzero(f == fr)[0].tolist() for fr in np.unique(f)}, cut
        texts.append(text)
    assert all(t == texts[0] for t in texts)


def test_a_short_trail_and_its_chunks(harness, tmp_path, log):
    for trail in (1, 2, 17, 33):
        geo_ref, trails_ref = U.reference(log, FPS, H, W, trail=trail)
        geo, trails, _, _, flags, _ = run(harness, tmp_path, log, 64, trail=trail)
        assert flags == 0 and np.array_equal(geo, geo_ref), trail
        assert all(np.array_equal(a, b) for a, b in zip(trails, trails_ref)), trail


def _insert(log, at, **fields):
    """`log` with a copy of row `at` - fields replaced - put right behind it"""
    rec = log[at:at + 1].copy()
    for k, v in fields.items():
        rec[k] = v
    return np.concatenate([log[:at + 1], rec, log[at + 1:]]), at + 1


CASES = {
    "nan": (dict(x=np.nan), U.BAD_ROW, {}),
    "inf-time": (dict(time=np.inf), U.BAD_ROW, {}),
    "negative-id": (dict(id=-1), U.BAD_ROW, {}),
    "negative-width": (dict(w=-0.1), U.BAD_ROW, {}),
    "time-steps-back": (dict(time=40 / FPS), U.ORDER, {}),
    "frame-above-max": (dict(time=133 / FPS), U.FRAME_RANGE, {}),
    "frame-zero": (dict(id=77, time=0.0), U.FRAME_RANGE, {}),
    "frame-full": (dict(id=30), U.FRAME_FULL, dict(mrpf=2)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_exactly_the_bad_row_is_skipped_and_flagged(harness, tmp_path, log, case):
    fields, flag, kw = CASES[case]
    f = U.frames_of(log, FPS)
    at = int(np.nonzero((f == 127) & (log["id"] == 12))[0][0]) if case == "frame-full" else (len(log) - 1 if case == "frame-above-max" else 60)
    bad_log, bad = _insert(log, at, **fields)
    clean = run(harness, tmp_path, log, 64, **kw)
    assert clean[4] == 0
    for cut in (1, 64, 0):
        geo, trails, frames, n, flags, _ = run(harness, tmp_path, bad_log, cut, **kw)
        assert n == len(bad_log) and flags == flag, (case, cut, flags)
        assert geo[bad, 7] == 0 and len(trails[bad]) == 0
        if flag == U.BAD_ROW:
            assert not geo[bad].any()
        keep = np.arange(len(bad_log)) != bad
        assert np.array_equal(geo[keep], clean[0]), (case, cut)                      # every other row is as in the clean log
        assert all(np.array_equal(a, b) for a, b in zip([t for i, t in enumerate(trails) if i != bad], clean[1])), (case, cut)
        back = lambda i: i - (i > bad)
        assert all(bad not in v for v in frames.values())
        assert {fr: [back(i) for i in v] for fr, v in frames.items()} == clean[2], (case, cut)


def test_all_bad_rows_together_set_all_flags(harness, tmp_path, log):
    f = U.frames_of(log, FPS)
    work, bads = log, []
    for case in ("frame-above-max", "frame-full", "time-steps-back", "nan"):           # from the back: earlier indices stay
        at = int(np.nonzero((f == 127) & (log["id"] == 12))[0][0]) if case == "frame-full" else (len(log) - 1 if case == "frame-above-max" else 60)
        work, bad = _insert(work, at + (1 if case == "nan" else 0), **CASES[case][0])
        bads = [b + (b >= bad) for b in bads] + [bad]
    clean = run(harness, tmp_path, log, 0, mrpf=2)
    geo, trails, frames, n, flags, _ = run(harness, tmp_path, work, 7, mrpf=2)
    assert flags == U.BAD_ROW | U.ORDER | U.FRAME_RANGE | U.FRAME_FULL and n == len(work)
    keep = ~np.isin(np.arange(len(work)), bads)
    assert (geo[~keep, 7] == 0).all() and np.array_equal(geo[keep], clean[0])


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib
    return _lib, _lib.lib()


def test_entry_points_are_exported_declared_and_bound():
    _lib_mod, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "vbt_hip.h")).read()
    assert "Following a device row log" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in _lib_mod.declared_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, code), name
    for name, bit in (("BAD_ROW", 1), ("ORDER", 2), ("FRAME_RANGE", 4), ("FRAME_FULL", 8), ("REWOUND", 16)):
        assert re.search(r"VBT_OVERLAY_FOLLOW_%s\s*=\s*%d\b" % (name, bit), code), name
    from vbt_amd import overlay
    assert overlay.FOLLOW_FLAGS == {1: "BAD_ROW", 2: "ORDER", 4: "FRAME_RANGE", 8: "FRAME_FULL", 16: "REWOUND"}
    assert overlay.follow_flag_names(10) == ["ORDER", "FRAME_FULL"]
    for name in ("follow", "follow_update", "follow_status"):
        assert callable(getattr(overlay.Overlay, name))


def test_follow_refuses_bad_arguments_before_any_device_call():
    _lib_mod, L = _lib()
    mem = np.zeros(16, np.int64)                                   # stands for device memory: never looked at before the refusal
    rows, nrows = mem.ctypes.data, mem.ctypes.data + 64

    def follow(rows=rows, nrows=nrows, cap=100, max_frame=50, mrpf=25, fps=30.0):
        rc = L.vbt_overlay_follow(None, rows, nrows, cap, max_frame, mrpf, fps)
        return rc, L.vbt_last_error().decode()
    rc, msg = follow()
    assert rc == -1 and "handle" in msg                             # good arguments get as far as the (missing) handle
    for kw, word in ((dict(rows=None), "NULL"), (dict(nrows=None), "NULL"), (dict(cap=0), "rows_cap"), (dict(max_frame=0), "max_frame"),
                     (dict(max_frame=(1 << 24) + 1), "max_frame"), (dict(mrpf=0), "max_rows_per_frame"), (dict(mrpf=65), "max_rows_per_frame"),
                     (dict(fps=0.0), "fps"), (dict(fps=float("nan")), "fps"), (dict(fps=float("inf")), "fps"), (dict(fps=-30.0), "fps")):
        rc, msg = follow(**kw)
        assert rc == -1 and word in msg and "handle" not in msg, (kw, msg)
    assert L.vbt_overlay_follow_update(None, None) == -1
    n, flags = ctypes.c_int32(), ctypes.c_int32()
    assert L.vbt_overlay_follow_status(None, ctypes.byref(n), ctypes.byref(flags), None) == -1
    assert L.vbt_pipeline_overlay_draw(None, None, None, 1, 1, 1, None) == -1
    with pytest.raises(_lib_mod.VbtArgError):
        _lib_mod.check(follow(cap=0)[0])


def test_tracker_rows_dev_refuses_bad_arguments_before_any_device_call():
    _, L = _lib()
    a, b, cap = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int()
    assert L.vbt_tracker_rows_dev(None, 0, ctypes.byref(a), ctypes.byref(b), ctypes.byref(cap)) == -1
    assert "NULL" in L.vbt_last_error().decode()


def test_track_help_lists_one_pass_and_the_cli_refuses_what_it_cannot_do(tmp_path):
    from vbt_amd.cli import main
    res = CliRunner().invoke(main, ["track", "--help"])
    assert res.exit_code == 0 and "--one_pass" in res.output
    src = str(tmp_path / "missing.npy")                            # never opened: the refusals come first
    out = str(tmp_path / "out")
    for extra, word in ((["--video_dir", out, "--hud"], "--hud"), (["--video_dir", out, "--concurrent", "2"], "--concurrent"), ([], "--video_dir")):
        res = CliRunner().invoke(main, ["track", src, "--one_pass"] + extra)
        assert res.exit_code == 2 and "--one_pass" in res.output and word in res.output, (extra, res.output)
        assert not os.path.exists(out)
