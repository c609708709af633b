"""Validation figure without a GPU (include/vbt_hip.h, "Validation figure"): the entry points of the C ABI and their bindings, the
refusals made before any device call with their texts, the numpy statement (tests/validation_ref.py) against results worked out by
hand and against validate.metric_trajectory / validate.compare on the five cases of tests/validation_cases.py, the shared core
(vbt_amd/csrc/validation_core.h) as a stand-alone host program under -fsanitize=address,undefined (tests/fuzz/validation_check.cc, run
as a program, never loaded into Python) against the numpy statement, and the CLI's new options."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from click.testing import CliRunner

import validation_cases as VC
import validation_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vbt_validation_default_params", "vbt_validation_create", "vbt_validation_destroy", "vbt_validation_set", "vbt_validation_stats",
                "vbt_validation_table", "vbt_validation_render")
ARG, CAPACITY, STATE = -1, -4, -5
IDS = ["%dx%d-s%d-t%d" % c for c in VC.CONFIGS]


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib
    return _lib, _lib.lib()


def test_entry_points_are_exported_declared_and_bound():
    _lib_mod, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "vbt_hip.h")).read()
    assert "Validation figure" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in _lib_mod.declared_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert ctypes.sizeof(_lib_mod.ValidationParams) == 36
    p = _lib_mod.ValidationParams()
    L.vbt_validation_default_params(ctypes.byref(p))
    assert {k: getattr(p, k) for k in VR.DEFAULTS} == VR.DEFAULTS and p.reserved == 0
    assert re.search(r"#define\s+VBT_VALIDATION_STAGE_POINTS\s+%d\b" % VR.STAGE_POINTS, code)
    assert re.search(r"#define\s+VBT_VALIDATION_STAGE_RECORDS\s+%d\b" % VR.STAGE_RECORDS, code)
    from vbt_amd import figure, validate
    assert validate.default_params() == VR.DEFAULTS and validate.STATS == VR.STATS and validate.KINDS == VR.KINDS
    assert issubclass(validate.Validation, figure.FigureHandle)
    for name in ("set", "stats", "table", "render", "device_frames", "frames"):
        assert callable(getattr(validate.Validation, name))
    assert callable(validate.validate_many)
    assert "without the figures" not in validate.__doc__ and "p-values" in validate.__doc__


def test_create_refuses_bad_sizes_before_any_device_call():
    _lib_mod, L = _lib()

    def create(**kw):
        p = _lib_mod.ValidationParams()
        L.vbt_validation_default_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        h = ctypes.c_void_p()
        return L.vbt_validation_create(0, ctypes.byref(p), ctypes.byref(h)), L.vbt_last_error().decode(), h.value
    # a 16 pixel panel needs 50 + 4 + 16 columns and 17 + 6 + 23 + 2 * 16 rows at scale 1
    for kw, word in ((dict(width=0), "16384"), (dict(height=16385), "16384"), (dict(scale=0), "scale"), (dict(scale=65), "scale"),
                     (dict(thickness=0), "thickness"), (dict(max_pairs=0), "max_pairs"), (dict(max_pairs=1025), "max_pairs"),
                     (dict(max_rows=1), "max_rows"), (dict(max_ref_rows=(1 << 20) + 1), "max_ref_rows"), (dict(max_grid=1), "max_grid"),
                     (dict(max_pairs=1024, max_rows=1 << 16), "2^26"),
                     (dict(width=69, height=78, scale=1), "plot rectangle"), (dict(width=70, height=77, scale=1), "plot rectangle"),
                     (dict(width=200, height=120, scale=2), "plot rectangle")):
        rc, msg, h = create(**kw)
        assert rc == ARG and word in msg and "vbt_validation_create" in msg and not h, (kw, msg)
    assert L.vbt_validation_create(0, None, None) == ARG and "out" in L.vbt_last_error().decode()


def test_set_stats_render_and_table_refuse_before_the_handle_is_looked_at():
    _lib_mod, L = _lib()
    good = VC.pairs()[:3]

    def vset(pairs, kinds=None, plate=0.5, rate=30.0, n=None, null=()):
        refs = np.ascontiguousarray(np.concatenate([np.asarray(r, np.float64).reshape(-1, 3) for r, _ in pairs]))
        rows = np.ascontiguousarray(np.concatenate([np.asarray(k, np.float64).reshape(-1, 5) for _, k in pairs]))
        rc_ = np.array([len(r) for r, _ in pairs], np.int32)
        kc = np.array([len(k) for _, k in pairs], np.int32)
        kd = np.array(kinds if kinds is not None else [0] * len(pairs), np.int32)
        args = dict(kinds=kd.ctypes.data, ref=refs.ctypes.data, ref_counts=rc_.ctypes.data, rows=rows.ctypes.data, row_counts=kc.ctypes.data)
        args.update({k: None for k in null})
        rc = L.vbt_validation_set(None, len(pairs) if n is None else n, args["kinds"], plate, rate, args["ref"], args["ref_counts"], args["rows"],
                                  args["row_counts"], None)
        return rc, L.vbt_last_error().decode()

    def edit(i, which, fn):
        """the good pairs with pair i's reference (0) or tracked rows (1) changed by fn"""
        out = [list(p) for p in good]
        a = np.array(out[i][which])
        out[i][which] = fn(a)
        return [tuple(p) for p in out]

    def put(r, c, v):
        def fn(a):
            a[r, c] = v
            return a
        return fn
    assert vset(good) == (ARG, "vbt_validation_set: handle is NULL")                # good arguments get as far as the (missing) handle
    assert vset(good, kinds=[1, 0, 1]) == (ARG, "vbt_validation_set: handle is NULL")
    for rc_msg, code, words in (
            (vset(good, n=-1), ARG, ("n -1",)),
            (vset(good, null=("ref",)), ARG, ("bad argument",)),
            (vset(good, null=("kinds",)), ARG, ("bad argument",)),
            (vset(good, n=1025), CAPACITY, ("1025 pairs",)),
            (vset(good, kinds=[0, 2, 0]), ARG, ("pair 1", "kind 2")),
            (vset(good, plate=0.0), ARG, ("plate_diameter 0",)),
            (vset(good, plate=float("nan")), ARG, ("plate_diameter nan",)),
            (vset(good, rate=float("inf")), ARG, ("rate inf",)),
            (vset(good, rate=-30.0), ARG, ("rate -30",)),
            (vset(edit(1, 0, put(7, 2, np.nan))), ARG, ("pair 1, reference row 7", "not finite")),
            (vset(edit(2, 1, put(1, 4, np.inf))), ARG, ("pair 2, tracked row 1", "not finite")),
            (vset(edit(0, 1, put(5, 3, 0.0))), ARG, ("pair 0, tracked row 5", "plate size")),
            (vset(edit(0, 1, put(6, 4, -0.2))), ARG, ("pair 0, tracked row 6", "plate size")),
            (vset(edit(1, 0, lambda a: a[:1])), ARG, ("pair 1", "1 reference rows", "fewer than 2")),
            (vset(edit(1, 1, lambda a: a[:0])), ARG, ("pair 1", "0 tracked rows", "fewer than 2")),
            (vset(edit(0, 0, put(9, 0, 0.35 + 0.06 * 8))), ARG, ("pair 0, reference row 9", "rise strictly")),
            (vset(edit(0, 1, put(3, 0, 0.1))), ARG, ("pair 0, tracked row 3", "rise strictly")),
            (vset(edit(0, 0, lambda a: a + np.array([100.0, 0, 0]))), ARG, ("pair 0", "no common time span")),
            (vset(good, rate=10.0), ARG, ("pair 2", "n = 1", "fewer than 2"))):
        assert rc_msg[0] == code and all(w in rc_msg[1] for w in words) and "vbt_validation_set" in rc_msg[1] and "handle" not in rc_msg[1], (rc_msg, words)
    # the order: the kind before the plate diameter before the rows; a non-finite value before the plate size before the count before the time
    assert "kind" in vset(edit(0, 1, put(0, 0, np.nan)), kinds=[0, 0, 5], plate=-1.0)[1]
    assert "plate_diameter" in vset(edit(0, 1, put(0, 0, np.nan)), plate=-1.0)[1]
    assert "not finite" in vset(edit(0, 1, lambda a: put(0, 3, -1.0)(put(2, 1, np.nan)(a))))[1]
    assert "plate size" in vset(edit(0, 1, lambda a: put(0, 3, -1.0)(a)[:1]))[1]
    both = edit(0, 1, put(3, 0, 0.1))
    both[0] = (both[0][0][:1], both[0][1])
    assert "fewer than 2" in vset(both)[1]
    assert L.vbt_validation_render(None, None, 0, 1, None) == ARG and "NULL" in L.vbt_last_error().decode()
    assert L.vbt_validation_stats(None, None, 0) == ARG and "vbt_validation_stats" in L.vbt_last_error().decode()
    n = ctypes.c_int()
    assert L.vbt_validation_table(None, 0, None, None, 0, ctypes.byref(n), None, 0, ctypes.byref(n), None, None, 0, ctypes.byref(n), None, 0, ctypes.byref(n)) == ARG
    from vbt_amd import validate
    with pytest.raises(ValueError, match="jpg or ppm"):
        validate.validate_many(good, "kinovea", fig_dir="x", fig_format="png")
    with pytest.raises(ValueError, match="kinovea"):
        validate.validate_many(good, "vicon")


def test_the_sum_order_by_hand():
    """Two sums whose value depends on the order.  (1) v[0] = 1e16, v[256] = 1, v[1] = -1e16: lane 0's partial is 1e16 + 1 = 1e16 (the 1
    is lost), lane 1's is -1e16, and the tree's last step adds them: 0, where a left-to-right or pairwise sum gives 1.
    (2) v[0] = 1e16, v[128] = -1e16, v[1] = 1: the tree's first step cancels lanes 0 and 128, the last adds lane 1: 1, where a
    left-to-right sum loses the 1."""
    v = np.zeros(300)
    v[0], v[256], v[1] = 1e16, 1.0, -1e16
    assert VR.fsum(v) == 0.0 and np.sum(v) == 1.0
    v = np.zeros(200)
    v[0], v[128], v[1] = 1e16, -1e16, 1.0
    assert VR.fsum(v) == 1.0 and (1e16 + 1.0) - 1e16 == 0.0
    assert VR.fsum(np.ones(777)) == 777.0 and VR.fsum([]) == 0.0 and VR.fsum([0.1, 0.2]) == 0.1 + 0.2


def test_pair_c_by_hand():
    """Pair (c), plate 0.5, kinovea.  Rolling(5) of x = (0.4, 0.42): (0.4, 0.41); the width stays 0.2: x = (1, 1.025) m, mean 1.0125;
    the reference's mean x is 0.125: shift -0.8875, x = (0.1125, 0.1375).  y = -(0.5, 0.525) * 0.5 / (0.2, 0.205) = (-1.25, -1.2804878...),
    shifted so that its mean is 0.15.  n = int(0.1 * 30) = 3: ts = 0, 0.05, 0.1; reference x 0.1, 0.125, 0.15 against 0.1125, 0.125, 0.1375:
    mse_x = 2 * 0.0125^2 / 3, r_x = 1.  X range: 0.1 .. 0.15, margin 0.0025; Y range 0.1 .. 0.2, margin 0.005: dX = 0.055 < dY = 0.11, so
    the X panel becomes 0.0975 - 0.055 .. 0.1525 + 0.055.  On the 160 x 100 figure (panels 106 x 27 at (50, 17) and (50, 50)) the time
    axis is 0 .. 0.1: columns 0 and 105; one tick at 0 s, labelled."""
    ref, rows = VC.pairs()[2]
    q = VR.prepare(ref, rows, "kinovea", 0.5, 30.0, **VC.params(VC.CONFIGS[0]))
    np.testing.assert_allclose(q["traj"][:, 1], [0.1125, 0.1375], rtol=1e-12)
    ym = np.array([-1.25, -0.525 * 0.5 / 0.205])
    np.testing.assert_allclose(q["traj"][:, 2], ym + (0.15 - ym.mean()), rtol=1e-12)
    np.testing.assert_allclose(q["grid"][:, 0], [0, 0.05, 0.1], rtol=1e-15)
    np.testing.assert_allclose(q["grid"][:, 1], [0.1, 0.125, 0.15], rtol=1e-12)
    np.testing.assert_allclose(q["grid"][:, 2], [0.1125, 0.125, 0.1375], rtol=1e-12)
    np.testing.assert_allclose(q["stats"], [2 * 0.0125 ** 2 / 3, 2 * (0.2 - q["traj"][0, 2]) ** 2 / 3, 1.0, 1.0, 3, 0.0, 0.1, 0], rtol=1e-9)
    np.testing.assert_allclose(q["head"], [0, 0.1, 0.0425, 0.2075, 0.095, 0.205], rtol=1e-12, atol=1e-15)
    G = VR.geom(**VC.params(VC.CONFIGS[0]))
    assert (G["X0"], G["Y0"], G["Y1"], G["PW"], G["PH"]) == (50, 17, 50, 106, 27)
    assert list(q["counts"]) == [2, 2, 2, 2] and [list(p[:2]) for p in q["pts"][:2]] == [[0, VR.FR.row(0.1, 0.0425, 0.2075, 27)], [105, VR.FR.row(0.15, 0.0425, 0.2075, 27)]]
    assert list(q["pts"][:, 2]) == [0, 1] * 4
    texts = ["".join(chr((int(r[12 + k // 4]) >> (8 * (k % 4))) & 255) for k in range(r[9])) for r in q["recs"] if r[0] in (VR.TEXT, VR.LEGEND_TEXT)]
    assert texts.count("0") == 1 and "X [m]" in texts and "Y [m]" in texts and "Time [s]" in texts and texts[-2:] == ["Kinovea", "Velocity Tracker"]
    assert "0.10" in texts and "0.20" in texts


def _pandas_window_means(table, windows, device=0):
    """what vbt_window_means computes (tests/test_gpu_validate.py holds the two equal to the bit), without a GPU"""
    import pandas as pd
    out = np.array(table, np.float64)
    for c, w in enumerate(windows):
        if w >= 0:
            s = pd.Series(out[:, c])
            out[:, c] = (s.expanding(min_periods=1) if w == 0 else s.rolling(window=w, center=False, min_periods=1)).mean().to_numpy()
    return out


def test_numpy_statement_against_metric_trajectory_and_compare(monkeypatch):
    """the five cases at the tolerances of tests/test_gpu_validate.py for exactly this comparison; the window means, the one step of
    validate.metric_trajectory that runs on the device, are pandas' here"""
    from vbt_amd import validate as V
    monkeypatch.setattr(V, "window_means", _pandas_window_means)
    for name, kind, (ref, rows) in zip(VC.NAMES, VC.KINDS, VC.pairs()):
        traj, grid, stats = VR.numbers(ref, rows, kind, VC.PLATE, VC.RATE)
        want = V.metric_trajectory(rows, ref, VC.PLATE, kind)
        np.testing.assert_allclose(traj, want, rtol=1e-13, atol=1e-15, err_msg=name)
        with np.errstate(all="ignore"):
            r = V.compare(ref, want)
        assert r["n"] == stats[4] == len(grid), name
        np.testing.assert_allclose(stats[:4], [r["mse_x"], r["mse_y"], r["r_x"], r["r_y"]], rtol=1e-10, err_msg=name)
        assert (stats[7] != 0) == (name == "e") and (name != "e" or (np.isnan(stats[2]) and stats[0] == 0.0 and stats[7] == 1))


def test_the_cases_hold_what_they_are_meant_to():
    prs = dict(zip(VC.NAMES, VC.pairs()))
    assert [len(prs[k][1]) for k in VC.NAMES] == [40, 12, 2, 330, 20] and [len(prs[k][0]) for k in VC.NAMES] == [55, 300, 2, 700, 25]
    for cfg in VC.CONFIGS:
        p = VC.params(cfg)
        ref = dict(zip(VC.NAMES, VC.reference(cfg)))
        a, b, c, d, e = (ref[k][0] for k in VC.NAMES)
        assert a["stats"][5] == prs["a"][0][0, 0] > prs["a"][1][0, 0] and a["stats"][6] == prs["a"][0][-1, 0] < prs["a"][1][-1, 0]
        assert a["head"][3] - a["head"][2] > a["head"][5] - a["head"][4]                # X widened by dY: now the wider one
        assert b["head"][5] - b["head"][4] > b["head"][3] - b["head"][2] and len(prs["b"][1]) < 30
        assert c["stats"][4] == 3 and list(c["counts"]) == [2, 2, 2, 2]
        assert d["stats"][4] > 256 and d["stats"][4] % 256 != 0 and d["counts"][0] < 700 and d["counts"][2] < 700
        assert e["stats"][0] == 0.0 and np.isnan(e["stats"][2]) and e["stats"][7] == 1
        st = {k: VR.staged(q["counts"], q["pts"], q["recs"], **p) for k, (q, _) in ref.items()}
        assert st["d"] == (False, True) and all(v == (True, True) for k, v in st.items() if k != "d"), st
        for k, (q, frame) in ref.items():                                              # merged and unmerged polylines cover the same pixels
            assert np.array_equal(VR.render_one(q, merged=True, **p), frame), (cfg, k)


# ---- the shared core as a host program ----

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("validation_check") / "validation_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "fuzz", "validation_check.cc"), "-o", exe])
    return exe


def write_case(path, cfg, kind, ref, rows):
    with open(path, "wb") as f:
        f.write(np.array(list(cfg) + [VR.KINDS[kind], len(ref), len(rows), 0], np.int32).tobytes())
        f.write(np.array([VC.PLATE, VC.RATE], np.float64).tobytes())
        f.write(np.ascontiguousarray(ref, np.float64).tobytes() + np.ascontiguousarray(rows, np.float64).tobytes())


def write_want(path, q, frame, seed):
    H, W = frame.shape[:2]
    rng = np.random.default_rng(seed)
    xs, ys = rng.integers(0, W, 6000), rng.integers(0, H, 6000)
    px = frame[ys, xs].astype(np.int32)
    pix = np.stack([xs, ys, px[:, 0] | px[:, 1] << 8 | px[:, 2] << 16], axis=1).astype(np.int32)
    with open(path, "wb") as f:
        for a in (q["stats"], q["head"], q["traj"]):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
        f.write(np.array([len(q["grid"]), 0], np.int32).tobytes() + np.ascontiguousarray(q["grid"], np.float64).tobytes())
        f.write(q["counts"].astype(np.int32).tobytes() + np.array([len(q["pts"]), len(q["recs"])], np.int32).tobytes())
        f.write(q["pts"].astype(np.int32).tobytes() + q["recs"].astype(np.int32).tobytes())
        f.write(np.array([len(pix), 0], np.int32).tobytes() + pix.tobytes())


def run(harness, case, want, expect=0):
    p = subprocess.run([harness, case, want], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert p.returncode == expect and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, (p.stdout[-1000:], p.stderr[-3000:])
    return p.stdout


@pytest.mark.parametrize("cfg", VC.CONFIGS, ids=IDS)
def test_host_program_equals_the_numpy_statement(harness, tmp_path, cfg):
    """every double with ==, every integer exactly, 6000 seeded pixels per pair (the program renders the MERGED tables, numpy the
    unmerged polylines)"""
    for i, (name, kind, (ref, rows), (q, frame)) in enumerate(zip(VC.NAMES, VC.KINDS, VC.pairs(), VC.reference(cfg))):
        case, want = str(tmp_path / f"{name}.case"), str(tmp_path / f"{name}.want")
        write_case(case, cfg, kind, ref, rows)
        write_want(want, q, frame, 100 + i)
        assert run(harness, case, want).startswith("ok:"), name


def test_host_program_tells_a_difference_and_a_refused_pair(harness, tmp_path):
    cfg = VC.CONFIGS[0]
    (ref, rows), (q, frame) = VC.pairs()[0], VC.reference(cfg)[0]
    case, want = str(tmp_path / "a.case"), str(tmp_path / "a.want")
    write_case(case, cfg, "kinovea", ref, rows)
    off = dict(q, stats=np.nextafter(q["stats"], 1.0))                                  # one unit in the last place
    write_want(want, off, frame, 1)
    assert "stats[0]" in run(harness, case, want, expect=1)
    bad = rows.copy()
    bad[4, 0] = bad[3, 0]
    write_case(case, cfg, "kinovea", ref, bad)
    assert "series 1, row 4" in run(harness, case, want, expect=3)


# ---- the CLI ----

def test_validate_help_lists_the_figure_options_and_a_bad_format_is_refused_before_any_work(tmp_path):
    from vbt_amd.cli import main
    res = CliRunner().invoke(main, ["validate", "--help"])
    assert res.exit_code == 0
    for word in ("--fig_dir", "--fig_format", "--fig_quality", "jpg|ppm", "no display", "p-values", "LaTeX"):
        assert word in res.output, word
    assert "--show_fig " not in res.output.replace("no --show_fig", "")
    missing = str(tmp_path / "nowhere")
    res = CliRunner().invoke(main, ["validate", "--kinovea_dir", missing, "--df_dir", missing, "--fig_dir", str(tmp_path / "figs"), "--fig_format", "png"])
    assert res.exit_code == 2 and "--fig_format" in res.output and not (tmp_path / "figs").exists()
    res = CliRunner().invoke(main, ["validate", "--kinovea_dir", missing, "--df_dir", missing, "--fig_dir", str(tmp_path / "figs"), "--fig_quality", "0"])
    assert res.exit_code == 2 and "--fig_quality" in res.output and not (tmp_path / "figs").exists()
    # no exports: the totals line alone, no figure, no device needed
    res = CliRunner().invoke(main, ["validate", "--kinovea_dir", missing, "--df_dir", missing, "--fig_dir", str(tmp_path / "figs")])
    assert res.exit_code == 0 and res.output == "Total MSEx = 0, MSEy = 0\n"
