"""Tracking overlay without a GPU: the six entry points of the C ABI, the argument refusals made before any device call, the numpy
statement of the raster contract (tests/overlay_ref.py) against cases worked out by hand, the frame-number round trip and the CLI option."""
import ctypes

import numpy as np
import pytest
from click.testing import CliRunner

import overlay_ref as R

ENTRY_POINTS = ("vbt_overlay_default_params", "vbt_overlay_create", "vbt_overlay_set_rows", "vbt_overlay_draw", "vbt_overlay_geometry",
                "vbt_overlay_destroy")
ROW = np.dtype([("id", "<i8"), ("time", "<f8"), ("x", "<f8"), ("y", "<f8"), ("dx", "<f8"), ("dy", "<f8"), ("h", "<f8"), ("w", "<f8")])


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib
    return _lib, _lib.lib()


def _grid(H, W):
    py, px = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    return px, py


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
    assert ctypes.sizeof(_lib_mod.OverlayParams) == 24
    p = _lib_mod.OverlayParams()
    L.vbt_overlay_default_params(ctypes.byref(p))
    assert (p.trail, p.thickness, p.radius, p.label_scale, list(p.rgb), p.label, p.box) == (120, 2, 10, 3, [255, 255, 255], 1, 1)


def test_create_refuses_bad_arguments_before_any_device_call():
    _lib_mod, L = _lib()

    def create(H, W, fmt, **kw):
        p = _lib_mod.OverlayParams()
        L.vbt_overlay_default_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        h = ctypes.c_void_p()
        rc = L.vbt_overlay_create(0, H, W, fmt, ctypes.byref(p), ctypes.byref(h))
        assert rc != 0 and not h.value
        return rc, L.vbt_last_error().decode()
    for args, kw, word in (((71, 104, 1), {}, "even"), ((72, 103, 2), {}, "even"), ((16385, 64, 0), {}, "16384"), ((64, 16386, 1), {}, "16384"),
                           ((72, 104, 0), {"trail": 0}, "trail"), ((72, 104, 0), {"label_scale": 0}, "label_scale"), ((72, 104, 3), {}, "unknown"),
                           ((0, 104, 0), {}, "16384")):
        rc, msg = create(*args, **kw)
        assert rc == -1 and word in msg, (args, kw, rc, msg)
    with pytest.raises(_lib_mod.VbtArgError):
        _lib_mod.check(create(71, 104, 1)[0])


def test_set_rows_refuses_bad_rows_before_any_device_call():
    _lib_mod, L = _lib()

    def rows(n=4):
        r = np.zeros(n, ROW)
        r["id"], r["time"] = 1, (np.arange(n) + 1) / 30.0
        r["x"], r["y"], r["h"], r["w"] = 0.5, 0.5, 0.3, 0.2
        return r

    def set_rows(r, fps=30.0):
        rc = L.vbt_overlay_set_rows(None, r.ctypes.data, len(r), fps, None)
        return rc, L.vbt_last_error().decode()
    good = rows()
    rc, msg = set_rows(good)
    assert rc == -1 and "handle" in msg                     # good rows get as far as the (missing) handle
    for field, value, word in (("x", np.nan, "non-finite"), ("time", np.inf, "non-finite"), ("dy", -np.inf, "non-finite"),
                               ("w", -1e-9, "negative"), ("h", -0.5, "negative"), ("id", -1, "negative id")):
        r = rows()
        r[field][2] = value
        rc, msg = set_rows(r)
        assert rc == -1 and word in msg and "handle" not in msg, (field, msg)
    for fps in (0.0, -30.0, float("nan"), float("inf")):
        rc, msg = set_rows(good, fps)
        assert rc == -1 and "fps" in msg, (fps, msg)
    r = rows()
    r["time"][[1, 2]] = r["time"][[2, 1]]
    rc, msg = set_rows(r)
    assert rc == -1 and "sorted" in msg
    r = rows()
    r["id"][0] = 2
    rc, msg = set_rows(r)
    assert rc == -1 and "sorted" in msg
    assert L.vbt_overlay_draw(None, None, 1, 1, 1, None) == -1
    assert L.vbt_overlay_geometry(None, None, 0, None) == -1


def test_reference_segment_by_hand():
    px, py = _grid(8, 9)
    m = R.segment_mask(px, py, (2, 2), (5, 2), 2)
    want = np.zeros((8, 9), bool)
    want[1:4, 2:6] = True
    want[2, 1] = want[2, 6] = True
    assert np.array_equal(m, want)
    assert np.array_equal(R.segment_mask(px, py, (5, 2), (2, 2), 2), want)                # direction does not matter
    wantv = np.zeros((8, 9), bool)                                                        # the same run, vertical
    wantv[2:6, 1:4] = True
    wantv[1, 2] = wantv[6, 2] = True
    assert np.array_equal(R.segment_mask(px, py, (2, 2), (2, 5), 2), wantv)
    dot = R.segment_mask(px, py, (4, 4), (4, 4), 2)                                       # L2 = 0: the end-point test alone
    assert dot.sum() == 5 and dot[4, 4] and dot[3, 4] and dot[4, 3] and dot[5, 4] and dot[4, 5]
    # far end points are clamped to +-32768 before the products: nothing overflows and the pixels next to the line are covered
    far = R.segment_mask(px, py, (-(1 << 20), 3), (1 << 20, 3), 2)
    assert np.array_equal(far, np.tile(((py[:, 0] >= 2) & (py[:, 0] <= 4))[:, None], (1, 9)))


def test_reference_box_marker_label_by_hand():
    px, py = _grid(40, 40)
    m = R.box_mask(px, py, 10, 10, 20, 20, 2)
    cols = np.nonzero(m[15])[0].tolist()
    assert cols == [9, 10, 20, 21] and np.nonzero(m[:, 15])[0].tolist() == [9, 10, 20, 21]
    assert m[9, 9:22].all() and m[21, 9:22].all() and not m[8].any() and not m[11:20, 11:20].any()
    assert np.nonzero(R.box_mask(px, py, 10, 10, 20, 20, 1)[15])[0].tolist() == [10, 20]          # a = 0, b = 1
    assert np.nonzero(R.box_mask(px, py, 10, 10, 20, 20, 3)[15])[0].tolist() == [9, 10, 11, 19, 20, 21]
    assert R.box_mask(px, py, 10, 10, 11, 20, 2)[15, 9:13].all()                                   # empty inner rectangle: filled
    assert R.marker_mask(px, py, 20, 20, 10).sum() == 317
    lab = R.label_mask(px, py, 7, 3, 20, 1)                      # ymin = 20: yb = 35, rows 29..35; characters at columns 3, 9, 15
    want = np.zeros((40, 40), bool)
    for k, ch in enumerate("id7"):
        want[29:36, 3 + 6 * k:8 + 6 * k] = R.glyph(ch)
    assert np.array_equal(lab, want)
    assert R.glyph("7")[0].all() and R.glyph("7")[1].tolist() == [False, False, False, False, True]
    big = R.label_mask(*_grid(80, 80), 7, 3, 40, 3)
    assert big.sum() == 9 * want.sum()


def test_reference_label_baseline_switch():
    px, py = _grid(72, 40)
    for ymin, yb in ((30, 45), (31, 16)):                         # ymin - 15 > 15 first holds at ymin = 31
        rows = np.nonzero(R.label_mask(px, py, 1, 2, ymin, 1).any(axis=1))[0]
        assert rows.min() == yb - 6 and rows.max() == yb, (ymin, rows)


def test_reference_yuv_colour_and_chroma_rule():
    assert R.yuv_colour((255, 255, 255)) == (235, 128, 128) and R.yuv_colour((0, 0, 0)) == (16, 128, 128)
    assert R.yuv_colour((252, 3, 115)) == (((66 * 252 + 129 * 3 + 25 * 115 + 128) >> 8) + 16, ((-38 * 252 - 74 * 3 + 112 * 115 + 128) >> 8) + 128,
                                           ((112 * 252 - 94 * 3 - 18 * 115 + 128) >> 8) + 128)
    H, W = 4, 6
    mask = np.zeros((H, W), bool)
    mask[1, 3] = True                                             # one pixel: its luma, and the chroma sample (0, 1)
    Y, U, V = R.yuv_colour((252, 3, 115))
    for fmt in ("nv12", "i420"):
        f = np.full((H * 3 // 2, W), 7, np.uint8)
        out = R.paint(f, mask, fmt, (252, 3, 115)).reshape(-1)
        want = np.full(H * W * 3 // 2, 7, np.uint8)
        want[1 * W + 3] = Y
        if fmt == "nv12":
            want[H * W + 0 * W + 2], want[H * W + 0 * W + 3] = U, V
        else:
            want[H * W + 1], want[H * W + (H // 2) * (W // 2) + 1] = U, V
        assert np.array_equal(out, want), fmt


@pytest.mark.parametrize("fps", [30.0, 29.97, 59.94, 23.976])
def test_frame_number_round_trip(fps):
    n = np.arange(1, 200001, dtype=np.float64)
    rows = {"time": n / np.float64(fps), "id": np.ones(len(n), np.int64)}
    for k in ("x", "y", "norm_plate_width", "norm_plate_height"):
        rows[k] = np.zeros(len(n))
    assert np.array_equal(np.rint(rows["time"] * np.float64(fps)), n)
    assert np.array_equal(R.geometry({k: v[:2000] for k, v in rows.items()}, fps, 8, 8, trail=1)[:, 0], n[:2000].astype(np.int64))


def test_reference_geometry_truncates_and_caps_the_trail():
    rows = R.sorted_rows({"id": [2, 1, 1, 1], "time": [0.1, 0.3, 0.1, 0.2], "x": [0.5, 0.03, 1.02, 0.0], "y": [0.5, 0.97, 0.5, 0.0],
                          "dx": [0] * 4, "dy": [0] * 4, "norm_plate_height": [0.3] * 4, "norm_plate_width": [0.22] * 4})
    assert rows["id"].tolist() == [1, 1, 1, 2] and rows["time"].tolist() == [0.1, 0.2, 0.3, 0.1]
    g = R.geometry(rows, 10.0, 72, 104, trail=2)
    assert g[:, 0].tolist() == [1, 2, 3, 1] and g[:, 7].tolist() == [1, 2, 2, 1]
    assert g[0, 1:3].tolist() == [106, 36] and g[1].tolist()[1:7] == [0, 0, -11, -10, 11, 10]       # trunc goes toward zero
    assert g[2, 3] == int((0.03 - 0.11) * 104) == -8


def test_track_help_lists_video_dir():
    from vbt_amd.cli import main
    res = CliRunner().invoke(main, ["track", "--help"])
    assert res.exit_code == 0 and "--video_dir" in res.output
    res = CliRunner().invoke(main, ["overlay", "--help"])
    assert res.exit_code == 0 and "--video_dir" in res.output and "--frame_stride" in res.output
