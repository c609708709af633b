"""Curve figure on the GPU (include/vbt_hip.h, "Curve figure") against the numpy statement (tests/curve_figure_ref.py): the tables the
prepare kernel forms - the MERGED points - compared before any pixel, then every byte of the rendered frames against numpy's render of
the UNMERGED polylines - frames pre-filled with seeded noise between two noise guards, so that a byte left unwritten or written
outside cannot pass.  The figures are tests/curve_figure_cases.py's (a) .. (h); its docstring says which of them read global memory at
which configuration, and `staged` asserts it here.  Then evaluate.plot_precision_recall / plot_roc and `cli eval --fig_dir` on curves
computed from tests/golden/eval_detections_ref.npz."""
import ctypes
import io
import os

import numpy as np
import pytest
from click.testing import CliRunner

import curve_figure_cases as CC
import curve_figure_ref as CR
import mjpeg_ref as MR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
ARG, CAPACITY, STATE = -1, -4, -5
IDS = ["%dx%d-s%d-t%d" % c for c in CC.CONFIGS]
PSNR_MARGIN_DB = 0.25        # as tests/test_gpu_mjpeg.py and tests/test_mjpeg_host.py
_cache = {}


def noise(n_frames, frame_bytes, seed):
    return np.random.default_rng(seed).integers(0, 256, (n_frames, frame_bytes), dtype=np.uint8)


def render_guarded(fig, fig0, n, seed, times=1):
    """frames fig0 .. fig0 + n - 1 rendered `times` times into noise between two noise guards: (guard before, frames, guard after, noise)"""
    from vbt_amd.mem import DeviceBuffer
    init = noise(n + 2, fig.frame_bytes, seed)
    buf = DeviceBuffer.from_host(init)
    for _ in range(times):
        fig.render(buf.ptr + fig.frame_bytes, fig0, n)
    got = buf.to_host((n + 2, fig.frame_bytes), np.uint8)
    return got[0], got[1:-1].reshape(n, fig.H, fig.W, 3), got[-1], init


def gpu(cfg):
    """the eight figures at one configuration, set once: (CurveFigure, tables, guarded render)"""
    if cfg not in _cache:
        from vbt_amd.curve_figure import CurveFigure
        fig = CurveFigure(**CC.MAX, **CC.params(cfg))
        fig.set(list(CC.figures()))
        tables = [fig.table(i) for i in range(len(CC.figures()))]
        _cache[cfg] = (fig, tables, render_guarded(fig, 0, len(CC.figures()), 11))
    return _cache[cfg]


@pytest.mark.parametrize("cfg", CC.CONFIGS, ids=IDS)
def test_tables_equal_the_numpy_prepare(cfg):
    _, tables, _ = gpu(cfg)
    for name, (counts, pts, recs), (wcounts, wpts, wrecs, _) in zip(CC.NAMES, tables, CC.reference(cfg)):
        assert np.array_equal(counts, wcounts), (name, counts, wcounts)
        assert pts.shape == wpts.shape and np.array_equal(pts, wpts), (name, np.argwhere(pts != wpts)[:5])       # the merged points
        assert recs.shape == wrecs.shape and np.array_equal(recs, wrecs), (name, recs.shape, wrecs.shape)


@pytest.mark.parametrize("cfg", CC.CONFIGS, ids=IDS)
def test_every_byte_equals_the_numpy_render_of_the_unmerged_polyline_and_none_outside(cfg):
    fig, tables, (before, frames, after, init) = gpu(cfg)
    assert (fig.W % 4 == 0) == (cfg[0] % 4 == 0)                                     # 160 / 320 wide: 32-bit stores; 161 wide: bytes
    for name, frame, (_, _, _, want) in zip(CC.NAMES, frames, CC.reference(cfg)):
        assert np.array_equal(frame, want), (name, np.argwhere((frame != want).any(axis=2))[:10])
    assert np.array_equal(before, init[0]) and np.array_equal(after, init[-1])
    # which path ran, from the tables the GPU formed: (d) reads global memory at 320 (400 merged points), stages at 160 / 161; (g) the
    # other way round; every tile stages its records
    st = dict(zip(CC.NAMES, (CR.staged(*t, **CC.params(cfg)) for t in tables)))
    wide = cfg[0] == 320
    assert st["d"] == (not wide, True) and st["g"] == (wide, True) and all(v == (True, True) for k, v in st.items() if k not in "dg"), st


def test_a_crowded_tile_reads_its_records_from_global_memory():
    """more than VBT_CURVE_FIGURE_STAGE_RECORDS records in one tile: minor grid lines every 20 thousandths on both axes of a 160 x 100 figure"""
    from vbt_amd.curve_figure import CurveFigure
    p = CC.params(CC.CONFIGS[1])
    f = dict(CC.figure_a(), minor_x=20, minor_y=20)
    fig = CurveFigure(max_figures=1, max_series=3, max_points=200, max_marks=0, **p)
    fig.set([f])
    counts, pts, recs = fig.table(0)
    wcounts, wpts, wrecs = CR.prepare(f, **p)
    assert np.array_equal(counts, wcounts) and np.array_equal(pts, wpts) and np.array_equal(recs, wrecs)
    assert CR.staged(wcounts, wpts, wrecs, **p) == (True, False)
    before, frames, after, init = render_guarded(fig, 0, 1, 17)
    assert np.array_equal(frames[0], CR.render_one(f, **p))
    assert np.array_equal(before, init[0]) and np.array_equal(after, init[-1])


@pytest.mark.parametrize("cfg", [CC.CONFIGS[1], CC.CONFIGS[2]], ids=[IDS[1], IDS[2]])
def test_rendering_twice_equals_once_and_a_range_writes_only_its_frames(cfg):
    fig, _, (_, frames, _, _) = gpu(cfg)
    n = len(frames)
    before, twice, after, init = render_guarded(fig, 0, n, 23, times=2)
    assert np.array_equal(twice, frames) and np.array_equal(before, init[0]) and np.array_equal(after, init[-1])
    before, part, after, init = render_guarded(fig, 2, 3, 29)                      # exactly frames 2..4 of the full render
    assert np.array_equal(part, frames[2:5]) and np.array_equal(before, init[0]) and np.array_equal(after, init[-1])


def test_a_frame_pointer_off_alignment_takes_the_byte_stores_and_writes_the_same_bytes():
    """160 wide (W % 4 == 0) at a device pointer that is not 4-aligned: the byte path of the store where the width alone takes words"""
    from vbt_amd.mem import DeviceBuffer
    fig, _, (_, frames, _, _) = gpu(CC.CONFIGS[1])
    assert fig.W == 160 and fig.params["scale"] == 1
    init = noise(1, fig.frame_bytes + 8, 31)[0]
    buf = DeviceBuffer.from_host(init)
    assert buf.ptr % 4 == 0
    fig.render(buf.ptr + 1, 0, 1)
    got = buf.to_host((fig.frame_bytes + 8,), np.uint8)
    assert np.array_equal(got[1:1 + fig.frame_bytes], frames[0].reshape(-1))         # figure (a) as the aligned render wrote it
    assert got[0] == init[0] and np.array_equal(got[1 + fig.frame_bytes:], init[1 + fig.frame_bytes:])


def test_refusals_that_need_a_handle_and_the_handle_renders_afterwards():
    from vbt_amd import _lib
    from vbt_amd.curve_figure import CurveFigure
    from vbt_amd.mem import DeviceBuffer
    cfg = CC.CONFIGS[1]
    L = _lib.lib()
    a, b, e = CC.figure_a(), CC.figure_b(), CC.figure_e()
    fig = CurveFigure(max_figures=2, max_series=3, max_points=120, max_marks=2, **CC.params(cfg))
    buf = DeviceBuffer(3 * fig.frame_bytes)
    assert L.vbt_curve_figure_render(fig._h, buf.ptr, 0, 1, None) == STATE         # render before set
    n = ctypes.c_int()
    assert L.vbt_curve_figure_table(fig._h, 0, None, 0, ctypes.byref(n), None, 0, ctypes.byref(n), None, 0, ctypes.byref(n)) == STATE

    def refused(figs, code, word):
        with pytest.raises(_lib.VbtError) as err:
            fig.set(figs)
        assert f"error {code}:" in str(err.value) and word in str(err.value), str(err.value)
    refused([a, b, b], CAPACITY, "3 figures")
    refused([dict(a, series=a["series"] + a["series"][:1])], CAPACITY, "4 series")
    refused([dict(a, series=[(np.repeat(a["series"][0][0], 4, axis=0), "long", 0)])], CAPACITY, "160 points")
    refused([e], CAPACITY, "5 marks")
    fig.set([a, b])
    refused([a] * 3, CAPACITY, "3 figures")                                        # a refused call leaves the handle as it was
    refused([dict(b, series=[(np.array([[0.1, 0.1], [0.3, 0.2], [0.2, 0.3]]), "zig", 0)])], ARG, "figure 0, series 0, point 2")
    for fig0, cnt in ((0, 3), (2, 1), (-1, 1), (1, 2), (0, -1)):
        assert L.vbt_curve_figure_render(fig._h, buf.ptr, fig0, cnt, None) == ARG, (fig0, cnt)
    assert L.vbt_curve_figure_table(fig._h, 2, None, 0, ctypes.byref(n), None, 0, ctypes.byref(n), None, 0, ctypes.byref(n)) == ARG
    ref = CC.reference(cfg)
    got = fig.frames()
    assert np.array_equal(got[0], ref[0][3]) and np.array_equal(got[1], ref[1][3])  # a set after a refused set renders the earlier figures
    fig.set([b])                                                                   # a second set replaces the first
    assert fig.n == 1 and np.array_equal(fig.frames()[0], ref[1][3])


def test_encode_follows_render_on_the_same_stream():
    from vbt_amd.mjpeg import Encoder
    cfg = CC.CONFIGS[1]
    fig, _, _ = gpu(cfg)
    enc = Encoder(fig.H, fig.W, "rgb24", 90, 2)
    enc.encode(fig.device_frames(), 2)                                             # no synchronisation between the two
    for jpeg, (_, _, _, want) in zip(enc.read(), CC.reference(cfg)):
        assert jpeg == MR.encode(want, 90)


# ---- evaluate.plot_precision_recall / plot_roc and the CLI ----

THRESHOLDS = [0.2, 0.5]
SIZE = dict(width=160, height=100, scale=1)


def _detections_df():
    import pandas as pd
    d = np.load(os.path.join(GOLDEN, "eval_detections_ref.npz"))
    names = [str(n) for n in d["model_names"]]
    return pd.DataFrame({"Score": d["score"], "Model": [names[i] for i in d["model"]], "IoU": d["iou"]})


def _names(models, t, ext):
    return sorted([f"precision_recall_iou_{t}.{ext}", f"roc_iou_{t}.{ext}"] + [f"{k}_{m}_iou_{t}.{ext}" for k in ("precision_recall", "roc") for m in models])


def _ppm(path, width, height):
    data = open(path, "rb").read()
    hdr = b"P6\n%d %d\n255\n" % (width, height)
    assert data.startswith(hdr) and len(data) == len(hdr) + width * height * 3, path
    return np.frombuffer(data, np.uint8, width * height * 3, len(hdr)).reshape(height, width, 3)


@pytest.fixture(scope="module")
def curves():
    from vbt_amd import evaluate
    return evaluate.curves(_detections_df(), 0.5)


def test_plot_functions_write_the_reference_s_files_and_numpy_s_pixels(tmp_path, curves):
    from PIL import Image
    from vbt_amd import evaluate
    from vbt_amd.mjpeg import probe
    models = list(curves)
    assert len(models) == 6
    out = str(tmp_path / "ppm")
    written = evaluate.plot_precision_recall(curves, out, 0.5, THRESHOLDS, fig_format="ppm", **SIZE)
    written += evaluate.plot_roc(curves, out, 0.5, THRESHOLDS, fig_format="ppm", **SIZE)
    assert sorted(os.listdir(out)) == _names(models, 0.5, "ppm") == sorted(os.path.basename(w) for w in written)
    for kind, stem in (("pr", "precision_recall"), ("roc", "roc")):
        combined, singles = evaluate.curve_figures(kind, curves, 0.5, THRESHOLDS)
        assert [c for _, _, c in combined["series"]] == list(range(6)) and combined["corner"] == (0 if kind == "pr" else 1)
        assert (combined["minor_x"], combined["minor_y"]) == ((0, 100) if kind == "pr" else (100, 100))
        want = CR.render_one(CR.figure(**combined), width=160, height=100, scale=1, thickness=2)
        assert np.array_equal(_ppm(os.path.join(out, f"{stem}_iou_0.5.ppm"), 160, 100), want), kind
        for k, (m, one) in enumerate(zip(models, singles)):
            c = curves[m]
            assert [s[2] for s in one["series"]] == [k] and (one["minor_x"], one["minor_y"]) == (50, 50)     # the model keeps its colour
            thr = np.r_[c.pr_thresholds, c.pr_thresholds[-1:]] if kind == "pr" else c.roc_thresholds
            order = THRESHOLDS[::-1] if kind == "pr" else THRESHOLDS
            assert one["marks"] == [(0, evaluate.closest_point(thr, v), f"{thr[evaluate.closest_point(thr, v)]:.4f}") for v in order]
            assert one["series"][0][1] == (f"{m}, AP={c.ap:.4f}" if kind == "pr" else f"{m}, AUC={c.auc:.4f}")
            want = CR.render_one(CR.figure(**one), width=160, height=75, scale=1, thickness=2)
            assert np.array_equal(_ppm(os.path.join(out, f"{stem}_{m}_iou_0.5.ppm"), 160, 75), want), (kind, m)
        assert combined["series"][0][1] == (f"{models[0]}, AP50={curves[models[0]].ap:.4f}" if kind == "pr" else f"{models[0]}, AUC={curves[models[0]].auc:.4f}")
    # jpg: the same frames through vbt_mjpeg_encode
    jpg = str(tmp_path / "jpg")
    evaluate.plot_precision_recall(curves, jpg, 0.5, THRESHOLDS, quality=90, **SIZE)
    evaluate.plot_roc(curves, jpg, 0.5, THRESHOLDS, **SIZE)
    assert sorted(os.listdir(jpg)) == _names(models, 0.5, "jpg")
    for name in os.listdir(jpg):
        h = 100 if name in ("precision_recall_iou_0.5.jpg", "roc_iou_0.5.jpg") else 75
        assert probe(open(os.path.join(jpg, name), "rb").read())[:2] == (h, 160), name
    for name in ("precision_recall_iou_0.5", f"roc_{models[1]}_iou_0.5"):
        data = open(os.path.join(jpg, name + ".jpg"), "rb").read()
        want = _ppm(os.path.join(out, name + ".ppm"), 160, 100 if name.startswith("precision") else 75)
        assert data == MR.encode(want, 90), name                                    # the encoder's own contract (tests/test_gpu_figure.py)
        got = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        pil = io.BytesIO()
        Image.fromarray(want).save(pil, "JPEG", quality=90, subsampling=2)
        bound = MR.psnr(np.asarray(Image.open(io.BytesIO(pil.getvalue()))), want) - PSNR_MARGIN_DB               # (tests/test_gpu_mjpeg.py)
        print(f"{name}: PSNR {MR.psnr(got, want):.3f} dB, bound {bound:.3f} dB")
        assert MR.psnr(got, want) >= bound, (name, MR.psnr(got, want), bound)
    # without thresholds: the two combined figures only (eval.py:278-279,405-406)
    bare = str(tmp_path / "bare")
    evaluate.plot_precision_recall(curves, bare, 0.5, fig_format="ppm", **SIZE)
    evaluate.plot_roc(curves, bare, 0.5, [], fig_format="ppm", **SIZE)
    assert sorted(os.listdir(bare)) == ["precision_recall_iou_0.5.ppm", "roc_iou_0.5.ppm"]
    assert open(os.path.join(bare, "roc_iou_0.5.ppm"), "rb").read() == open(os.path.join(out, "roc_iou_0.5.ppm"), "rb").read()


def test_cli_eval_fig_dir_writes_the_figures_and_prints_the_same_lines(tmp_path, curves):
    from vbt_amd.cli import main
    df_path = str(tmp_path / "det.pkl.gz")
    _detections_df().to_pickle(df_path)
    base = ["eval", "--detections_df", df_path, "--iou_threshold", "0.5", "--score_thresholds", "[0.2, 0.5]"]
    plain = CliRunner().invoke(main, base + ["--curve_dir", str(tmp_path / "csv0")])
    assert plain.exit_code == 0, (plain.output, plain.exception)
    assert plain.output.startswith(f"Loading dataframe '{df_path}'.") and plain.output.count("AUC=") == 6 and plain.output.count("  PR  threshold") == 12
    out = str(tmp_path / "figs")
    res = CliRunner().invoke(main, base + ["--curve_dir", str(tmp_path / "csv1"), "--fig_dir", out, "--fig_size", "160x100", "--fig_scale", "1", "--fig_format", "ppm"])
    assert res.exit_code == 0, (res.output, res.exception)
    assert res.output == plain.output                                              # the same lines
    for name in sorted(os.listdir(tmp_path / "csv0")):                             # and the same CSV files
        assert (tmp_path / "csv0" / name).read_bytes() == (tmp_path / "csv1" / name).read_bytes(), name
    models = list(curves)
    assert sorted(os.listdir(out)) == _names(models, 0.5, "ppm") and len(os.listdir(out)) == 2 + 2 * len(models)
    from vbt_amd import evaluate
    combined, singles = evaluate.curve_figures("roc", curves, 0.5, THRESHOLDS)
    assert np.array_equal(_ppm(os.path.join(out, "roc_iou_0.5.ppm"), 160, 100), CR.render_one(CR.figure(**combined), width=160, height=100, scale=1, thickness=2))
    assert np.array_equal(_ppm(os.path.join(out, f"roc_{models[3]}_iou_0.5.ppm"), 160, 75),
                          CR.render_one(CR.figure(**singles[3]), width=160, height=75, scale=1, thickness=2))
    res = CliRunner().invoke(main, base + ["--fig_dir", str(tmp_path / "jpg"), "--fig_size", "160x100", "--fig_scale", "1", "--fig_quality", "80"])
    assert res.exit_code == 0 and res.output == plain.output and sorted(os.listdir(tmp_path / "jpg")) == _names(models, 0.5, "jpg")
    res = CliRunner().invoke(main, base + ["--fig_dir", str(tmp_path / "small"), "--fig_size", "40x40"])
    assert res.exit_code == 2 and "plot rectangle" in res.output                   # a size the layout refuses is a usage error
