"""Rep figure on the GPU (include/vbt_hip.h, "Rep figure") against the numpy statement (tests/figure_ref.py): the tables the prepare
kernel forms, compared before any pixel, then every byte of the rendered frames - frames pre-filled with seeded noise between two
noise guards, so that a byte left unwritten or written outside cannot pass.  The figures are tests/figure_cases.py's: (a) 40 rows and
phases that start before t0, share a boundary column, hold, and end after t1; (b) T = 1; (c) T = 0; (d) 700 rows on about 116 columns,
whose tiles hold more than VBT_FIGURE_STAGE_POINTS points and so read global memory, while (a)-(c) render from LDS."""
import ctypes
import os

import numpy as np
import pytest
from click.testing import CliRunner

import figure_cases as FC
import figure_ref as FR
import mjpeg_ref as MR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
ARG, CAPACITY, STATE = -1, -4, -5
IDS = ["%dx%d-s%d-t%d" % c for c in FC.CONFIGS]
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
    """the four figures at one configuration, set once: (Figure, tables, guarded render)"""
    if cfg not in _cache:
        from vbt_amd.figure import Figure
        fig = Figure(max_figures=4, max_rows=700, max_phases=5, **FC.params(cfg))
        fig.set(list(FC.figures()))
        tables = [fig.table(i) for i in range(4)]
        _cache[cfg] = (fig, tables, render_guarded(fig, 0, 4, 11))
    return _cache[cfg]


@pytest.mark.parametrize("cfg", FC.CONFIGS, ids=IDS)
def test_tables_equal_the_numpy_prepare(cfg):
    _, tables, _ = gpu(cfg)
    for i, ((hd, pts, recs), (whd, wpts, wrecs, _)) in enumerate(zip(tables, FC.reference(cfg))):
        assert np.array_equal(hd, whd), (i, hd, whd)                                # doubles with ==
        assert np.array_equal(pts, wpts), (i, np.argwhere(pts != wpts)[:5])
        assert recs.shape == wrecs.shape and np.array_equal(recs, wrecs), (i, recs.shape, wrecs.shape)


@pytest.mark.parametrize("cfg", FC.CONFIGS, ids=IDS)
def test_every_byte_equals_the_numpy_render_and_none_outside(cfg):
    fig, tables, (before, frames, after, init) = gpu(cfg)
    assert (fig.W % 4 == 0) == (cfg[0] % 4 == 0)                                     # 160 / 320 wide: 32-bit stores; 161 wide: bytes
    for i, (_, _, _, want) in enumerate(FC.reference(cfg)):
        assert np.array_equal(frames[i], want), (i, np.argwhere((frames[i] != want).any(axis=2))[:10])
    assert np.array_equal(before, init[0]) and np.array_equal(after, init[-1])
    # which path ran: (d)'s tiles read their points from global memory, the others stage them; every tile stages its records
    st = [FR.staged(t[1], t[2], **FC.params(cfg)) for t in tables]
    assert [s[0] for s in st] == [True, True, True, False] and all(s[1] for s in st)


def test_a_crowded_tile_reads_its_records_from_global_memory():
    """more than VBT_FIGURE_STAGE_RECORDS records in one tile: 60 concentric phases put 120 spans and 120 labels on a 160 x 100 figure"""
    from vbt_amd.figure import Figure
    cfg = FC.CONFIGS[1]
    rows, _ = FC.figure_a()
    ph = np.array([[0.5 + 0.1 * i, 0.6 + 0.1 * i, 0.6, 0.4, 0.3 + 0.01 * i, 0.0] for i in range(60)], np.float64)
    fig = Figure(max_figures=1, max_rows=40, max_phases=60, **FC.params(cfg))
    fig.set([(rows, ph)])
    hd, pts, recs = fig.table(0)
    whd, wpts, wrecs = FR.prepare(rows, ph, **FC.params(cfg))
    assert np.array_equal(hd, whd) and np.array_equal(pts, wpts) and np.array_equal(recs, wrecs)
    assert FR.staged(wpts, wrecs, **FC.params(cfg)) == (True, False)
    before, frames, after, init = render_guarded(fig, 0, 1, 17)
    assert np.array_equal(frames[0], FR.render_one(whd, wpts, wrecs, **FC.params(cfg)))
    assert np.array_equal(before, init[0]) and np.array_equal(after, init[-1])


@pytest.mark.parametrize("cfg", [FC.CONFIGS[1], FC.CONFIGS[2]], ids=[IDS[1], IDS[2]])
def test_rendering_twice_equals_once_and_a_range_writes_only_its_frames(cfg):
    fig, _, (_, frames, _, _) = gpu(cfg)
    before, twice, after, init = render_guarded(fig, 0, 4, 23, times=2)
    assert np.array_equal(twice, frames) and np.array_equal(before, init[0]) and np.array_equal(after, init[-1])
    before, part, after, init = render_guarded(fig, 1, 2, 29)                      # exactly frames 1..2 of the full render
    assert np.array_equal(part, frames[1:3]) and np.array_equal(before, init[0]) and np.array_equal(after, init[-1])


def test_a_frame_pointer_off_alignment_takes_the_byte_stores_and_writes_the_same_bytes():
    """160 wide (W % 4 == 0) at a device pointer that is not 4-aligned: the byte path of the store where the width alone takes words"""
    from vbt_amd.mem import DeviceBuffer
    fig, _, (_, frames, _, _) = gpu(FC.CONFIGS[0])
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
    from vbt_amd.figure import Figure
    from vbt_amd.mem import DeviceBuffer
    cfg = FC.CONFIGS[1]
    L = _lib.lib()
    (ra, pa), (rb, pb) = FC.figure_a(), FC.figure_b()
    fig = Figure(max_figures=2, max_rows=40, max_phases=5, **FC.params(cfg))
    buf = DeviceBuffer(3 * fig.frame_bytes)
    assert L.vbt_figure_render(fig._h, buf.ptr, 0, 1, None) == STATE                # render before set
    head = np.zeros(6)
    n = ctypes.c_int()
    assert L.vbt_figure_table(fig._h, 0, head.ctypes.data, None, 0, ctypes.byref(n), None, 0, ctypes.byref(n)) == STATE

    def refused(figs, code, word):
        with pytest.raises(_lib.VbtError) as e:
            fig.set(figs)
        assert f"error {code}:" in str(e.value) and word in str(e.value), str(e.value)
    refused([(np.concatenate([ra, ra[-1:]]), pa)], CAPACITY, "41 rows")
    refused([(ra, np.concatenate([pa, pa[-1:]]))], CAPACITY, "6 phases")
    refused([(ra, pa), (rb, pb), (rb, pb)], CAPACITY, "3 figures")
    fig.set([(ra, pa), (rb, pb)])
    refused([(ra, pa)] * 3, CAPACITY, "3 figures")                                 # a refused call leaves the handle as it was
    for fig0, cnt in ((0, 3), (2, 1), (-1, 1), (1, 2), (0, -1)):
        assert L.vbt_figure_render(fig._h, buf.ptr, fig0, cnt, None) == ARG, (fig0, cnt)
    assert L.vbt_figure_table(fig._h, 2, head.ctypes.data, None, 0, ctypes.byref(n), None, 0, ctypes.byref(n)) == ARG
    ref = FC.reference(cfg)
    got = fig.frames()
    assert np.array_equal(got[0], ref[0][3]) and np.array_equal(got[1], ref[1][3])
    fig.set([(rb, pb)])                                                            # a second set replaces the first
    assert fig.n == 1 and np.array_equal(fig.frames()[0], ref[1][3])


def test_encode_follows_render_on_the_same_stream():
    from vbt_amd.mjpeg import Encoder
    cfg = FC.CONFIGS[1]
    fig, _, _ = gpu(cfg)
    enc = Encoder(fig.H, fig.W, "rgb24", 90, 4)
    enc.encode(fig.device_frames(), 4)                                             # no synchronisation between the two
    for i, (jpeg, (_, _, _, want)) in enumerate(zip(enc.read(), FC.reference(cfg))):
        assert jpeg == MR.encode(want, 90), i


COLS = ["time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width"]


def _golden_rows():
    full = np.load(os.path.join(GOLDEN, "dfs_ocsort_full.npz"))
    m = full["c001_id"] == 1
    return np.stack([full[f"c001_{c}"][m] for c in COLS], axis=1).astype(np.float64)


def test_a_real_clip_shows_a_label_per_concentric_rep():
    from vbt_amd.figure import Figure
    from vbt_amd.velocity import Phase, analyze_rows
    rows = _golden_rows()
    phases = analyze_rows(rows, 0.45, preprocess=True)
    reps = [p for p in phases if p.type == Phase.CONCENTRIC]
    assert len(reps) == 6
    fig = Figure(max_figures=1, max_rows=len(rows), max_phases=len(phases), width=320, height=200, scale=1, thickness=2)
    fig.set([(rows, phases)])
    hd, pts, recs = fig.table(0)
    labels = recs[(recs[:, 0] == FR.TEXT) & (recs[:, 11] >> 8 == 1)]
    assert len(labels) == 2 * len(reps)                                            # one in each rectangle
    assert labels[0::2, 10].tolist() == [FR.HR.centi(p.rom) for p in reps]
    assert labels[1::2, 10].tolist() == [FR.HR.centi(p.rom / p.duration) for p in reps]
    assert (hd[0], hd[1]) == (rows[0, 0], rows[-1, 0]) and len(pts) == len(rows)


def test_cli_plot_writes_the_figures_and_prints_what_analyze_prints(tmp_path):
    import pandas as pd
    from vbt_amd.cli import main
    from vbt_amd.figure import Figure, load
    from vbt_amd.mjpeg import probe
    gold = _golden_rows()[:400]
    paths = []
    for name, tid, rows in (("clipA_id1_m.pkl.gz", 1, gold), ("clipB_id7_lite0.pkl.gz", 7, FC.figure_d()[0])):
        other = rows[::3].copy()                                                   # another id's rows in the same file: not plotted
        other[:, 2] += 0.05
        df = pd.DataFrame({"id": [tid] * len(rows) + [tid + 1] * len(other), **{c: np.concatenate([rows[:, k], other[:, k]]) for k, c in enumerate(COLS)}})
        paths.append(str(tmp_path / name))
        df.to_pickle(paths[-1])
    bad = str(tmp_path / "wrongname.pkl.gz")
    pd.DataFrame({"id": [1]}).to_pickle(bad)
    out = str(tmp_path / "figs")
    args = [paths[0], bad, paths[1], "--fig_dir", out, "--fig_size", "160x100", "--fig_scale", "1"]
    res = CliRunner().invoke(main, ["plot"] + args + ["--fig_format", "ppm"])
    assert res.exit_code == 0, (res.output, res.exception)
    assert f"Couldn't create a plot for file '{bad}'." in res.output
    assert sorted(os.listdir(out)) == ["clipA_id1_m.ppm", "clipB_id7_lite0.ppm"]
    ana = CliRunner().invoke(main, ["analyze", paths[0], bad, paths[1]])
    assert ana.exit_code == 0 and res.output == ana.output and "rep 1:" in ana.output
    loaded = [load(p, 0.45) for p in paths]
    fig = Figure(max_figures=2, max_rows=700, max_phases=512, width=160, height=100, scale=1)
    fig.set(loaded)
    want = fig.frames()
    for i, name in enumerate(("clipA_id1_m.ppm", "clipB_id7_lite0.ppm")):
        data = open(os.path.join(out, name), "rb").read()
        hdr = b"P6\n160 100\n255\n"
        assert data.startswith(hdr) and data[len(hdr):] == want[i].tobytes(), name
    assert len(loaded[0][0]) == 400 and np.array_equal(loaded[1][0], FC.figure_d()[0])
    res = CliRunner().invoke(main, ["plot"] + args + ["--fig_quality", "80"])
    assert res.exit_code == 0, (res.output, res.exception)
    for name in ("clipA_id1_m.jpg", "clipB_id7_lite0.jpg"):
        assert probe(open(os.path.join(out, name), "rb").read())[:2] == (100, 160), name
