"""Validation figure on the GPU (include/vbt_hip.h, "Validation figure") against the numpy statement (tests/validation_ref.py): the
numbers and the tables the prepare kernel forms - doubles with ==, integers exactly - compared before any pixel, then every byte of
the rendered frames against numpy's render of the UNMERGED polylines - frames pre-filled with seeded noise between two noise guards,
so that a byte left unwritten or written outside cannot pass.  The pairs are tests/validation_cases.py's (a) .. (e); (d) reads
global memory at every configuration, and `staged` asserts it here.  Then the 37 golden pairs against tests/golden/validation.npz, and
`cli validate --fig_dir`."""
import io
import os
import struct

import numpy as np
import pytest
from click.testing import CliRunner

import mjpeg_ref as MR
import validation_cases as VC
import validation_ref as VR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
ARG, CAPACITY, STATE = -1, -4, -5
IDS = ["%dx%d-s%d-t%d" % c for c in VC.CONFIGS]
PSNR_MARGIN_DB = 0.25        # as tests/test_gpu_mjpeg.py and tests/test_gpu_curve_figure.py
_cache = {}


def noise(n_frames, frame_bytes, seed):
    return np.random.default_rng(seed).integers(0, 256, (n_frames, frame_bytes), dtype=np.uint8)


def render_guarded(fig, pair0, n, seed, times=1):
    """frames pair0 .. pair0 + n - 1 rendered `times` times into noise between two noise guards: (guard before, frames, guard after, noise)"""
    from vbt_amd.mem import DeviceBuffer
    init = noise(n + 2, fig.frame_bytes, seed)
    buf = DeviceBuffer.from_host(init)
    for _ in range(times):
        fig.render(buf.ptr + fig.frame_bytes, pair0, n)
    got = buf.to_host((n + 2, fig.frame_bytes), np.uint8)
    return got[0], got[1:-1].reshape(n, fig.H, fig.W, 3), got[-1], init


def gpu(cfg):
    """the five pairs at one configuration, set in one call: (Validation, stats, tables, guarded render)"""
    if cfg not in _cache:
        from vbt_amd.validate import Validation
        v = Validation(**VC.MAX, **VC.params(cfg))
        v.set(VC.pairs(), VC.KINDS, VC.PLATE, VC.RATE)
        stats = v.stats()
        tables = [v.table(i) for i in range(len(VC.NAMES))]
        _cache[cfg] = (v, stats, tables, render_guarded(v, 0, len(VC.NAMES), 11))
    return _cache[cfg]


def same(a, b):
    """doubles with ==, two NaNs equal"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("cfg", VC.CONFIGS, ids=IDS)
def test_stats_and_tables_equal_the_numpy_statement(cfg):
    _, stats, tables, _ = gpu(cfg)
    for i, (name, (head, traj, grid, counts, pts, recs), (q, _)) in enumerate(zip(VC.NAMES, tables, VC.reference(cfg))):
        print(name, "stats", stats[i], "numpy", q["stats"])
        assert same(stats[i], q["stats"]), (name, stats[i], q["stats"])
        assert same(traj, q["traj"]), (name, np.argwhere(traj != q["traj"])[:5])
        assert same(grid, q["grid"]), (name, np.argwhere(grid != q["grid"])[:5])
        assert same(head, q["head"]), (name, head, q["head"])
        assert np.array_equal(counts, q["counts"]), (name, counts, q["counts"])
        assert pts.shape == q["pts"].shape and np.array_equal(pts, q["pts"]), (name, pts.shape, q["pts"].shape)          # the merged points
        assert recs.shape == q["recs"].shape and np.array_equal(recs, q["recs"]), (name, recs.shape, q["recs"].shape)
    assert [int(s[7]) for s in stats] == [0, 0, 0, 0, 1] and stats[4][0] == 0.0 and np.isnan(stats[4][2])              # (e) alone carries a flag


@pytest.mark.parametrize("cfg", VC.CONFIGS, ids=IDS)
def test_every_byte_equals_the_numpy_render_of_the_unmerged_polylines_and_none_outside(cfg):
    v, _, tables, (before, frames, after, init) = gpu(cfg)
    assert (v.W % 4 == 0) == (cfg[0] % 4 == 0)                                       # 160 / 320 wide: 32-bit stores; 161 wide: bytes
    for name, frame, (_, want) in zip(VC.NAMES, frames, VC.reference(cfg)):
        assert np.array_equal(frame, want), (name, np.argwhere((frame != want).any(axis=2))[:10])
    assert np.array_equal(before, init[0]) and np.array_equal(after, init[-1])
    # which path ran, from the tables the GPU formed: (d) reads its points from global memory, every other pair stages them; every
    # tile stages its records
    st = {name: VR.staged(t[3], t[4], t[5], **VC.params(cfg)) for name, t in zip(VC.NAMES, tables)}
    assert st["d"] == (False, True) and all(s == (True, True) for k, s in st.items() if k != "d"), st


@pytest.mark.parametrize("cfg", [VC.CONFIGS[1], VC.CONFIGS[2]], ids=[IDS[1], IDS[2]])
def test_rendering_twice_equals_once_and_a_range_writes_only_its_frames(cfg):
    v, _, _, (_, frames, _, _) = gpu(cfg)
    n = len(frames)
    before, twice, after, init = render_guarded(v, 0, n, 23, times=2)
    assert np.array_equal(twice, frames) and np.array_equal(before, init[0]) and np.array_equal(after, init[-1])
    before, part, after, init = render_guarded(v, 2, 3, 29)                        # exactly frames 2..4 of the full render
    assert np.array_equal(part, frames[2:5]) and np.array_equal(before, init[0]) and np.array_equal(after, init[-1])


def test_a_frame_pointer_off_alignment_takes_the_byte_stores_and_writes_the_same_bytes():
    """160 wide (W % 4 == 0) at a device pointer that is not 4-aligned: the byte path of the store where the width alone takes words"""
    from vbt_amd.mem import DeviceBuffer
    v, _, _, (_, frames, _, _) = gpu(VC.CONFIGS[0])
    assert v.W == 160
    init = noise(1, v.frame_bytes + 8, 31)[0]
    buf = DeviceBuffer.from_host(init)
    assert buf.ptr % 4 == 0
    v.render(buf.ptr + 1, 3, 1)                                                    # pair (d): the global-memory path
    got = buf.to_host((v.frame_bytes + 8,), np.uint8)
    assert np.array_equal(got[1:1 + v.frame_bytes], frames[3].reshape(-1))
    assert got[0] == init[0] and np.array_equal(got[1 + v.frame_bytes:], init[1 + v.frame_bytes:])


def test_refusals_that_need_a_handle_and_the_handle_renders_afterwards():
    import ctypes
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.validate import Validation
    cfg = VC.CONFIGS[0]
    L = _lib.lib()
    a, b, c, d, e = VC.pairs()
    v = Validation(max_pairs=2, max_rows=40, max_ref_rows=300, max_grid=107, **VC.params(cfg))
    buf = DeviceBuffer(3 * v.frame_bytes)
    assert L.vbt_validation_render(v._h, buf.ptr, 0, 1, None) == STATE             # render, stats and table before set
    out = np.zeros(16)
    assert L.vbt_validation_stats(v._h, out.ctypes.data, 2) == STATE
    n, hd, cn = ctypes.c_int(), np.zeros(6), np.zeros(4, np.int32)

    def table(pair):
        return L.vbt_validation_table(v._h, pair, hd.ctypes.data, None, 0, ctypes.byref(n), None, 0, ctypes.byref(n), cn.ctypes.data, None, 0, ctypes.byref(n),
                                      None, 0, ctypes.byref(n))
    assert table(0) == STATE

    def refused(pairs, kinds, code, word):
        with pytest.raises(_lib.VbtError) as err:
            v.set(pairs, kinds, VC.PLATE, VC.RATE)
        assert f"error {code}:" in str(err.value) and word in str(err.value), str(err.value)
    refused([a, b, c], "kinovea", CAPACITY, "3 pairs")
    refused([d], "kinovea", CAPACITY, "pair 0 has 700 reference rows")
    refused([c, (a[0], d[1])], "kinovea", CAPACITY, "pair 1 has 330 tracked rows")
    refused([(np.array([[0.0, 0.1, 0.2], [5.0, 0.2, 0.3]]), a[1])], "kinovea", CAPACITY, "n = 117")     # the tracked rows end at 3.9 s
    v.set([a, b], ["kinovea", "qualisys"], VC.PLATE, VC.RATE)
    refused([a] * 3, "kinovea", CAPACITY, "3 pairs")                                # a refused call leaves the handle as it was
    for pair0, cnt in ((0, 3), (2, 1), (-1, 1), (1, 2), (0, -1)):
        assert L.vbt_validation_render(v._h, buf.ptr, pair0, cnt, None) == ARG, (pair0, cnt)
    assert table(2) == ARG and table(0) == CAPACITY and L.vbt_validation_stats(v._h, out.ctypes.data, 1) == CAPACITY
    ref = VC.reference(cfg)
    got = v.frames()
    assert np.array_equal(got[0], ref[0][1]) and np.array_equal(got[1], ref[1][1])  # a set after a refused set renders the earlier pairs
    v.set([b], "qualisys", VC.PLATE, VC.RATE)                                      # a second set replaces the first
    assert v.n == 1 and np.array_equal(v.frames()[0], ref[1][1])


def test_encode_follows_render_on_the_same_stream():
    from vbt_amd.mjpeg import Encoder
    cfg = VC.CONFIGS[0]
    v, _, _, _ = gpu(cfg)
    enc = Encoder(v.H, v.W, "rgb24", 90, 2)
    enc.encode(v.device_frames(), 2)                                               # no synchronisation between the two
    for jpeg, (_, want) in zip(enc.read(), VC.reference(cfg)):
        assert jpeg == MR.encode(want, 90)


# ---- the corpus ----

@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "validation.npz"))


def golden_pairs(gold):
    """(key, ref, rows, source) of the 32 Kinovea and 5 Qualisys pairs, the rows as tests/test_gpu_validate.py::test_validation_tables takes them"""
    main = np.load(os.path.join(GOLDEN, "dfs_ocsort_main.npz"))
    out = []
    for k in sorted(k[:-6] for k in gold.files if k.endswith("_stats")):
        if k.startswith("q_"):
            rows, src = gold[k + "_rows"], "qualisys"
        else:
            c = "c" + k[1:]
            rows = np.stack([main[f"{c}_{n}"] for n in ("time", "x", "y", "norm_plate_height", "norm_plate_width")], axis=1)
            src = "kinovea"
        out.append((k, gold[k + "_ref"], rows, src))
    return out


def test_all_37_golden_pairs_in_one_handle(gold):
    """stats only, no render: the aligned trajectory at rtol 1e-13 / atol 1e-15, MSE and r at rtol 1e-10 (tests/test_gpu_validate.py's)"""
    from vbt_amd.validate import Validation, grid_size
    items = golden_pairs(gold)
    assert len(items) == 37 and sum(s == "kinovea" for *_, s in items) == 32
    v = Validation(max_pairs=37, max_rows=max(len(r) for _, _, r, _ in items), max_ref_rows=max(len(r) for _, r, _, _ in items),
                   max_grid=max(grid_size(f, r) for _, f, r, _ in items), **VC.params(VC.CONFIGS[0]))
    v.set([(f, r) for _, f, r, _ in items], [s for *_, s in items], 0.45, 30.0)
    stats = v.stats()
    assert not stats[:, 7].any()
    for i, (k, _, rows, _) in enumerate(items):
        _, traj, _, _, _, _ = v.table(i)
        assert np.array_equal(traj[:, 0], rows[:, 0])
        np.testing.assert_allclose(traj[:, 1:], gold[k + "_xy"], rtol=1e-13, atol=1e-15, err_msg=k)
        np.testing.assert_allclose(stats[i, :4], gold[k + "_stats"][:4], rtol=1e-10, err_msg=k)


# ---- the CLI ----

def _setup(gold, tmp_path):
    """the set-up of tests/test_gpu_validate.py::test_validate_command"""
    import pandas as pd
    import shutil
    rows = gold["q_squat1_rows"]
    df = pd.DataFrame({"id": np.full(len(rows), 23), "time": rows[:, 0], "x": rows[:, 1], "y": rows[:, 2], "dx": 0.0, "dy": 0.0,
                       "norm_plate_height": rows[:, 3], "norm_plate_width": rows[:, 4]})
    dfs = tmp_path / "dfs"
    dfs.mkdir()
    df.to_pickle(str(dfs / "squat1_mobile_side_6reps_id23_efficientdet_lite0_whole.pkl.gz"))
    ex = tmp_path / "exports"
    ex.mkdir()
    shutil.copy(os.path.join(GOLDEN, "qualisys_sample.tsv"), str(ex / "squat1.tsv"))
    (ex / "other.tsv").write_text(open(os.path.join(GOLDEN, "qualisys_sample.tsv")).read())
    return str(ex), str(dfs), rows


def test_cli_validate_fig_dir_writes_the_figure_under_the_reference_s_name(gold, tmp_path):
    from PIL import Image
    from vbt_amd import validate as V
    from vbt_amd.cli import main
    from vbt_amd.figure import ppm
    ex, dfs, rows = _setup(gold, tmp_path)
    base = ["validate", "--qualysis_dir", ex, "--df_dir", dfs]
    plain = CliRunner().invoke(main, base)
    assert plain.exit_code == 0, (plain.output, plain.exception)
    ref = V.read_qualisys(os.path.join(ex, "squat1.tsv"))
    r = V.validate_pair(ref, rows, 0.45, "qualisys")                               # the parent's way to the numbers
    want = (f"No matching df file found for: {os.path.join(ex, 'other.tsv')}\n"
            f"squat1_mobile_side_6reps: MSEx {r['mse_x']:.4f}  MSEy {r['mse_y']:.4f}  r_x {r['r_x']:.4f}  r_y {r['r_y']:.4f}\n"
            f"Total MSEx = {r['mse_x']}, MSEy = {r['mse_y']}\n")
    assert plain.output == want                                                    # without --fig_dir: the parent's output, full doubles and all
    name = "squat1_mobile_side_6reps_id23_efficientdet_lite0_whole"
    jpg = tmp_path / "figs"
    res = CliRunner().invoke(main, base + ["--fig_dir", str(jpg)])
    assert res.exit_code == 0, (res.output, res.exception)
    assert res.output.splitlines()[:2] == plain.output.splitlines()[:2] and res.output.splitlines()[2].startswith("Total MSEx = ")
    assert os.listdir(jpg) == [name + ".jpg"]
    data = (jpg / (name + ".jpg")).read_bytes()
    p = V.default_params()
    sof = [payload for m, payload in MR.segments(data) if m == 0xC0]
    assert data[:2] == b"\xff\xd8" and len(sof) == 1 and struct.unpack(">HH", sof[0][1:5]) == (p["height"], p["width"])
    out = tmp_path / "ppm"
    res = CliRunner().invoke(main, base + ["--fig_dir", str(out), "--fig_format", "ppm"])
    assert res.exit_code == 0 and os.listdir(out) == [name + ".ppm"]
    v = V.Validation(max_pairs=1, max_rows=len(rows), max_ref_rows=len(ref), max_grid=V.grid_size(ref, rows))
    v.set([(ref, rows)], "qualisys", 0.45)
    frame = v.frames()[0]
    assert (out / (name + ".ppm")).read_bytes() == ppm(frame)
    got = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))                  # it decodes, to the handle's size and to the frame
    pil = io.BytesIO()
    Image.fromarray(frame).save(pil, "JPEG", quality=90, subsampling=2)
    bound = MR.psnr(np.asarray(Image.open(io.BytesIO(pil.getvalue()))), frame) - PSNR_MARGIN_DB
    print(f"PSNR {MR.psnr(got, frame):.3f} dB, bound {bound:.3f} dB")
    assert got.shape == frame.shape == (p["height"], p["width"], 3) and MR.psnr(got, frame) >= bound
    total = float(res.output.splitlines()[2].split("=")[1].split(",")[0])
    np.testing.assert_allclose([total, v.stats()[0][0]], [r["mse_x"]] * 2, rtol=1e-10)
