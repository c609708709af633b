"""Tracking overlay on the GPU, bit for bit against the numpy statement of the raster contract (tests/overlay_ref.py), on random
noise frames so that an untouched byte cannot pass by accident."""
import os

import numpy as np
import pytest
from click.testing import CliRunner

import overlay_ref as R

pytestmark = pytest.mark.gpu

H, W, FPS = 72, 104, 30.0
BATCH = (126, 127, 128, 129, 130, 131)          # frame numbers of the batch; 130 has no row
COLOR0 = (252, 3, 115)                          # COLORS[0] of reference track.py:23 as RGB


def synthetic_rows():
    """Id 1: 131 rows (frames 1..129, 131, 132) on a Lissajous path - the trail cap of 120 bites, rows 1..125 only feed trails - with
    two equal consecutive centres (100, 101), an exactly horizontal run (105..108), an exactly vertical run (110..113), boxes over the
    left, top, right and bottom border (126..129), a centre outside the frame (128, x = 1.02) and one at (0, 0) (131).
    Id 12: frames 127 and 129, on top of id 1, its labels on either side of the `ymin - 15 > 15` switch."""
    d = {k: [] for k in R.COLUMNS}

    def add(tid, f, x, y, h=0.3, w=0.22):
        for k, v in zip(R.COLUMNS, (tid, f / FPS, x, y, 0.0, 0.0, h, w)):
            d[k].append(v)
    for f in list(range(1, 130)) + [131, 132]:
        x, y = 0.5 + 0.38 * np.sin(2 * np.pi * f / 37), 0.5 + 0.36 * np.sin(2 * np.pi * f / 23 + 0.7)
        if f == 101:
            x, y = 0.5 + 0.38 * np.sin(2 * np.pi * 100 / 37), 0.5 + 0.36 * np.sin(2 * np.pi * 100 / 23 + 0.7)
        if 105 <= f <= 108:
            y = 0.40
        if 110 <= f <= 113:
            x = 0.62
        x, y = {126: (0.03, y), 127: (x, 0.05), 128: (1.02, y), 129: (x, 0.97), 131: (0.0, 0.0)}.get(f, (x, y))
        add(1, f, x, y)
    add(12, 127, 0.45, 0.6, h=2 * (0.6 - 30.5 / H))             # ymin = 30: label below the box top
    add(12, 129, 0.55, 0.6, h=2 * (0.6 - 31.5 / H))             # ymin = 31: label above it
    return d


def only(data, ids):
    keep = [i for i, v in enumerate(data["id"]) if v in ids]
    return {k: [data[k][i] for i in keep] for k in data}


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def gpu_draw(frames, datas, frame0, frame_step=1, pix_fmt="rgb24", hw=(H, W), times=1, **params):
    """frames through the device: one handle per entry of `datas`, all drawing `times` times on one stream; (frames back, handles)"""
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.overlay import Overlay
    frames = np.ascontiguousarray(frames)
    buf = DeviceBuffer.from_host(frames)
    ovs = []
    for data in datas:
        ov = Overlay(hw[0], hw[1], pix_fmt, **params)
        ov.set_rows(data, FPS)
        ovs.append(ov)
    for _ in range(times):
        for ov in ovs:
            ov.draw(buf.ptr, len(frames), frame0, frame_step)
    _lib.check(_lib.lib().vbt_stream_synchronize(None))
    return buf.to_host(frames.shape, np.uint8), ovs


def assert_same(got, want):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} bytes differ, first at {bad[:5].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


@pytest.fixture(scope="module")
def rows():
    return synthetic_rows()


@pytest.fixture(scope="module")
def rgb_case(rows):
    frames = noise((len(BATCH), H, W, 3), 1)
    want = R.draw(frames, rows, FPS, frame0=BATCH[0])
    want.setflags(write=False)
    return frames, want


def test_scenario_holds_what_it_promises(rows, rgb_case):
    """the synthetic rows really contain the cases the tests are about (checked on the reference's integers)"""
    s = R.sorted_rows(rows)
    g = R.geometry(s, FPS, H, W)
    one = g[s["id"] == 1]
    assert len(one) == 131 and one[-1, 7] == 120 and one[:, 0].tolist() == list(range(1, 130)) + [131, 132]
    by = {int(r[0]): r for r in one}
    assert by[100][1:3].tolist() == by[101][1:3].tolist()
    assert len({by[f][2] for f in range(105, 109)}) == 1 and len({by[f][1] for f in range(105, 109)}) == 4
    assert len({by[f][1] for f in range(110, 114)}) == 1 and len({by[f][2] for f in range(110, 114)}) == 4
    assert by[126][3] < 0 and by[127][4] < 0 and by[128][5] > W and by[129][6] > H and by[128][1] >= W
    assert by[131][1:3].tolist() == [0, 0]
    twelve = g[s["id"] == 12]
    assert twelve[:, 0].tolist() == [127, 129] and twelve[:, 4].tolist() == [30, 31]
    s1, s12 = R.sorted_rows(only(rows, {1})), R.sorted_rows(only(rows, {12}))
    a = R.coverage(s1, R.geometry(s1, FPS, H, W), 127, H, W)
    b = R.coverage(s12, R.geometry(s12, FPS, H, W), 127, H, W)
    assert (a & b).any() and (a & ~b).any() and (b & ~a).any()            # id 12 overlaps id 1
    frames, want = rgb_case
    assert np.array_equal(want[4], frames[4]) and all((want[i] != frames[i]).any() for i in (0, 1, 2, 3, 5))


def test_rgb24_batch_is_bit_exact(rows, rgb_case):
    frames, want = rgb_case
    got, _ = gpu_draw(frames, [rows], BATCH[0])
    assert np.array_equal(got[4], frames[4])                               # the frame without a row comes back identical
    assert_same(got, want)


def test_frame_step_odd_sizes_and_two_handles(rows):
    h, w = 71, 101
    frames = noise((4, h, w, 3), 2)                                        # frames 125, 127, 129, 131
    a, b = only(rows, {1}), only(rows, {12})
    want = R.draw(R.draw(frames, a, FPS, frame0=125, frame_step=2), b, FPS, frame0=125, frame_step=2)
    got, _ = gpu_draw(frames, [a, b], 125, 2, hw=(h, w))
    assert_same(got, want)
    assert_same(want, R.draw(frames, rows, FPS, frame0=125, frame_step=2))  # one colour: two handles draw what one with all rows draws


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_yuv_formats_are_bit_exact(rows, fmt):
    frames = noise((len(BATCH), H * 3 // 2, W), 3)
    want = R.draw(frames, rows, FPS, frame0=BATCH[0], pix_fmt=fmt, rgb=COLOR0)
    got, _ = gpu_draw(frames, [rows], BATCH[0], pix_fmt=fmt, rgb=COLOR0)
    assert np.array_equal(got[4], frames[4])
    assert_same(got, want)
    Y, U, V = R.yuv_colour(COLOR0)
    assert U != V and (got[0][:H] == Y).any()


def test_idempotence_and_geometry(rows, rgb_case):
    frames, want = rgb_case
    got, ovs = gpu_draw(frames, [rows], BATCH[0], times=2)
    assert_same(got, want)                                                 # drawing twice = drawing once
    s = R.sorted_rows(rows)
    geo = ovs[0].geometry()
    assert geo.dtype == np.int32 and geo.shape == (len(s["id"]), 8)
    ref = R.geometry(s, FPS, H, W)
    for k, name in enumerate(R.GEOMETRY):
        assert np.array_equal(geo[:, k], ref[:, k]), name


@pytest.mark.parametrize("params", [dict(thickness=1), dict(thickness=3), dict(label_scale=1), dict(label=False), dict(box=False),
                                    dict(trail=5, radius=4)], ids=lambda p: "-".join(f"{k}{int(v)}" for k, v in p.items()))
def test_parameters_and_switches(rows, params):
    frames = noise((1, H, W, 3), 4)                                        # frame 127: both ids
    want = R.draw(frames, rows, FPS, frame0=127, **params)
    got, _ = gpu_draw(frames, [rows], 127, **params)
    assert_same(got, want)
    assert (want != R.draw(frames, rows, FPS, frame0=127)).any()           # the parameter changes the picture


@pytest.mark.parametrize("stride", [1, 4])
def test_track_video_dir_and_overlay_command(tmp_path, model_path, stride):
    """`track --video_dir` writes the overlay of the DataFrame the same command exports, and `overlay` redraws it from that file"""
    import pandas as pd
    from vbt_amd import synth
    from vbt_amd.cli import main
    frames = synth.clip_frames(12, 0, 12, size=416)
    src = tmp_path / "demo.npy"
    np.save(str(src), frames)
    out, dfs = tmp_path / "out", tmp_path / "dfs"
    res = CliRunner().invoke(main, ["track", str(src), "--model", model_path, "--df_dir", str(dfs), "--fps", "60", "--detection_treshold", "0.3",
                                    "--frame_stride", str(stride), "--video_dir", str(out)])
    assert res.exit_code == 0, res.output
    files = os.listdir(dfs)
    assert len(files) == 1, res.output
    df = pd.read_pickle(os.path.join(dfs, files[0]))
    assert len(df) > 0
    want = R.render(frames, df, 60.0, frame_stride=stride)
    assert want.shape == (12 // stride, 416, 416, 3) and (want != frames[stride - 1::stride]).any()
    got = np.load(str(out / "demo.npy"))
    assert_same(got, want)
    out2 = tmp_path / "out2"
    res = CliRunner().invoke(main, ["overlay", str(src), os.path.join(dfs, files[0]), "--fps", "60", "--frame_stride", str(stride), "--video_dir", str(out2)])
    assert res.exit_code == 0, res.output
    assert (out2 / "demo.npy").read_bytes() == (out / "demo.npy").read_bytes()


def test_overlay_command_writes_raw_yuv_for_size_sources(tmp_path, rows):
    """a --size source comes back as headerless raw video in its own pixel format (no model involved: rows from a stored DataFrame)"""
    import pandas as pd
    from vbt_amd.cli import main
    frames = noise((8, H * 3 // 2, W), 5)                                  # frames 1..8; --frame_stride 2 keeps 2, 4, 6, 8
    src = tmp_path / "clip.yuv"
    frames.tofile(str(src))
    data = {k: v[:8] for k, v in only(rows, {1}).items()}
    df = tmp_path / "clip_id1_model.pkl.gz"
    pd.DataFrame(data).to_pickle(str(df))
    res = CliRunner().invoke(main, ["overlay", str(src), str(df), "--fps", str(FPS), "--frame_stride", "2", "--pix_fmt", "nv12", "--size", f"{W}x{H}",
                                    "--video_dir", str(tmp_path / "out")])
    assert res.exit_code == 0, res.output
    want = R.render(frames, data, FPS, frame_stride=2, pix_fmt="nv12")
    got = np.fromfile(str(tmp_path / "out" / "clip.yuv"), np.uint8).reshape(want.shape)
    assert_same(got, want)
    assert (want != frames[1::2]).any()


def test_track_concurrent_writes_the_same_videos(tmp_path, model_path):
    """--concurrent N renders each clip as it finishes: the same files as one clip at a time"""
    from vbt_amd import synth
    from vbt_amd.cli import main
    srcs = []
    for i in range(2):
        path = tmp_path / f"clip{i}.npy"
        np.save(str(path), synth.clip_frames(12 + i, 3 * i, 10 + 2 * i, size=416))
        srcs.append(str(path))
    common = ["--model", model_path, "--fps", "60", "--detection_treshold", "0.3"]
    for conc, d in ((2, "A"), (1, "B")):
        res = CliRunner().invoke(main, ["track", *srcs, "--concurrent", str(conc), "--video_dir", str(tmp_path / d)] + common)
        assert res.exit_code == 0, res.output
    for i in range(2):
        a, b = np.load(str(tmp_path / "A" / f"clip{i}.npy")), np.load(str(tmp_path / "B" / f"clip{i}.npy"))
        assert a.shape == (10 + 2 * i, 416, 416, 3) and (a != np.load(srcs[i])).any()
        assert_same(a, b)
