"""Scaled export on the GPU (include/vbt_hip.h, "Scaled export"): vbt_scaler against the numpy statement (tests/scale_ref.py), the
scaled encoder against both the numpy encoder on the numpy-scaled frames and the plain encoder on the Scaler's frames, and the
CLI's --display_image_height - everything bit for bit, at the smallest shapes at which the kernels can go wrong.
The Encoder(out_hw=) shapes for nv12 / i420 use a 28 x 796 source where rgb24 uses 27 x 795 (YUV 4:2:0 sides are even); the output,
18 x 530, and with it the MCU geometry is the same."""
import io
import os

import numpy as np
import pytest
from click.testing import CliRunner
from PIL import Image

import mjpeg_ref as M
import overlay_ref as R
import scale_ref as S

pytestmark = pytest.mark.gpu

FPS = 30.0


def gpu_scale(frames, fmt, H, W, h, w, scaler=None):
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.scale import Scaler
    frames = np.ascontiguousarray(frames)
    sc = scaler or Scaler(H, W, h, w, fmt)
    src = DeviceBuffer.from_host(frames)
    shape = (len(frames),) + S.frame_shape(fmt, h, w)
    dst = DeviceBuffer.from_host(np.full(shape, 0xA5, np.uint8))                    # every byte must be written
    sc.run(src.ptr, dst.ptr, len(frames))
    from vbt_amd import _lib
    _lib.check(_lib.lib().vbt_stream_synchronize(None))
    return dst.to_host(shape, np.uint8)


def assert_same_frames(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


def assert_same_bytes(got, want, what="", size=None):
    assert len(got) == len(want), f"{what}: {len(got)} frames, want {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            k = next((j for j in range(min(len(g), len(w))) if g[j] != w[j]), min(len(g), len(w)))
            raise AssertionError(f"{what} frame {i}: {len(g)} bytes, want {len(w)}; first difference at byte {k}: got {g[k:k + 8].hex()}, want {w[k:k + 8].hex()}")
        im = Image.open(io.BytesIO(g))
        im.load()
        if size is not None:
            assert im.size == size, (what, im.size, size)                           # Pillow opens every frame at (w, h)


@pytest.mark.parametrize("case", S.cases(), ids=lambda c: "%s-%dx%d-%dx%d" % c)
def test_scaler_equals_the_numpy_statement(case):
    fmt, H, W, h, w = case
    frames = S.noise((2,) + S.frame_shape(fmt, H, W), 100 + H + W)
    want = S.scale_frames(frames, fmt, h, w)
    got = gpu_scale(frames, fmt, H, W, h, w)
    assert_same_frames(got, want, str(case))
    if (H, W) == (h, w):
        assert np.array_equal(got, frames)                                          # a copy


def test_an_unaligned_destination_takes_the_byte_path():
    """16 x 16 -> 8 x 12 rgb24 has rows of 36 bytes (words), written at a destination one byte off a multiple of 4 (bytes)"""
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.scale import Scaler
    frames = S.noise((2, 16, 16, 3), 31)
    want = S.scale_frames(frames, "rgb24", 8, 12)
    src = DeviceBuffer.from_host(frames)
    dst = DeviceBuffer.from_host(np.full(want.size + 8, 0xA5, np.uint8))
    Scaler(16, 16, 8, 12).run(src.ptr, dst.ptr + 1, 2)
    _lib.check(_lib.lib().vbt_stream_synchronize(None))
    got = dst.to_host((want.size + 8,), np.uint8)
    assert got[0] == 0xA5 and (got[1 + want.size:] == 0xA5).all()
    assert_same_frames(got[1:1 + want.size].reshape(want.shape), want)


def test_batches_on_one_handle_and_the_tables():
    from vbt_amd.scale import Scaler
    H, W, h, w = 30, 46, 20, 30
    frames = S.noise((5, H, W, 3), 32)
    want = S.scale_frames(frames, "rgb24", h, w)
    assert len({f.tobytes() for f in want}) == 5
    sc = Scaler(H, W, h, w)
    assert_same_frames(gpu_scale(frames, "rgb24", H, W, h, w, sc), want, "five")
    assert_same_frames(gpu_scale(frames[3:], "rgb24", H, W, h, w, sc), want[3:], "two after five")
    for axis, (n_src, n_dst) in enumerate(((H, h), (W, w))):
        i0, _, a = S.axis_table(n_src, n_dst)
        g0, ga = sc.tables(0, axis)
        assert g0.tolist() == i0.tolist() and ga.tolist() == a.tolist(), axis
    with pytest.raises(ValueError):
        sc.tables(1, 0)                                                             # an RGB handle has no chroma tables
    sy = Scaler(36, 52, 24, 34, "nv12")
    for plane, axis, n_src, n_dst in ((0, 0, 36, 24), (0, 1, 52, 34), (1, 0, 18, 12), (1, 1, 26, 17)):
        i0, _, a = S.axis_table(n_src, n_dst)
        g0, ga = sy.tables(plane, axis)
        assert g0.tolist() == i0.tolist() and ga.tolist() == a.tolist(), (plane, axis)


def gpu_encode(frames, fmt, H, W, out_hw=None, quality=85):
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.mjpeg import Encoder
    frames = np.ascontiguousarray(frames)
    enc = Encoder(H, W, fmt, quality=quality, max_batch=len(frames), out_hw=out_hw)
    buf = DeviceBuffer.from_host(frames)
    enc.encode(buf.ptr, len(frames))
    return enc.read()


@pytest.mark.parametrize("case", S.enc_cases(), ids=lambda c: "%s-%dx%d-%dx%d" % c)
def test_scaled_encoder_equals_scale_then_encode(case):
    fmt, H, W, h, w = case
    frames = S.noise((2,) + S.frame_shape(fmt, H, W), 200 + H + W)
    got = gpu_encode(frames, fmt, H, W, out_hw=(h, w))
    scaled = S.scale_frames(frames, fmt, h, w)
    assert_same_bytes(got, [M.encode(f, 85, fmt) for f in scaled], f"{case} against the numpy statements", size=(w, h))
    assert_same_bytes(got, gpu_encode(gpu_scale(frames, fmt, H, W, h, w), fmt, h, w), f"{case} against Scaler + Encoder")


def test_scaled_encoder_nv12_and_i420_agree_and_full_size_is_the_plain_encoder():
    H, W, h, w = 36, 52, 24, 34
    nv12 = S.noise((2, H * 3 // 2, W), 33)
    uv = nv12[:, H:].reshape(2, H // 2, W // 2, 2)
    i420 = np.concatenate([nv12[:, :H].reshape(2, -1), uv[..., 0].reshape(2, -1), uv[..., 1].reshape(2, -1)], axis=1).reshape(2, H * 3 // 2, W)
    a = gpu_encode(nv12, "nv12", H, W, out_hw=(h, w))
    assert_same_bytes(gpu_encode(i420, "i420", H, W, out_hw=(h, w)), a, "i420 against nv12", size=(w, h))
    assert_same_bytes(a, [M.encode(f, 85, "nv12") for f in S.scale_frames(nv12, "nv12", h, w)], "nv12")
    for fmt, frames in (("nv12", nv12), ("rgb24", S.noise((2, H, W, 3), 34))):
        assert_same_bytes(gpu_encode(frames, fmt, H, W, out_hw=(H, W)), gpu_encode(frames, fmt, H, W), f"{fmt} at full size", size=(W, H))


# ---- rows for the overlay: one id moving across the frame, a second one on two frames
OH, OW = 72, 104
BATCH = (126, 127, 128, 129, 130, 131)


def rows():
    d = {k: [] for k in R.COLUMNS}

    def add(tid, f, x, y, h=0.3, w=0.22):
        for k, v in zip(R.COLUMNS, (tid, f / FPS, x, y, 0.0, 0.0, h, w)):
            d[k].append(v)
    for f in list(range(100, 130)) + [131, 132]:
        add(1, f, 0.5 + 0.38 * np.sin(2 * np.pi * f / 37), 0.5 + 0.36 * np.sin(2 * np.pi * f / 23 + 0.7))
    add(12, 127, 0.45, 0.6)
    add(12, 129, 0.55, 0.6)
    return d


@pytest.mark.parametrize("fmt", ["rgb24", "nv12"])
def test_draw_then_encode_scaled_on_one_stream(fmt):
    """vbt_overlay_draw and the scaled vbt_mjpeg_encode back to back on one stream, no host synchronisation in between"""
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.mjpeg import Encoder
    from vbt_amd.overlay import Overlay
    h, w = 36, 52
    data = rows()
    frames = S.noise((len(BATCH),) + S.frame_shape(fmt, OH, OW), 40)
    drawn = R.draw(frames, data, FPS, frame0=BATCH[0], pix_fmt=fmt)
    assert (drawn != frames).any()
    want = [M.encode(f, 85, fmt) for f in S.scale_frames(drawn, fmt, h, w)]
    assert want != [M.encode(f, 85, fmt) for f in S.scale_frames(frames, fmt, h, w)]
    buf = DeviceBuffer.from_host(frames)
    ov = Overlay(OH, OW, fmt)
    ov.set_rows(data, FPS)
    enc = Encoder(OH, OW, fmt, max_batch=len(BATCH), out_hw=(h, w))
    ov.draw(buf.ptr, len(BATCH), BATCH[0])
    enc.encode(buf.ptr, len(BATCH))
    assert_same_bytes(enc.read(), want, fmt, size=(w, h))


@pytest.mark.parametrize("fmt", ["rgb24", "i420"])
def test_render_with_a_short_last_batch(tmp_path, fmt):
    """overlay.render(display_hw=) on 5 kept frames, 2 at a time, into a sink and into an array"""
    from vbt_amd.mjpeg import AviWriter
    from vbt_amd.overlay import render
    h, w = 36, 52
    data = rows()
    frames = S.noise((11,) + S.frame_shape(fmt, OH, OW), 42)
    shifted = dict(data, time=[t - 120 / FPS for t in data["time"]])                # clip frames 2, 4 .. 10 are frames 122 .. 130 of the rows
    small = S.scale_frames(R.render(frames, shifted, FPS, frame_stride=2, pix_fmt=fmt), fmt, h, w)
    assert len(small) == 5
    path = tmp_path / "tail.avi"
    with AviWriter(str(path), w, h, 15) as sink:
        assert render(frames, shifted, FPS, frame_stride=2, pix_fmt=fmt, batch=2, sink=sink, quality=90, display_hw=(h, w)) == 5
    avi = M.avi_parse(path.read_bytes())
    assert_same_bytes(avi["frames"], [M.encode(f, 90, fmt) for f in small], fmt, size=(w, h))
    assert_same_frames(render(frames, shifted, FPS, frame_stride=2, pix_fmt=fmt, batch=2, display_hw=(h, w)), small, fmt)
    with pytest.raises(ValueError, match="render: out must be uint8"):
        render(frames, shifted, FPS, frame_stride=2, pix_fmt=fmt, out=np.empty((5,) + S.frame_shape(fmt, OH, OW), np.uint8), display_hw=(h, w))


@pytest.fixture(scope="module")
def tracked(tmp_path_factory, model_path):
    """the synthetic clip, tracked once by `track ... --display_image_height 24` (two passes, mjpeg): (dir, frames, DataFrame, small frames)"""
    import pandas as pd
    from vbt_amd import synth
    from vbt_amd.cli import main
    d = tmp_path_factory.mktemp("scaled")
    frames = synth.clip_frames(12, 0, 12, size=416)
    np.save(str(d / "clip.npy"), frames)
    base = ["track", str(d / "clip.npy"), "--model", model_path, "--detection_treshold", "0.3", "--fps", "60", "--display_image_height", "24"]
    res = CliRunner().invoke(main, base + ["--df_dir", str(d / "dfs"), "--video_dir", str(d / "a"), "--video_format", "mjpeg"])
    assert res.exit_code == 0, res.output
    files = os.listdir(d / "dfs")
    assert len(files) == 1
    df = pd.read_pickle(str(d / "dfs" / files[0]))
    full = R.render(frames, df, 60.0)                                               # what the full-size raw export holds (tests/test_gpu_mjpeg.py)
    assert (full != frames).any()
    return d, base, str(d / "dfs" / files[0]), S.scale_frames(full, "rgb24", 24, 24)


def test_cli_writes_the_same_scaled_avi_on_every_route(tracked):
    from vbt_amd.cli import main
    d, base, df, small = tracked
    a = (d / "a" / "clip.avi").read_bytes()
    avi = M.avi_parse(a)
    assert (avi["avih"]["width"], avi["avih"]["height"]) == (24, 24) and avi["avih"]["total_frames"] == 12
    assert_same_bytes(avi["frames"], [M.encode(f, 85) for f in small], "track", size=(24, 24))
    res = CliRunner().invoke(main, base + ["--video_dir", str(d / "b"), "--video_format", "mjpeg", "--one_pass"])
    assert res.exit_code == 0, res.output
    assert (d / "b" / "clip.avi").read_bytes() == a
    res = CliRunner().invoke(main, ["overlay", str(d / "clip.npy"), df, "--fps", "60", "--video_dir", str(d / "c"), "--video_format", "mjpeg",
                                    "--display_image_height", "24"])
    assert res.exit_code == 0, res.output
    assert (d / "c" / "clip.avi").read_bytes() == a


def test_cli_raw_route_writes_scaled_frames(tracked):
    from vbt_amd.cli import main
    d, base, df, small = tracked
    res = CliRunner().invoke(main, base + ["--video_dir", str(d / "r1"), "--one_pass"])
    assert res.exit_code == 0, res.output
    got = np.load(str(d / "r1" / "clip.npy"))
    assert got.shape == (12, 24, 24, 3)
    assert_same_frames(got, small, "track --one_pass")
    res = CliRunner().invoke(main, ["overlay", str(d / "clip.npy"), df, "--fps", "60", "--video_dir", str(d / "r2"), "--display_image_height", "24"])
    assert res.exit_code == 0, res.output
    assert_same_frames(np.load(str(d / "r2" / "clip.npy")), small, "overlay")
