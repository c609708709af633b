"""MJPEG export on the GPU: the bytes of every frame must EQUAL those of the numpy statement of the bitstream contract
(tests/mjpeg_ref.py), at the smallest shapes at which the kernels can go wrong; every frame must open in Pillow."""
import io
import os

import numpy as np
import pytest
from click.testing import CliRunner
from PIL import Image

import mjpeg_ref as M
import overlay_ref as R

pytestmark = pytest.mark.gpu

FPS = 30.0
PSNR_MARGIN_DB = 0.25        # as tests/test_mjpeg_host.py: the larger of 0.25 dB and twice the largest measured shortfall (0.047 dB)


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def gpu_encode(frames, pix_fmt="rgb24", quality=85, max_batch=None):
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.mjpeg import Encoder
    from vbt_amd.rawvideo import source_hw
    frames = np.ascontiguousarray(frames)
    H, W = source_hw(frames, pix_fmt)
    enc = Encoder(H, W, pix_fmt, quality=quality, max_batch=max_batch or len(frames))
    buf = DeviceBuffer.from_host(frames)
    enc.encode(buf.ptr, len(frames))
    return enc.read()


def assert_same_bytes(got, want, what=""):
    assert len(got) == len(want), f"{what}: {len(got)} frames, want {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            k = next((j for j in range(min(len(g), len(w))) if g[j] != w[j]), min(len(g), len(w)))
            raise AssertionError(f"{what} frame {i}: {len(g)} bytes, want {len(w)}; first difference at byte {k}: "
                                 f"got {g[k:k + 8].hex()}, want {w[k:k + 8].hex()}")
        im = Image.open(io.BytesIO(g))
        im.load()                                                                  # every GPU frame decodes in Pillow


@pytest.mark.parametrize("shape,seed", [((16, 16), 1), ((17, 33), 2), ((1, 1), 3)], ids=["one-mcu", "padded-both-axes", "one-pixel"])
def test_small_rgb_frames(shape, seed):
    frame = noise(shape + (3,), seed)
    want = M.encode(frame, 85)
    if shape == (16, 16):
        assert not any(want[i] == 0xFF and 0xD0 <= want[i + 1] <= 0xD7 for i in range(629, len(want) - 2))      # one interval: no RST
    assert_same_bytes(gpu_encode(frame[None]), [want], str(shape))


def test_ten_intervals_stuffing_and_unaligned_intervals():
    """160 x 32 noise at q = 95: RST7 wraps to RST0; the reference stream holds a stuffed FF 00 and an interval that ends inside a byte"""
    frame = noise((160, 32, 3), 11)
    info = {}
    want = M.encode(frame, 95, info=info)
    assert len(info["bits"]) == 10 and any(n % 8 for n in info["bits"]) and any(b"\xff" in raw for raw in info["raw"])
    body = want[629:-2]
    assert b"\xff\x00" in body
    assert [body[i + 1] for i in range(len(body) - 1) if body[i] == 0xFF and body[i + 1] != 0] == [0xD0 + i % 8 for i in range(9)]
    assert_same_bytes(gpu_encode(frame[None], quality=95), [want])


def test_one_long_interval():
    """16 x 2064: 129 MCUs = 774 blocks in one interval - five groups of the transform kernel, four chunks of the entropy kernel's walk"""
    frame = noise((16, 2064, 3), 12)
    frame[:, 700:1500] = (np.arange(800)[None, :, None] // 4).astype(np.uint8)     # a smooth stretch: short blocks next to long ones
    assert_same_bytes(gpu_encode(frame[None]), [M.encode(frame, 85)])


def test_nv12_and_i420_give_identical_bytes():
    H, W = 48, 64
    nv12 = noise((H * 3 // 2, W), 13)
    nv12[0, :4] = (16, 235, 0, 255)
    nv12[H, :4] = (16, 240, 240, 16)                                               # the chroma ties of the range expansion
    uv = nv12[H:].reshape(H // 2, W // 2, 2)
    i420 = np.concatenate([nv12[:H].reshape(-1), uv[..., 0].reshape(-1), uv[..., 1].reshape(-1)]).reshape(H * 3 // 2, W)
    want = M.encode(nv12, 85, "nv12")
    assert want == M.encode(i420, 85, "i420")
    a, b = gpu_encode(nv12[None], "nv12"), gpu_encode(i420[None], "i420")
    assert_same_bytes(a, [want], "nv12")
    assert_same_bytes(b, [want], "i420")


@pytest.mark.parametrize("value", [0, 255])
def test_constant_frames(value):
    frame = np.full((40, 24, 3), value, np.uint8)
    assert_same_bytes(gpu_encode(frame[None]), [M.encode(frame, 85)])


@pytest.mark.parametrize("q", [1, 100])
def test_quality_extremes_on_noise(q):
    """the clamps of the tables (Q = 255 at q = 1, Q = 1 at q = 100) and the longest codes.  The scratch is sized for the worst case, so q = 100 on noise must match the reference - VBT_ERR_CAPACITY is
    not an accepted outcome"""
    frame = noise((32, 48, 3), 14)
    frame[:8, :8] = (np.indices((8, 8)).sum(0) & 1)[..., None] * 255                # a 0 / 255 checkerboard: the largest coefficients
    assert_same_bytes(gpu_encode(frame[None], quality=q), [M.encode(frame, q)])


def test_batch_of_five_frames_is_independent_per_frame():
    frames = np.stack([noise((40, 56, 3), 20), np.full((40, 56, 3), 90, np.uint8), noise((40, 56, 3), 21) // 8, noise((40, 56, 3), 22),
                       np.zeros((40, 56, 3), np.uint8)])
    want = [M.encode(f, 85) for f in frames]
    assert len({len(w) for w in want}) >= 4
    got = gpu_encode(frames, max_batch=8)
    assert_same_bytes(got, want)
    assert_same_bytes(gpu_encode(frames[::-1], max_batch=5), want[::-1], "reversed")     # frame i does not depend on its neighbours
    assert_same_bytes(gpu_encode(frames[2:3]), want[2:3], "alone")


def test_a_smaller_batch_after_a_larger_one_on_one_handle():
    """5 frames, then 3, then 5 again through one Encoder: the overflow flag has a place of its own, so what an earlier batch left in the
    offset table is never read as a flag"""
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.mjpeg import Encoder
    frames = noise((5, 24, 40, 3), 23)
    want = [M.encode(f, 85) for f in frames]
    buf = DeviceBuffer.from_host(frames)
    enc = Encoder(24, 40, max_batch=5)
    for first, n in ((0, 5), (1, 3), (4, 1), (0, 5)):
        enc.encode(buf.ptr + first * 24 * 40 * 3, n)
        assert_same_bytes(enc.read(), want[first:first + n], f"{n} frames from {first}")


def test_error_codes_and_the_small_buffer():
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.mjpeg import Encoder
    L = _lib.lib()
    frames = noise((3, 16, 16, 3), 30)
    buf = DeviceBuffer.from_host(frames)
    enc = Encoder(16, 16, max_batch=2)
    off = np.zeros(4, np.uint64)
    host = np.zeros(1 << 16, np.uint8)
    assert L.vbt_mjpeg_read(enc._h, host.ctypes.data, host.nbytes, off.ctypes.data, None) == -5         # nothing encoded
    assert L.vbt_mjpeg_encode(enc._h, buf.ptr, 3, None) == -4 and "created for 2" in L.vbt_last_error().decode()
    assert L.vbt_mjpeg_encode(enc._h, buf.ptr, 2, None) == 0
    assert L.vbt_mjpeg_encode(enc._h, buf.ptr, 2, None) == -5 and "not been read" in L.vbt_last_error().decode()
    want = [M.encode(f, 85) for f in frames[:2]]
    assert L.vbt_mjpeg_read(enc._h, host.ctypes.data, 100, off.ctypes.data, None) == -4                 # too small: the batch stays readable
    assert int(off[2]) == len(want[0]) + len(want[1]) and not host.any()
    assert L.vbt_mjpeg_read(enc._h, host.ctypes.data, host.nbytes, off.ctypes.data, None) == 0
    assert off[:3].tolist() == [0, len(want[0]), len(want[0]) + len(want[1])] and host[:int(off[2])].tobytes() == want[0] + want[1]
    assert L.vbt_mjpeg_read(enc._h, host.ctypes.data, host.nbytes, off.ctypes.data, None) == -5
    enc.encode(buf.ptr + 16 * 16 * 3, 2)                                                                # the handle is free again
    assert_same_bytes(enc.read(), [M.encode(f, 85) for f in frames[1:]])


# ---- the synthetic rows of the overlay tests, re-stated
H, W = 72, 104
BATCH = (126, 127, 128, 129, 130, 131)


def synthetic_rows():
    """id 1 on a Lissajous path over frames 1..129, 131, 132 with boxes over every border of the frame at 126..129; id 12 on frames 127
    and 129; frame 130 has no row"""
    d = {k: [] for k in R.COLUMNS}

    def add(tid, f, x, y, h=0.3, w=0.22):
        for k, v in zip(R.COLUMNS, (tid, f / FPS, x, y, 0.0, 0.0, h, w)):
            d[k].append(v)
    for f in list(range(1, 130)) + [131, 132]:
        x, y = 0.5 + 0.38 * np.sin(2 * np.pi * f / 37), 0.5 + 0.36 * np.sin(2 * np.pi * f / 23 + 0.7)
        x, y = {126: (0.03, y), 127: (x, 0.05), 128: (1.02, y), 129: (x, 0.97), 131: (0.0, 0.0)}.get(f, (x, y))
        add(1, f, x, y)
    add(12, 127, 0.45, 0.6, h=2 * (0.6 - 30.5 / H))
    add(12, 129, 0.55, 0.6, h=2 * (0.6 - 31.5 / H))
    return d


@pytest.mark.parametrize("fmt", ["rgb24", "nv12"])
def test_draw_then_encode_on_one_stream(fmt):
    """vbt_overlay_draw and vbt_mjpeg_encode back to back on one stream, no host synchronisation in between"""
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.mjpeg import Encoder
    from vbt_amd.overlay import Overlay
    rows = synthetic_rows()
    frames = noise((len(BATCH), H, W, 3), 40) if fmt == "rgb24" else noise((len(BATCH), H * 3 // 2, W), 41)
    drawn = R.draw(frames, rows, FPS, frame0=BATCH[0], pix_fmt=fmt)
    assert (drawn != frames).any() and np.array_equal(drawn[4], frames[4])
    want = [M.encode(f, 85, fmt) for f in drawn]
    assert want != [M.encode(f, 85, fmt) for f in frames]
    buf = DeviceBuffer.from_host(frames)
    ov = Overlay(H, W, fmt)
    ov.set_rows(rows, FPS)
    enc = Encoder(H, W, fmt, max_batch=len(BATCH))
    ov.draw(buf.ptr, len(BATCH), BATCH[0])
    enc.encode(buf.ptr, len(BATCH))
    assert_same_bytes(enc.read(), want, fmt)


@pytest.mark.parametrize("fmt", ["rgb24", "i420"])
def test_render_into_a_sink_with_a_short_last_batch(tmp_path, fmt):
    """overlay.render(sink=) on 10 kept frames, 4 at a time: batches of 4, 4 and 2 through one Encoder; every frame byte for byte"""
    from vbt_amd.mjpeg import AviWriter
    from vbt_amd.overlay import render
    rows = synthetic_rows()
    frames = noise((21, H, W, 3), 42) if fmt == "rgb24" else noise((21, H * 3 // 2, W), 43)
    shifted = dict(rows, time=[t - 110 / FPS for t in rows["time"]])               # clip frames 2, 4 .. 20 are frames 112 .. 130 of the rows
    drawn = R.render(frames, shifted, FPS, frame_stride=2, pix_fmt=fmt)
    assert len(drawn) == 10 and (drawn != frames[1::2]).any()
    path = tmp_path / "tail.avi"
    with AviWriter(str(path), W, H, 15) as sink:
        assert render(frames, shifted, FPS, frame_stride=2, pix_fmt=fmt, batch=4, sink=sink, quality=90) == 10
    avi = M.avi_parse(path.read_bytes())
    assert_same_bytes(avi["frames"], [M.encode(f, 90, fmt) for f in drawn], fmt)
    assert avi["avih"]["total_frames"] == 10


def _avi_frames(path):
    avi = M.avi_parse(open(path, "rb").read())
    assert avi["avih"]["total_frames"] == len(avi["frames"]) == len(avi["idx"]) == avi["strh"]["length"]
    return avi, [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in avi["frames"]]


@pytest.mark.parametrize("stride", [1, 4])
def test_track_and_overlay_commands_write_an_avi(tmp_path, model_path, stride):
    import pandas as pd
    from vbt_amd import synth
    from vbt_amd.cli import main
    frames = synth.clip_frames(12, 0, 12, size=416)
    src = tmp_path / "clip.npy"
    np.save(str(src), frames)
    common = ["--fps", "60", "--frame_stride", str(stride)]
    track = ["track", str(src), "--model", model_path, "--df_dir", str(tmp_path / "dfs"), "--detection_treshold", "0.3"] + common
    res = CliRunner().invoke(main, track + ["--video_dir", str(tmp_path / "d"), "--video_format", "mjpeg"])
    assert res.exit_code == 0, res.output
    res = CliRunner().invoke(main, track + ["--video_dir", str(tmp_path / "raw"), "--video_format", "raw"])
    assert res.exit_code == 0, res.output
    files = os.listdir(tmp_path / "dfs")
    assert len(files) == 1
    df = pd.read_pickle(str(tmp_path / "dfs" / files[0]))
    raw = np.load(str(tmp_path / "raw" / "clip.npy"))
    assert np.array_equal(raw, R.render(frames, df, 60.0, frame_stride=stride))        # the raw export is what it was
    assert sorted(os.listdir(tmp_path / "d")) == ["clip.avi"]
    avi, decoded = _avi_frames(str(tmp_path / "d" / "clip.avi"))
    assert len(decoded) == 12 // stride and (avi["avih"]["width"], avi["avih"]["height"]) == (416, 416)
    assert avi["strh"]["rate"] * stride == 60 * avi["strh"]["scale"]                   # plays at fps / frame_stride
    for k, (got, want) in enumerate(zip(decoded, raw)):
        pil = io.BytesIO()
        Image.fromarray(want).save(pil, "JPEG", quality=85, subsampling=2, restart_marker_rows=1)
        bound = M.psnr(np.asarray(Image.open(io.BytesIO(pil.getvalue()))), want) - PSNR_MARGIN_DB
        assert M.psnr(got, want) >= bound, (k, M.psnr(got, want), bound)
    res = CliRunner().invoke(main, ["overlay", str(src), str(tmp_path / "dfs" / files[0]), "--video_dir", str(tmp_path / "d2"), "--video_format", "mjpeg"] + common)
    assert res.exit_code == 0, res.output
    assert (tmp_path / "d2" / "clip.avi").read_bytes() == (tmp_path / "d" / "clip.avi").read_bytes()


def test_overlay_command_writes_an_avi_for_yuv_sources(tmp_path):
    import pandas as pd
    from vbt_amd.cli import main
    frames = noise((8, H * 3 // 2, W), 50) // 2 + 64
    src = tmp_path / "clip.yuv"
    frames.tofile(str(src))
    rows = synthetic_rows()
    keep = [i for i, v in enumerate(rows["id"]) if v == 1][:8]
    data = {k: [rows[k][i] for i in keep] for k in rows}
    df = tmp_path / "clip_id1_model.pkl.gz"
    pd.DataFrame(data).to_pickle(str(df))
    res = CliRunner().invoke(main, ["overlay", str(src), str(df), "--fps", str(FPS), "--frame_stride", "2", "--pix_fmt", "nv12", "--size", f"{W}x{H}",
                                    "--video_dir", str(tmp_path / "out"), "--video_format", "mjpeg", "--video_quality", "90"])
    assert res.exit_code == 0, res.output
    avi = M.avi_parse((tmp_path / "out" / "clip.avi").read_bytes())
    drawn = R.render(frames, data, FPS, frame_stride=2, pix_fmt="nv12")
    assert avi["frames"] == [M.encode(f, 90, "nv12") for f in drawn] and len(drawn) == 4
    assert (avi["strh"]["rate"], avi["strh"]["scale"]) == (15, 1)


def test_track_concurrent_writes_the_same_avi(tmp_path, model_path):
    """--concurrent N --video_format mjpeg renders each clip as it finishes: the same files as one clip at a time"""
    from vbt_amd import synth
    from vbt_amd.cli import main
    srcs = []
    for i in range(2):
        path = tmp_path / f"clip{i}.npy"
        np.save(str(path), synth.clip_frames(12 + i, 3 * i, 10 + 2 * i, size=416))
        srcs.append(str(path))
    common = ["--model", model_path, "--fps", "60", "--detection_treshold", "0.3", "--video_format", "mjpeg", "--time_batch", "8"]
    for conc, d in ((2, "A"), (1, "B")):
        res = CliRunner().invoke(main, ["track", *srcs, "--concurrent", str(conc), "--video_dir", str(tmp_path / d)] + common)
        assert res.exit_code == 0, res.output
    for i in range(2):
        a, b = (tmp_path / "A" / f"clip{i}.avi").read_bytes(), (tmp_path / "B" / f"clip{i}.avi").read_bytes()
        assert a == b
        _, decoded = _avi_frames(str(tmp_path / "A" / f"clip{i}.avi"))
        assert len(decoded) == 10 + 2 * i and decoded[0].shape == (416, 416, 3)          # 10 and 12 frames, 8 at a time: a short last batch
