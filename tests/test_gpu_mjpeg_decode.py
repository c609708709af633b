"""MJPEG import on the GPU: every decoded frame must EQUAL the numpy statement of the reconstruction contract (tests/mjpeg_dec_ref.py,
itself pinned against Pillow's libjpeg-turbo in tests/test_mjpeg_decode_host.py), at the smallest shapes at which the kernels can go
wrong; a damaged scan spoils its own frame only; an .avi file tracks like the .npy of its frames."""
import os

import numpy as np
import pytest
from click.testing import CliRunner

import mjpeg_dec_ref as D
import mjpeg_ref as M

pytestmark = pytest.mark.gpu

NAMES = sorted(D.vectors())


def gpu_decode(jpegs, dec=None, max_batch=None):
    """-> (frames uint8 [B, H, W, 3], status int32 [B])"""
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.mjpeg import Decoder
    d = D.parse(jpegs[0])
    H, W = d["H"], d["W"]
    dec = dec or Decoder(H, W, max_batch=max_batch or len(jpegs))
    buf = DeviceBuffer(len(jpegs) * H * W * 3)
    dec.decode(jpegs, buf.ptr)
    status = dec.status()
    return buf.to_host((len(jpegs), H, W, 3), np.uint8), status


def assert_same_frame(got, want, what=""):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        y, x, c = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {want.size} samples differ; first at (y {y}, x {x}, c {c}): got {got[y, x, c]}, want {want[y, x, c]}")


@pytest.mark.parametrize("name", NAMES)
def test_every_vector_equals_the_numpy_statement(name):
    jpeg = D.vectors()[name]
    if name == "own-160x32-noise-q95":
        info = {}
        assert M.encode(D.noise((160, 32, 3), 11), 95, info=info) == jpeg
        assert b"\xff\x00" in jpeg[629:-2] and any(n % 8 for n in info["bits"]) and len(info["bits"]) == 10     # a stuffed FF 00, an interval ending inside a byte
    if name == "own-16x2064-one-interval":
        assert D.parse(jpeg)["ri"] * 6 == 774
    frames, status = gpu_decode([jpeg])
    assert status.tolist() == [0]
    assert_same_frame(frames[0], D.expected(name), name)


def test_a_frame_without_dht_decodes_like_the_frame_with_tables():
    with_tables, without = D.vectors()["own-17x33"], D.vectors()["own-17x33-no-dht"]
    assert len(without) == len(with_tables) - 2 * (2 + 19 + 12) - 2 * (2 + 19 + 162)
    frames, status = gpu_decode([with_tables, without])
    assert status.tolist() == [0, 0] and np.array_equal(frames[0], frames[1])
    assert_same_frame(frames[1], D.expected("own-17x33"))


def mixed_batch():
    """five frames of 40 x 56, five kinds: 4:2:0, 4:4:4, grey, constant, noise"""
    v = D.vectors()
    return [v["pil-40x56-no-restarts"], D.pil_jpeg(D.smooth(40, 56, 5), quality=85, subsampling=0), D.pil_jpeg(D.smooth(40, 56, 6)[..., 1], quality=85),
            M.encode(np.full((40, 56, 3), 90, np.uint8), 85), M.encode(D.noise((40, 56, 3), 22), 85)]


def test_batch_of_five_kinds_is_independent_per_frame():
    jpegs = mixed_batch()
    want = [D.decode(j) for j in jpegs]
    assert {(D.parse(j)["comps"][0][:2], len(D.parse(j)["comps"])) for j in jpegs} == {((2, 2), 3), ((1, 1), 3), ((1, 1), 1)}
    for what, order in (("in order", [0, 1, 2, 3, 4]), ("reversed", [4, 3, 2, 1, 0]), ("alone", [2])):
        frames, status = gpu_decode([jpegs[i] for i in order], max_batch=8)
        assert not status.any(), (what, status)
        for k, i in enumerate(order):
            assert_same_frame(frames[k], want[i], f"{what}, frame {i}")


def test_smaller_and_larger_batches_on_one_handle():
    from vbt_amd.mjpeg import Decoder
    jpegs = mixed_batch()
    want = [D.decode(j) for j in jpegs]
    dec = Decoder(40, 56, max_batch=5)
    for first, n in ((0, 5), (1, 3), (4, 1), (0, 5)):
        frames, status = gpu_decode(jpegs[first:first + n], dec=dec)
        assert not status.any()
        for k in range(n):
            assert_same_frame(frames[k], want[first + k], f"{n} frames from {first}, frame {k}")


def test_a_damaged_scan_spoils_its_own_frame_only():
    """the middle frame of three is cut inside its last interval and padded with zeros to its old length: the bounded reader ends that
    interval with a status (the path the CPU fuzz run walks under ASan); the call succeeds; the neighbours are exact"""
    v = D.vectors()
    good0, good2 = v["pil-40x56-restart-rows-1"], v["pil-40x56-420-optimize"]
    bad = D.damaged_frame(good0)
    assert len(bad) == len(good0) and D.decode(bad, with_status=True)[1] != 0
    frames, status = gpu_decode([good0, bad, good2])
    assert status[0] == 0 and status[1] != 0 and status[2] == 0, status
    assert status[1] == D.decode(bad, with_status=True)[1]
    assert_same_frame(frames[0], D.expected("pil-40x56-restart-rows-1"))
    assert_same_frame(frames[2], D.expected("pil-40x56-420-optimize"))


def test_error_codes_leave_the_output_and_the_handle_alone():
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.mjpeg import Decoder
    L = _lib.lib()
    v = D.vectors()
    good = v["pil-40x56-no-restarts"]
    progressive = D.pil_jpeg(D.smooth(40, 56, 4), quality=85, progressive=True)
    dec = Decoder(40, 56, max_batch=3)
    marker = np.full((3, 40, 56, 3), 0xA5, np.uint8)
    buf = DeviceBuffer.from_host(marker)

    def call(jpegs, ptr=None):
        off = np.zeros(len(jpegs) + 1, np.uint64)
        off[1:] = np.cumsum([len(j) for j in jpegs])
        data = np.frombuffer(b"".join(jpegs) or b"\0", np.uint8)
        return L.vbt_mjpeg_decode(dec._h, data.ctypes.data, off.ctypes.data, len(jpegs), buf.ptr if ptr is None else ptr, None)

    st = np.zeros(3, np.int32)
    assert L.vbt_mjpeg_decode_status(dec._h, st.ctypes.data, None) == -5                               # nothing decoded yet
    assert call([good] * 4) == -4 and "created for 3" in L.vbt_last_error().decode()
    assert call([]) == -1
    assert L.vbt_mjpeg_decode(dec._h, None, None, 1, buf.ptr, None) == -1
    assert call([good, good, progressive]) == -2
    text = L.vbt_last_error().decode()
    assert "frame 2" in text and "progressive" in text, text
    assert call([good, v["pil-24x40-444"]]) == -2 and "frame 1" in L.vbt_last_error().decode() and "the handle is for 56x40" in L.vbt_last_error().decode()
    _lib.check(L.vbt_device_synchronize(0))
    assert np.array_equal(buf.to_host(marker.shape, np.uint8), marker)                                  # nothing was enqueued
    frames, status = gpu_decode([good, good], dec=dec)                                                  # the handle is still usable
    assert not status.any()
    assert_same_frame(frames[1], D.expected("pil-40x56-no-restarts"))


# ---- through a file
@pytest.fixture(scope="module")
def clip_files(tmp_path_factory):
    """12 synthetic frames of 416 x 416: clip.avi (written by this project's encoder at 60 frames/s) and clip.npy, the frames AviClip decodes from it"""
    from vbt_amd import synth
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.mjpeg import AviClip, AviWriter, Encoder
    d = tmp_path_factory.mktemp("roundtrip")
    frames = synth.clip_frames(12, 0, 12, size=416)
    enc = Encoder(416, 416, max_batch=12)
    buf = DeviceBuffer.from_host(frames)
    enc.encode(buf.ptr, 12)
    with AviWriter(str(d / "clip.avi"), 416, 416, 60) as w:
        for j in enc.read():
            w.write(j)
    clip = AviClip(str(d / "clip.avi"))
    assert clip.shape == (12, 416, 416, 3) and clip.dtype == np.uint8 and clip.fps == 60.0 and len(clip) == 12
    decoded = clip[:]
    assert not clip.damaged
    assert np.array_equal(clip[3], decoded[3]) and np.array_equal(clip[-1], decoded[11]) and np.array_equal(clip[1:9:4], decoded[1:9:4])
    assert_same_frame(decoded[0], D.decode(clip.reader.frame(0)), "frame 0")
    for k in range(12):                                                                        # what every player shows for this file
        assert_same_frame(decoded[k], D.pil_decode(clip.reader.frame(k)), f"frame {k} against Pillow")
    assert (decoded != decoded[0]).any()
    np.save(str(d / "clip.npy"), decoded)
    return d


@pytest.mark.parametrize("stride", [1, 4])
def test_an_avi_tracks_like_the_npy_of_its_frames(clip_files, tmp_path, model_path, stride):
    import pandas as pd
    from vbt_amd.cli import main
    from vbt_amd.mjpeg import AviReader
    dfs = {}
    for kind, fps in (("avi", []), ("npy", ["--fps", "60"])):                                # the .avi brings its own 60 frames/s
        res = CliRunner().invoke(main, ["track", str(clip_files / f"clip.{kind}"), "--model", model_path, "--df_dir", str(tmp_path / kind),
                                        "--detection_treshold", "0.3", "--frame_stride", str(stride)] + fps)
        assert res.exit_code == 0, res.output
        files = os.listdir(tmp_path / kind)
        assert len(files) == 1, res.output
        dfs[kind] = pd.read_pickle(str(tmp_path / kind / files[0]))
    assert len(dfs["avi"]) > 0
    pd.testing.assert_frame_equal(dfs["avi"], dfs["npy"], check_exact=True)
    assert np.isclose(dfs["avi"]["time"].min() * 60, round(dfs["avi"]["time"].min() * 60))       # times are frame numbers / 60
    df = str(tmp_path / "avi" / os.listdir(tmp_path / "avi")[0])
    res = CliRunner().invoke(main, ["overlay", str(clip_files / "clip.avi"), df, "--video_dir", str(tmp_path / "out"), "--video_format", "mjpeg",
                                    "--frame_stride", str(stride)])
    assert res.exit_code == 0, res.output
    out = AviReader(str(tmp_path / "out" / "clip.avi"))
    assert len(out) == 12 // stride and (out.width, out.height) == (416, 416) and out.rate * stride == 60 * out.scale
    res = CliRunner().invoke(main, ["overlay", str(clip_files / "clip.avi"), df, "--video_dir", str(clip_files), "--video_format", "mjpeg"])
    assert res.exit_code == 2 and "overwrite its own source" in res.output                       # the export is never its own input
    assert len(AviReader(str(clip_files / "clip.avi"))) == 12


def test_decode_into_and_step_runs_without_torch(clip_files, tmp_path, model_path):
    """AviClip.decode_into -> Pipeline.step_runs by device pointer in a child process that never imports torch; its rows are those of
    track_frames on the decoded frames"""
    import pickle
    import subprocess
    import sys
    from vbt_amd.track import track_frames
    code = (
        "import sys, pickle, numpy as np\n"
        "from vbt_amd.mjpeg import AviClip\n"
        "from vbt_amd.mem import DeviceBuffer\n"
        "from vbt_amd.track import Pipeline\n"
        "clip = AviClip(sys.argv[1], batch=8)\n"
        "T, H, W, _ = clip.shape\n"
        "pipe = Pipeline(sys.argv[2], 8, max_frames=T, fps=clip.fps, detection_treshold=0.3, rows_per_frame=25, tracker_clips=1)\n"
        "bufs = [DeviceBuffer(8 * H * W * 3) for _ in range(2)]\n"
        "for k, i0 in enumerate(range(0, T, 8)):\n"
        "    idx = list(range(i0, min(i0 + 8, T)))\n"
        "    pipe.join_detectors(0)\n"
        "    clip.decode_into(idx, bufs[k % 2].ptr, 0)\n"
        "    pipe.step_runs(bufs[k % 2].ptr, [(0, 0, len(idx), i0 + 1, 1)], stream=0, src_hw=None if (H, W) == (pipe._size, pipe._size) else (H, W))\n"
        "pipe.finish()\n"
        "rows = pipe.rows(0)\n"
        "assert 'torch' not in sys.modules, 'torch was imported'\n"
        "pickle.dump(rows, open(sys.argv[3], 'wb'))\n")
    dst = tmp_path / "rows.pkl"
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    subprocess.run([sys.executable, "-c", code, str(clip_files / "clip.avi"), model_path, str(dst)], check=True, cwd=root, timeout=300)
    got = pickle.load(open(dst, "rb"))
    want = track_frames(np.load(str(clip_files / "clip.npy")), model_path, fps=60.0, detection_treshold=0.3, time_batch=8)
    assert len(want["id"]) > 0 and got == want
