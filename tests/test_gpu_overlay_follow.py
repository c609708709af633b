"""Follow mode of the tracking overlay on the GPU (include/vbt_hip.h, "Following a device row log"): frames drawn from a row log in
device memory that grows while they are drawn, bit for bit against the numpy statement of the raster contract (tests/overlay_ref.py)
and against the two-pass render of the same rows - from a synthetic log, from a real tracker's log, and through the pipeline and
`track --one_pass`."""
import os

import numpy as np
import pytest
from click.testing import CliRunner

import overlay_follow_util as U
import overlay_ref as R
from test_gpu_overlay import BATCH, COLOR0, FPS, H, W, assert_same, noise, synthetic_rows

pytestmark = pytest.mark.gpu

MAX_FRAME = 132


class DeviceLog:
    """a row log in device memory with its device counter, appended from the host the way a tracker appends on the device"""

    def __init__(self, cap):
        from vbt_amd.mem import DeviceBuffer
        self.cap, self.n = cap, 0
        self.rows = DeviceBuffer(cap * 64)
        self.count = DeviceBuffer.from_host(np.zeros(1, np.int32))

    def set_count(self, n):
        from vbt_amd import _lib
        c = np.array([n], np.int32)
        _lib.check(_lib.lib().vbt_memcpy(self.count.ptr, c.ctypes.data, 4, 0))
        self.n = n

    def append(self, recs):
        from vbt_amd import _lib
        recs = np.ascontiguousarray(recs)
        if len(recs):
            _lib.check(_lib.lib().vbt_memcpy(self.rows.ptr + self.n * 64, recs.ctypes.data, recs.nbytes, 0))   # the rows, then the counter
        self.set_count(self.n + len(recs))


def follow_draw(frames, log, frame0, upto, by_frame, frame_step=1, pix_fmt="rgb24", hw=(H, W), times=1, mrpf=25, **params):
    """frames through the device, drawn by a handle that followed `log` through frame `upto` - frame by frame or in one update;
    (frames back, handle, device log)"""
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.overlay import Overlay
    frames = np.ascontiguousarray(frames)
    buf = DeviceBuffer.from_host(frames)
    dl = DeviceLog(len(log) + 3)
    ov = Overlay(hw[0], hw[1], pix_fmt, **params)
    ov.follow(dl.rows.ptr, dl.count.ptr, dl.cap, MAX_FRAME, mrpf, FPS)
    f = U.frames_of(log, FPS)
    n = int((f <= upto).sum())
    assert (f[:n] <= upto).all()                                                     # a prefix of the log
    cuts = [0] + [i for i in range(1, n) if f[i] != f[i - 1]] + [n] if by_frame else [0, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        dl.append(log[a:b])
        ov.follow_update()
    for _ in range(times):
        ov.draw(buf.ptr, len(frames), frame0, frame_step)
    _lib.check(_lib.lib().vbt_stream_synchronize(None))
    return buf.to_host(frames.shape, np.uint8), ov, dl


@pytest.fixture(scope="module")
def rows():
    return synthetic_rows()


@pytest.fixture(scope="module")
def log(rows):
    out = U.emission_log(rows)
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def rgb_case(rows):
    frames = noise((len(BATCH), H, W, 3), 1)
    want = R.draw(frames, rows, FPS, frame0=BATCH[0])
    want.setflags(write=False)
    return frames, want


@pytest.mark.parametrize("by_frame", [True, False], ids=["frame-by-frame", "one-update"])
def test_rgb24_batch_is_bit_exact_and_geometry_is_the_references(log, rgb_case, by_frame):
    frames, want = rgb_case
    got, ov, _ = follow_draw(frames, log, BATCH[0], MAX_FRAME, by_frame, times=2)     # drawing twice = drawing once
    assert np.array_equal(got[4], frames[4]) and (got[5] != frames[5]).any()          # frame 130 has no row, frame 131 has one
    assert_same(got, want)
    assert ov.follow_status() == (len(log), 0)
    geo = ov.geometry()
    ref, _ = U.reference(log, FPS, H, W)
    assert geo.dtype == np.int32 and geo.shape == (len(log), 8)
    for k, name in enumerate(R.GEOMETRY):
        assert np.array_equal(geo[:, k], ref[:, k]), name


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_yuv_formats_are_bit_exact(rows, log, fmt):
    frames = noise((len(BATCH), H * 3 // 2, W), 3)
    want = R.draw(frames, rows, FPS, frame0=BATCH[0], pix_fmt=fmt, rgb=COLOR0)
    got, _, _ = follow_draw(frames, log, BATCH[0], MAX_FRAME, True, pix_fmt=fmt, rgb=COLOR0)
    assert np.array_equal(got[4], frames[4])
    assert_same(got, want)


@pytest.mark.parametrize("by_frame", [True, False], ids=["frame-by-frame", "one-update"])
def test_a_batch_past_the_log_leaves_those_frames_and_later_rows_reach_no_earlier_frame(log, rgb_case, by_frame):
    frames, _ = rgb_case
    f = U.frames_of(log, FPS)
    want = R.draw(frames, U.as_data(log[f <= 128]), FPS, frame0=BATCH[0])             # the clip as if it ended at frame 128
    got, ov, dl = follow_draw(frames, log, BATCH[0], 128, by_frame)
    assert_same(got, want)
    assert np.array_equal(got[3:], frames[3:])
    # the rest of the log arrives: frames 126..128 come out as before (and as with the whole clip), the later ones are drawn now
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer
    dl.append(log[f > 128])
    ov.follow_update()
    buf = DeviceBuffer.from_host(frames)
    ov.draw(buf.ptr, len(frames), BATCH[0])
    _lib.check(_lib.lib().vbt_stream_synchronize(None))
    full = buf.to_host(frames.shape, np.uint8)
    assert_same(full, R.draw(frames, U.as_data(log), FPS, frame0=BATCH[0]))
    assert_same(full[:3], got[:3])


def test_frame_step_odd_sizes_and_trail_parameters(rows, log):
    h, w = 71, 101
    frames = noise((4, h, w, 3), 2)                                                  # frames 125, 127, 129, 131
    got, _, _ = follow_draw(frames, log, 125, MAX_FRAME, True, frame_step=2, hw=(h, w))
    assert_same(got, R.draw(frames, rows, FPS, frame0=125, frame_step=2))
    one = noise((1, H, W, 3), 4)                                                     # frame 127: both ids
    for params in (dict(trail=5, radius=4), dict(trail=17), dict(trail=33, thickness=3), dict(trail=1), dict(label=False, box=False)):
        got, _, _ = follow_draw(one, log, 127, MAX_FRAME, False, **params)
        assert_same(got, R.draw(one, rows, FPS, frame0=127, **params))


def test_empty_update_rewind_and_switching_back(rows, log, rgb_case):
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer
    frames, want = rgb_case
    got, ov, dl = follow_draw(frames, log, BATCH[0], MAX_FRAME, False)
    geo = ov.geometry()
    ov.follow_update()                                                               # no new row: nothing changes
    assert ov.follow_status() == (len(log), 0) and np.array_equal(ov.geometry(), geo)
    dl.set_count(0)                                                                  # the clip was reset: nothing is consumed, the flag says so
    ov.follow_update()
    assert ov.follow_status() == (len(log), U.REWOUND) and np.array_equal(ov.geometry(), geo)
    ov.follow(dl.rows.ptr, dl.count.ptr, dl.cap, MAX_FRAME, 25, FPS)                 # the caller follows again, from the start of the new clip
    assert ov.follow_status() == (0, 0)
    dl.append(log[:70])
    ov.follow_update()
    assert ov.follow_status() == (70, 0)
    ov.set_rows(rows, FPS)                                                           # back to sorted mode: what test_gpu_overlay draws
    buf = DeviceBuffer.from_host(frames)
    ov.draw(buf.ptr, len(frames), BATCH[0])
    _lib.check(_lib.lib().vbt_stream_synchronize(None))
    assert_same(buf.to_host(frames.shape, np.uint8), want)
    with pytest.raises(_lib.VbtError):
        ov.follow_update()                                                           # not in follow mode any more


def test_skipped_rows_on_the_device(log, rgb_case):
    """rows that must be skipped take the kernel off its side-by-side path: exactly they are skipped, the flags say why, and the
    frames come out as from the clean log"""
    frames, want = rgb_case
    f = U.frames_of(log, FPS)
    bad = np.concatenate([log[:61], log[60:61], log[60:61], log[61:], log[-1:]])
    bad["x"][61] = np.nan                                                            # BAD_ROW
    bad["time"][62] = 40 / FPS                                                       # ORDER
    bad["time"][-1] = 133 / FPS                                                      # FRAME_RANGE
    clean = np.ones(len(bad), bool)
    clean[[61, 62, len(bad) - 1]] = False
    ref, _ = U.reference(log, FPS, H, W)
    for by_frame in (True, False):
        got, ov, _ = follow_draw(frames, bad, BATCH[0], 1 << 30, by_frame)
        assert ov.follow_status() == (len(bad), U.BAD_ROW | U.ORDER | U.FRAME_RANGE)
        geo = ov.geometry()
        assert np.array_equal(geo[clean], ref) and (geo[~clean, 7] == 0).all() and not geo[61].any()
        assert_same(got, want)
    # a frame that is full: with room for one row per frame, id 12 at frames 127 and 129 is skipped
    got, ov, _ = follow_draw(frames, log, BATCH[0], MAX_FRAME, False, mrpf=1)
    assert ov.follow_status() == (len(log), U.FRAME_FULL)
    assert (ov.geometry()[:, 7] == 0).tolist() == (log["id"] == 12).tolist()
    assert_same(got, R.draw(frames, U.as_data(log[log["id"] == 1]), FPS, frame0=BATCH[0]))


def crossing_scene(n_frames=140, gap=(60, 64)):
    """two plates that cross, nothing detected on frames 60..63; detections [x1, y1, x2, y2, score, class] per frame and the times"""
    frames, times = [], []
    for fr in range(1, n_frames + 1):
        if gap[0] <= fr < gap[1]:
            continue
        d = [[cx - 0.08, cy - 0.1, cx + 0.08, cy + 0.1, 0.9, 0.0] for cx, cy in ((0.2 + 0.004 * fr, 0.40 + 0.0005 * fr), (0.8 - 0.004 * fr, 0.52 - 0.0003 * fr))]
        frames.append(np.asarray(d, np.float64))
        times.append(fr / FPS)
    return frames, np.asarray(times)


def test_a_real_tracker_log_followed_while_it_grows():
    from oracle import ocsort_np as oc
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.ocsort import MultiClipTracker
    from vbt_amd.overlay import Overlay, render
    T = 140
    dets, times = crossing_scene(T)
    want_rows = oc.track_boxes(dets, times, asso_func="diou")
    ids = np.asarray(want_rows["id"])
    assert len(np.unique(ids)) >= 2 and max(int((ids == i).sum()) for i in np.unique(ids)) >= 121      # an empty or trivial log must not pass
    mc = MultiClipTracker(1, 4096, max_age=30, asso_func="diou", iou_threshold=0.1)
    frames = noise((T, H, W, 3), 6)
    buf = DeviceBuffer.from_host(frames)
    ov = Overlay(H, W)
    ov.follow(*mc.rows_dev(0), max_frame=T, max_rows_per_frame=25, fps=FPS)
    drawn = 0
    for d, t in zip(dets, times):
        one = np.zeros((1, 1, 25, 6))
        one[0, 0, :len(d)] = d
        mc.update_frames(one, np.array([[len(d)]], np.int32), np.array([[t]]))       # (on the null stream)
        ov.follow_update()
        fr = int(round(t * FPS))
        if fr % 16 == 0:                                                             # frames drawn in batches of 16 while tracking
            ov.draw(buf.ptr + drawn * H * W * 3, fr - drawn, drawn + 1)
            drawn = fr
    ov.draw(buf.ptr + drawn * H * W * 3, T - drawn, drawn + 1)
    n, flags = ov.follow_status()
    got_rows = mc.rows(0)
    assert got_rows["id"] == want_rows["id"] and (n, flags) == (len(ids), 0)
    got = buf.to_host(frames.shape, np.uint8)
    assert_same(got, render(frames, got_rows, FPS))                                  # the two-pass render of the same rows
    assert np.array_equal(got[60], frames[60]) and (got[100] != frames[100]).any()


def test_pipeline_overlay_draw_in_every_tracker_placement(model_path, monkeypatch):
    """one clip, one frame per step, drawn in place four frames at a time through vbt_pipeline_overlay_draw: the tracker inline, on
    its own stream, and with deferred groups - the same bytes, those of the two-pass render"""
    from vbt_amd import _lib, synth
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.overlay import Overlay, render
    from vbt_amd.track import Pipeline
    T, S = 12, 416                                                                   # the clip of test_track_one_pass_writes_the_same_files
    frames = synth.clip_frames(12, 0, T, size=S)
    fb = frames[0].nbytes
    outs = {}
    for mode in ("inline", "own", "defer"):
        monkeypatch.setenv("VBT_TRACKER_STREAM", "own" if mode == "own" else "inline")
        monkeypatch.setenv("VBT_TRACKER_DEFER", "1" if mode == "defer" else "0")
        pipe = Pipeline(model_path, 1, max_frames=T, fps=60.0, detection_treshold=0.3, rows_per_frame=25, depth=2 if mode == "own" else 3)
        assert pipe._trk_inline == (mode != "own") and (pipe._defer > 0) == (mode == "defer")
        buf = DeviceBuffer.from_host(frames)
        ov = Overlay(S, S)
        ov.follow(*pipe.tracker.rows_dev(0), max_frame=T, max_rows_per_frame=25, fps=60.0)
        for t in range(T):
            pipe.step(buf.ptr + t * fb, stream=0, src_hw=(S, S))
            if t % 4 == 3:
                pipe.overlay_draw(ov, buf.ptr + (t - 3) * fb, 4, t - 2, stream=0)
        n, flags = ov.follow_status(0)
        pipe.finish()
        rows = pipe.rows(0)
        assert flags == 0 and n == len(rows["id"]) > 0
        outs[mode] = buf.to_host(frames.shape, np.uint8)
        assert_same(outs[mode], render(frames, rows, 60.0))
        assert (outs[mode] != frames).any()
    assert_same(outs["own"], outs["inline"])
    assert_same(outs["defer"], outs["inline"])


def _track(tmp_path, src, model_path, tag, extra):
    from vbt_amd.cli import main
    out, dfs = tmp_path / ("out" + tag), tmp_path / ("dfs" + tag)
    res = CliRunner().invoke(main, ["track", str(src), "--model", model_path, "--df_dir", str(dfs), "--detection_treshold", "0.3", "--video_dir", str(out)] + extra)
    assert res.exit_code == 0, res.output
    files = os.listdir(dfs)
    assert len(files) == 1, res.output
    return out, dfs / files[0], res.output.replace(str(dfs), "DFS")


@pytest.mark.parametrize("case", ["npy-stride1", "npy-stride3", "npy-mjpeg", "avi-source", "nv12-raw"])
def test_track_one_pass_writes_the_same_files(tmp_path, model_path, case):
    """`track --video_dir --one_pass` against the same command without it: the same video bytes, rows, export name and line.  The clip
    is the recipe of test_gpu_overlay.test_track_video_dir_and_overlay_command, on which the synthetic model gives rows."""
    import pandas as pd
    from vbt_amd import synth
    frames = synth.clip_frames(12, 0, 12, size=416)
    src = tmp_path / "demo.npy"
    np.save(str(src), frames)
    extra = ["--fps", "60", "--time_batch", "5"]                   # 12 frames in batches of 5: three batches, the last one short
    name = "demo.npy"
    if case == "npy-stride3":
        extra += ["--frame_stride", "3"]
    if case in ("npy-mjpeg", "avi-source"):
        extra += ["--video_format", "mjpeg"]
        name = "demo.avi"
    if case == "nv12-raw":                                          # a headerless NV12 file comes back as one: DIR/demo.yuv
        import yuv_ref
        src = tmp_path / "demo.yuv"
        yuv_ref.encode(frames, "nv12").tofile(str(src))
        extra += ["--pix_fmt", "nv12", "--size", "416x416", "--frame_stride", "2"]
        name = "demo.yuv"
    if case == "avi-source":                                        # a Motion-JPEG source from this project's own export
        first, _, _ = _track(tmp_path, src, model_path, "S", extra)
        src = first / "demo.avi"
        extra = ["--time_batch", "5", "--frame_stride", "2"]
        name = "demo.npy"
    two, df2, line2 = _track(tmp_path, src, model_path, "2", extra)
    one, df1, line1 = _track(tmp_path, src, model_path, "1", extra + ["--one_pass"])
    assert (one / name).read_bytes() == (two / name).read_bytes()
    assert df1.name == df2.name and line1 == line2
    a, b = pd.read_pickle(str(df1)), pd.read_pickle(str(df2))
    assert len(a) > 0 and a.equals(b)
    if name.endswith(".npy"):
        got = np.load(str(one / name))
        stride = {"npy-stride3": 3, "avi-source": 2}.get(case, 1)
        assert len(got) == 12 // stride
        if case != "avi-source":
            assert_same(got, R.render(frames, a, 60.0, frame_stride=stride))
            assert (got != frames[stride - 1::stride]).any()


def test_one_pass_with_live_analysis(model_path):
    """track_frames(one_pass=True, live=...) - both follow the same tracker stream - gives the two-pass frames and rows"""
    from vbt_amd import synth
    from vbt_amd.track import track_frames
    frames = synth.clip_frames(12, 0, 12, size=416)
    seen = []
    out1, out2 = np.zeros_like(frames), np.zeros_like(frames)
    d1 = track_frames(frames, model_path, fps=60.0, detection_treshold=0.3, time_batch=5, live=lambda rec, final: seen.append(final), video_out=out1,
                      one_pass=True)
    d2 = track_frames(frames, model_path, fps=60.0, detection_treshold=0.3, time_batch=5, video_out=out2)
    assert d1 == d2 and len(d1["id"]) > 0 and seen == [False, False, False, True]
    assert_same(out1, out2)
