"""YUV 4:2:0 ingest on the GPU (include/vbt_hip.h, "pixel formats"): the fused conversion + resize kernel against
oracle.preprocess.preprocess_image(yuv_ref.rgb_from_*(frame)), and NV12 / I420 clips through the pipeline, the C ABI's refusals and
the CLI against the same clips as decoded RGB.  Everything is compared bit for bit."""
import ctypes
import os

import numpy as np
import pytest
from click.testing import CliRunner

import yuv_ref

pytestmark = pytest.mark.gpu

FMTS = ("nv12", "i420")
COLS = ("id", "time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width")


def _scaled(frames, H, W):
    """nearest-neighbour copy of square synthetic frames [T,S,S,3] at H x W"""
    S = frames.shape[1]
    return np.ascontiguousarray(frames[:, (np.arange(H) * S // H)[:, None], (np.arange(W) * S // W)[None, :]])


def _synth_clip(seed, T, H, W, speed=3):
    """A synthetic clip at H x W whose plates move `speed` times as fast as synth's (one squat rep in 198 / speed frames)."""
    from vbt_amd import synth
    bg = synth.background(seed)
    return _scaled(np.stack([synth.render(bg, speed * t) for t in range(T)]), H, W)


# ---- 1. the stand-alone kernel ----
@pytest.mark.parametrize("geom", [(1080, 1920, 320), (720, 1280, 320), (480, 640, 320), (6, 8, 320), (320, 320, 320),
                                  (1080, 1920, 448), (6, 8, 448), (448, 448, 448)], ids=lambda g: f"{g[0]}x{g[1]}to{g[2]}")
@pytest.mark.parametrize("fmt", FMTS)
def test_resize_frames_yuv_equals_oracle_on_decoded_rgb(geom, fmt):
    """vbt_resize_frames_yuv == preprocess_image(rgb_from_yuv(frame)): frame 0 is uniformly random bytes (conversion clips at both
    ends, chroma changes at every sample), frame 1 an encoded synthetic frame; host and device sources."""
    import torch
    from oracle.preprocess import preprocess_image
    from vbt_amd import _lib, synth
    from vbt_amd.rawvideo import pix_fmt_code
    H, W, n = geom
    rng = np.random.default_rng(H * 7 + W + n)
    src = np.stack([rng.integers(0, 256, (H * 3 // 2, W), dtype=np.uint8),
                    yuv_ref.encode(_scaled(synth.clip_frames(3, 40, 1), H, W)[0], fmt)])
    want = np.concatenate([preprocess_image(yuv_ref.rgb_from_yuv(f, fmt), (n, n)) for f in src])
    dec0 = yuv_ref.rgb_from_yuv(src[0], fmt)
    assert want.shape == (2, n, n, 3) and dec0.min() == 0 and dec0.max() == 255 and want[1].std() > 10     # clipping is exercised
    L = _lib.lib()
    got = np.full((2, n, n, 3), 7, np.uint8)
    _lib.check(L.vbt_resize_frames_yuv(src.ctypes.data, 2, H, W, pix_fmt_code(fmt), 0, got.ctypes.data, n, n, 0, 0, None))
    assert np.array_equal(got, want), "host source"
    sd = torch.from_numpy(src).cuda()
    dd = torch.full((2, n, n, 3), 9, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.vbt_resize_frames_yuv(sd.data_ptr(), 2, H, W, pix_fmt_code(fmt), 1, dd.data_ptr(), n, n, 1, 0, st))
    torch.cuda.synchronize()
    assert np.array_equal(dd.cpu().numpy(), want), "device source"


# ---- 2. / 3. pipeline equivalence ----
def _rows_equal(a, b):
    return a["id"] == b["id"] and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in COLS[1:])


def _dets_equal(a, b):
    return len(a) == len(b) and all(all(np.array_equal(x, y) for x, y in zip(da, db)) for da, db in zip(a, b))


def _run_clip(one, pipe, clip, fmt, hw, on_device):
    """track_clip, then the same clip as two staggered clips through step_runs with one source per run (16 frames each, the second
    clip 8 frames ahead).  Returns rows / phases / per-step detections and the bytes uploaded."""
    import torch
    one.set_pixel_format(fmt)
    pipe.set_pixel_format(fmt)
    src = torch.from_numpy(clip).cuda() if on_device else clip
    up0 = one.info().h2d_bytes
    out = {"track_clip": one.track_clip(src, src_hw=hw)}
    out["track_clip_phases"] = one.phases(0)
    out["track_clip_h2d"] = int(one.info().h2d_bytes - up0)
    one.reset()
    T, R, lead = len(clip), 16, 8
    dets = []
    up0 = pipe.info().h2d_bytes
    for t0 in range(0, T - lead - R + 1, R):
        pipe.step_runs([src[t0:t0 + R], src[t0 + lead:t0 + lead + R]], [(0, 0, R, t0 + 1), (1, R, R, t0 + 1)], src_hw=hw)
        dets.append(pipe.detections())
    out["runs_h2d"] = int(pipe.info().h2d_bytes - up0)
    pipe.finish()
    out["runs_dets"] = dets
    out["runs_rows"] = [pipe.rows(c) for c in range(2)]
    out["runs_phases"] = [pipe.phases(c) for c in range(2)]
    pipe.reset()
    return out


_CASES = {}


def _case(model_path, name):
    """One geometry: the clip encoded to NV12 and I420, each decoded with the reference, and every variant through one pipeline."""
    if name in _CASES:
        return _CASES[name]
    from vbt_amd.track import Pipeline
    # (seed, speed, T): clips on which the detector + tracker find the plates and at least one phase at that geometry (72 frames at
    # three times synth's speed keep the 1080-row clip small; the others take 104 frames at twice the speed)
    H, W, on_device, seed, speed, T = {"host_1080x1920_compact": (1080, 1920, False, 31, 3, 72), "host_480x640": (480, 640, False, 4242, 2, 104),
                                       "host_1920x1080_integer_scale": (1920, 1080, False, 4242, 3, 72),
                                       "device_480x640": (480, 640, True, 4242, 2, 104),
                                       "device_322x322_gather_fallback": (322, 322, True, 4242, 2, 104)}[name]
    rgb = _synth_clip(seed, T, H, W, speed)
    fps = 60.0 / speed
    one = Pipeline(model_path, 32, max_frames=T, fps=fps, rows_per_frame=25, tracker_clips=1)      # vbt_track_clip follows one clip
    pipe = Pipeline(model_path, 32, max_frames=T, fps=fps, rows_per_frame=25, tracker_clips=2)
    res = {}
    for fmt in FMTS:
        yuv = yuv_ref.encode(rgb, fmt)
        assert yuv.shape == (T, H * 3 // 2, W)
        dec = yuv_ref.rgb_from_yuv(yuv, fmt)
        res[fmt] = (_run_clip(one, pipe, dec, "rgb24", (H, W), on_device), _run_clip(one, pipe, yuv, fmt, (H, W), on_device))
    _CASES[name] = res
    return res


def _phases_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", ["host_1080x1920_compact", "host_1920x1080_integer_scale", "host_480x640", "device_480x640", "device_322x322_gather_fallback"])
def test_pipeline_yuv_clip_equals_decoded_rgb_clip(model_path, name):
    """An NV12 / I420 clip gives the detections, rows and phases of the RGB clip the reference decodes from it: host-fed with the
    compact upload (1080 rows -> 320: a row table; 1920 rows -> 320: pairs at one pitch, one strided copy per frame), host-fed whole frames, device-fed through the gather kernel, and device-fed with a frame
    of 322 * 322 * 3 / 2 bytes - not a multiple of 16, so the batch is assembled by one copy per run."""
    assert (322 * 322 * 3 // 2) % 16 != 0 and (480 * 640 * 3 // 2) % 16 == 0
    for fmt, (want, got) in _case(model_path, name).items():
        # not vacuous: the RGB run tracks the plates and finds at least one phase
        assert len(want["track_clip"]["id"]) > 0 and len(want["track_clip_phases"][1]) >= 1, fmt
        assert all(len(r["id"]) > 0 for r in want["runs_rows"]) and any(int(d[3].sum()) > 0 for d in want["runs_dets"]), fmt
        assert _rows_equal(got["track_clip"], want["track_clip"]), fmt
        assert _phases_equal(got["track_clip_phases"], want["track_clip_phases"]), fmt
        assert _dets_equal(got["runs_dets"], want["runs_dets"]), fmt
        for c in range(2):
            assert _rows_equal(got["runs_rows"][c], want["runs_rows"][c]), (fmt, c)
            assert _phases_equal(got["runs_phases"][c], want["runs_phases"][c]), (fmt, c)


def test_compact_yuv_upload_moves_at_most_two_thirds_of_the_rgb_bytes(model_path):
    """1080x1920 host-fed: luma row pairs + the chroma planes against the RGB row pairs of the same steps
    ((2 * 320 + 540 + 1) / (6 * 320) = 0.615: one luma row below the last pair travels with the chroma)."""
    for fmt, (want, got) in _case(model_path, "host_1080x1920_compact").items():
        for key, frames in (("track_clip_h2d", 72), ("runs_h2d", 4 * 32)):
            assert want[key] == frames * 2 * 320 * 1920 * 3, (fmt, key)               # the RGB row-pair upload, as before
            print(f"{fmt} {key}: yuv {got[key]} bytes, rgb {want[key]} bytes, ratio {got[key] / want[key]:.4f}")
            assert 0 < got[key] <= want[key] * 2 // 3, (fmt, key)
            assert got[key] == frames * (2 * 319 * 1920 + (1080 - 1077) * 1920 + 1080 * 1920 // 2), (fmt, key)   # pairs 0..318, rows 1077.., chroma
    # 1920 rows -> 320 (portrait): the chroma planes are 960 W against 640 W of luma pairs - 0.834 of the RGB bytes, counted exactly
    for fmt, (want, got) in _case(model_path, "host_1920x1080_integer_scale").items():
        for key, frames in (("track_clip_h2d", 72), ("runs_h2d", 4 * 32)):
            assert want[key] == frames * 2 * 320 * 1080 * 3, (fmt, key)
            assert got[key] == frames * (2 * 319 * 1080 + (1920 - 1916) * 1080 + 1920 * 1080 // 2), (fmt, key)
    # whole frames where the source is not more than twice as tall as the network input: exactly half the RGB bytes
    for fmt, (want, got) in _case(model_path, "host_480x640").items():
        assert want["track_clip_h2d"] == 104 * 480 * 640 * 3 and got["track_clip_h2d"] == 104 * 480 * 640 * 3 // 2, fmt


# ---- 4. refusals on a live pipeline ----
def test_refusals_leave_the_pipeline_untouched_and_rgb24_restores(model_path):
    import torch
    from vbt_amd import _lib, synth
    from vbt_amd.track import Pipeline
    L = _lib.lib()
    T, S = 24, 320
    rgb = synth.clip_frames(9, 0, T)
    yuv = yuv_ref.encode(rgb, "nv12")                        # source at the network resolution: conversion only
    dec = yuv_ref.rgb_from_nv12(yuv)
    yd = torch.from_numpy(yuv).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def run(pipe, refuse):
        pipe.reset()
        pipe.set_pixel_format("nv12")
        for t in range(T):
            if refuse and t in (0, 5, 11):
                before = (pipe.info().steps_enqueued, pipe.info().frame_count, pipe.info().h2d_bytes)
                args = lambda h, w, swap: (pipe._h, yd[t:t + 1].data_ptr(), 1, h, w, swap, None, None, None, 1, st)
                assert L.vbt_pipeline_step(*args(S, S, 1)) == -1 and "swap_rb" in L.vbt_last_error().decode()
                assert L.vbt_pipeline_step(*args(0, 0, 0)) == -1
                assert L.vbt_pipeline_step(*args(S, S - 1, 0)) == -1
                run1 = (_lib.Run * 1)(_lib.Run(0, 0, 1, 1, t + 1, 1, 30.0))
                rargs = lambda h, w, swap: (pipe._h, yd[t:t + 1].data_ptr(), None, 1, run1, 1, h, w, swap, 1, None, None, None, None, st)
                assert L.vbt_pipeline_step_runs(*rargs(S, S, 1)) == -1
                assert L.vbt_pipeline_step_runs(*rargs(0, 0, 0)) == -1
                assert L.vbt_pipeline_step_runs(*rargs(S, S + 1, 0)) == -1
                with pytest.raises(ValueError):
                    pipe.step(yd[t:t + 1], src_hw=(S, S), swap_rb=True)
                with pytest.raises(ValueError):
                    pipe.step(yd[t:t + 1])
                assert (pipe.info().steps_enqueued, pipe.info().frame_count, pipe.info().h2d_bytes) == before
            pipe.step(yd[t:t + 1], src_hw=(S, S))
        pipe.finish()
        return pipe.rows(0)

    pipe = Pipeline(model_path, 1, max_frames=T, fps=30.0, rows_per_frame=25)
    clean = run(pipe, False)
    assert len(clean["id"]) > 0
    assert _rows_equal(run(pipe, True), clean)
    # track_clip refuses the same way (before its reset) ...
    ids, cols, n = np.empty(64, np.int64), np.empty((64, 7)), ctypes.c_int()
    one = Pipeline(model_path, 8, max_frames=T, fps=30.0, rows_per_frame=25, tracker_clips=1)
    one.set_pixel_format("nv12")
    for h, w, swap in ((S, S, 1), (0, 0, 0), (S, S - 1, 0)):
        assert L.vbt_track_clip(one._h, yuv.ctypes.data, 0, T, h, w, swap, 1, ids.ctypes.data, cols.ctypes.data, 64, ctypes.byref(n)) == -1
    assert L.vbt_pipeline_set_pixel_format(one._h, 3) == -1 and one.track_clip(yuv, src_hw=(S, S)) == clean
    # ... and back at RGB24 the pipeline takes packed frames as a pipeline that never left it does
    pipe.reset()
    pipe.set_pixel_format("rgb24")
    dd = torch.from_numpy(dec).cuda()
    for t in range(T):
        pipe.step(dd[t:t + 1])
    pipe.finish()
    assert _rows_equal(pipe.rows(0), clean)
    fresh = Pipeline(model_path, 1, max_frames=T, fps=30.0, rows_per_frame=25)
    for t in range(T):
        fresh.step(dd[t:t + 1])
    fresh.finish()
    assert _rows_equal(fresh.rows(0), clean)


# ---- 5. CLI ----
@pytest.mark.parametrize("fmt", FMTS)
def test_cli_tracks_a_raw_yuv_file_like_the_decoded_npy(tmp_path, model_path, fmt):
    import pandas as pd
    from vbt_amd import synth
    from vbt_amd.cli import main
    H = W = 416
    yuv = yuv_ref.encode(synth.clip_frames(12, 0, 12, size=416), fmt)
    raw, npy = tmp_path / "clip.yuv", tmp_path / "clip.npy"
    yuv.tofile(str(raw))
    np.save(str(npy), yuv_ref.rgb_from_yuv(yuv, fmt))
    common = ["--model", model_path, "--fps", "60", "--detection_treshold", "0.3"]
    dfs = []
    for src, extra in ((npy, []), (raw, ["--pix_fmt", fmt, "--size", f"{W}x{H}"])):
        out = tmp_path / ("df_" + src.suffix[1:])
        res = CliRunner().invoke(main, ["track", str(src), "--df_dir", str(out)] + common + extra)
        assert res.exit_code == 0, res.output
        files = os.listdir(out)
        assert len(files) == 1 and files[0].startswith("clip_id"), files
        dfs.append((files[0], pd.read_pickle(os.path.join(out, files[0]))))
    assert dfs[0][0] == dfs[1][0] and len(dfs[0][1]) > 0
    pd.testing.assert_frame_equal(dfs[1][1], dfs[0][1], check_exact=True)
    # --live and --concurrent read the same file
    res = CliRunner().invoke(main, ["track", str(raw), "--live", "--pix_fmt", fmt, "--size", f"{W}x{H}"] + common)
    assert res.exit_code == 0 and f"{len(dfs[0][1])} rows" in res.output, res.output
    res = CliRunner().invoke(main, ["track", str(raw), str(raw), "--concurrent", "2", "--pix_fmt", fmt, "--size", f"{W}x{H}"] + common)
    assert res.exit_code == 0 and res.output.count(f"{len(dfs[0][1])} rows") == 2, res.output
