"""Packed 4:2:2, P010 and colour descriptions on the GPU (include/vbt_hip.h, "more source formats"): the fused conversion + resize
kernels against oracle.preprocess.preprocess_image(pixfmt_ref.decode(frame)), clips of every new format through the pipeline against
the same clips as decoded RGB, format and colour changes on a live handle, and the CLI.  Everything is compared bit for bit."""
import ctypes
import itertools
import os

import numpy as np
import pytest
from click.testing import CliRunner

import pixfmt_ref as pr

pytestmark = pytest.mark.gpu

COLS = ("id", "time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width")
GRID = np.array([0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 240, 254, 255])
PACKED = ("yuyv422", "uyvy422")


def _scaled(frames, H, W):
    """nearest-neighbour copy of square frames [T,S,S,3] at H x W"""
    S = frames.shape[1]
    return np.ascontiguousarray(frames[:, (np.arange(H) * S // H)[:, None], (np.arange(W) * S // W)[None, :]])


def _grid_frame(fmt, H, W):
    """The edge values {0,1,15,16,17,127,128,129,234,235,236,240,254,255}^3 laid out as pixels: chroma site k carries the (U, V)
    pair k % 196, the luma samples under the sites of one pair walk through the 14 luma values.  P010: 4 x the value plus an offset
    0..3, random low 6 bits."""
    cy = 1 if fmt in PACKED else 2
    k = np.arange((H // cy) * (W // 2)).reshape(H // cy, W // 2)
    u, v = GRID[k % 14], GRID[(k // 14) % 14]
    ky = k[(np.arange(H) // cy)[:, None], (np.arange(W) // 2)[None, :]]
    sub = (np.arange(H) % cy)[:, None] * 2 + (np.arange(W) % 2)[None, :]
    y = GRID[((ky // 196) * (2 * cy) + sub) % 14]
    if fmt == "p010le":
        y, u, v = 4 * y + (sub & 3), 4 * u + (k & 3), 4 * v + ((k >> 2) & 3)
    f = pr.pack(y, u, v, fmt)
    if fmt == "p010le":
        f = f | np.random.default_rng(H + W).integers(0, 64, f.shape, dtype=np.uint16)
    return f


def _random_frame(fmt, H, W, seed, matrix, rng):
    """uniformly random bytes (16-bit words for P010) whose decoded frame reaches 0 and 255: the first seed that does"""
    from vbt_amd.rawvideo import frame_dtype, frame_shape
    shape, dtype = frame_shape(fmt, H, W), frame_dtype(fmt)
    for s in range(seed, seed + 1000):
        f = np.random.default_rng(s).integers(0, 1 << (8 * dtype.itemsize), shape, dtype=dtype)
        dec = pr.decode(f, fmt, matrix, rng)
        if dec.min() == 0 and dec.max() == 255:
            return f
    raise AssertionError("no random frame clips at both ends")


SMALL = [(2, 2, 3, 3), (6, 8, 5, 7), (7, 8, 4, 4), (18, 34, 7, 5), (320, 320, 320, 320)]
GEOMS = [(fmt, g) for fmt in pr.FMTS for g in SMALL + [(1080, 1920, 320, 320)] if g[0] % 2 == 0 or fmt in PACKED]


# ---- 1. the stand-alone kernels ----
@pytest.mark.parametrize("fmt,geom", GEOMS, ids=[f"{f}-{g[0]}x{g[1]}to{g[2]}x{g[3]}" for f, g in GEOMS])
def test_resize_frames_pix_equals_oracle_on_decoded_rgb(fmt, geom):
    """vbt_resize_frames_pix == preprocess_image(decode(frame)) under every colour description: frame 0 uniformly random (the decoded
    frame reaches 0 and 255: the conversion clips at both ends), frame 1 an encoded synthetic frame, frame 2 the edge grid; host and
    device sources.  The 1080 x 1920 case (long offsets) runs under (bt709, full) with frames 0 and 1."""
    import torch
    from oracle.preprocess import preprocess_image
    from vbt_amd import _lib, synth
    from vbt_amd.rawvideo import colour_codes, pix_fmt_code
    H, W, h, w = geom
    big = H * W > 320 * 320
    L = _lib.lib()
    rgb = _scaled(synth.clip_frames(3, 40, 1), H, W)[0]
    for matrix, rng in ([("bt709", "full")] if big else itertools.product(pr.MATRICES, pr.RANGES)):
        tag = f"{matrix} {rng}"
        frames = [_random_frame(fmt, H, W, H * 7 + W, matrix, rng), pr.encode(rgb, fmt, matrix, rng)] + ([] if big else [_grid_frame(fmt, H, W)])
        src = np.stack(frames)
        B = len(src)
        assert src.nbytes == B * L.vbt_pix_frame_bytes(H, W, pix_fmt_code(fmt))
        if (H, W) == (320, 320):                                           # the whole grid is there, and the identity resize reads all of it
            y, u, v, cy = pr.planes(src[2], fmt)
            up = lambda p: np.repeat(np.repeat(p, cy, axis=-2), 2, axis=-1)
            sh = 2 if fmt == "p010le" else 0
            assert len(np.unique(((y >> sh).astype(np.int64) << 16 | (up(u) >> sh).astype(np.int64) << 8 | (up(v) >> sh)).ravel())) == 14 ** 3
        want = np.concatenate([preprocess_image(pr.decode(f, fmt, matrix, rng), (h, w)) for f in src])
        assert want.shape == (B, h, w, 3)
        if H >= 18:
            assert want[1].std() > 10, tag
        m, r = colour_codes(matrix, rng)
        got = np.full((B, h, w, 3), 7, np.uint8)
        _lib.check(L.vbt_resize_frames_pix(src.ctypes.data, B, H, W, pix_fmt_code(fmt), m, r, 0, got.ctypes.data, h, w, 0, 0, None))
        assert np.array_equal(got, want), f"host source, {tag}"
        sd = torch.from_numpy(src.view(np.uint8)).cuda()
        dd = torch.full((B, h, w, 3), 9, dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(L.vbt_resize_frames_pix(sd.data_ptr(), B, H, W, pix_fmt_code(fmt), m, r, 1, dd.data_ptr(), h, w, 1, 0, st))
        torch.cuda.synchronize()
        assert np.array_equal(dd.cpu().numpy(), want), f"device source, {tag}"


def test_default_description_gives_what_resize_frames_yuv_gives():
    """nv12 / i420 under (bt601, limited) through the new entry point are the older entry point's bytes; yuyv422 decodes as nv12 does"""
    from vbt_amd import _lib
    L = _lib.lib()
    H, W, n = 18, 34, 7
    rng = np.random.default_rng(3)
    for fmt, code in (("nv12", 1), ("i420", 2)):
        src = rng.integers(0, 256, (2, H * 3 // 2, W), dtype=np.uint8)
        a, b = np.zeros((2, n, n, 3), np.uint8), np.ones((2, n, n, 3), np.uint8)
        _lib.check(L.vbt_resize_frames_yuv(src.ctypes.data, 2, H, W, code, 0, a.ctypes.data, n, n, 0, 0, None))
        _lib.check(L.vbt_resize_frames_pix(src.ctypes.data, 2, H, W, code, 0, 0, 0, b.ctypes.data, n, n, 0, 0, None))
        assert np.array_equal(a, b), fmt
        # the same samples as yuyv422 / uyvy422, every chroma row written twice: the 8-bit constants hold for every 8-bit format
        y, u, v, _ = pr.planes(src, fmt)
        for packed, pcode in (("yuyv422", 16), ("uyvy422", 17)):
            src2 = np.ascontiguousarray(pr.pack(y, np.repeat(u, 2, axis=-2), np.repeat(v, 2, axis=-2), packed))
            c = np.full((2, n, n, 3), 2, np.uint8)
            _lib.check(L.vbt_resize_frames_pix(src2.ctypes.data, 2, H, W, pcode, 0, 0, 0, c.ctypes.data, n, n, 0, 0, None))
            assert np.array_equal(c, a), (fmt, packed)


@pytest.mark.parametrize("H,W", [(2, 16386), (16386, 8)], ids=["2x16386", "16386x8"])
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_pipeline_takes_420_sources_above_16384_as_before(model_path, fmt, H, W):
    """NV12 / I420 sources of the pipeline have no upper size limit (the limit belongs to the 4:2:2 formats and P010): a strip with a
    side of 16386 steps, host-fed and device-resident, under both descriptions, and gives the detections of its decoded RGB frames."""
    import torch
    from vbt_amd.track import Pipeline
    src = np.random.default_rng(H).integers(0, 256, (2, H * 3 // 2, W), dtype=np.uint8)
    pipe = Pipeline(model_path, 2, max_frames=8, fps=30.0, rows_per_frame=25)
    for colour in (("bt601", "limited"), ("bt709", "full")):
        pipe.set_pixel_format("rgb24")
        pipe.step(pr.decode(src, fmt, *colour), src_hw=(H, W))
        want = pipe.detections()
        pipe.set_pixel_format(fmt)
        pipe.set_colour(*colour)
        for frames in (src, torch.from_numpy(src).cuda()):
            n0 = pipe.info().steps_enqueued
            pipe.step(frames, src_hw=(H, W))
            assert pipe.info().steps_enqueued == n0 + 1
            assert all(np.array_equal(a, b) for a, b in zip(pipe.detections(), want)), colour
    pipe.finish()


# ---- 2. pipeline equivalence ----
def _rows_equal(a, b):
    return a["id"] == b["id"] and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in COLS[1:])


def _dets_equal(a, b):
    return len(a) == len(b) and all(all(np.array_equal(x, y) for x, y in zip(da, db)) for da, db in zip(a, b))


def _phases_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


T, SPEED, R, LEAD = 72, 3, 16, 8                     # one squat rep takes 198 / SPEED frames of the synthetic clip
SEED, WIDTH = 4242, 322                              # a clip on which the RGB runs find the plates and a phase at every geometry below
STEPS = len(range(0, T - LEAD - R + 1, R))
_PIPES = {}
_CLIP = {}


def _pipes(model_path):
    if not _PIPES:
        from vbt_amd.track import Pipeline
        fps = 60.0 / SPEED
        _PIPES["one"] = Pipeline(model_path, 32, max_frames=T, fps=fps, rows_per_frame=25, tracker_clips=1)      # vbt_track_clip follows one clip
        _PIPES["runs"] = Pipeline(model_path, 32, max_frames=T, fps=fps, rows_per_frame=25, tracker_clips=2)
    return _PIPES["one"], _PIPES["runs"]


def _samples_320(fmt, matrix, rng):
    """the synthetic clip at its own 320 x 320 as encoder samples; computed once per (chroma layout, depth, colour description)"""
    from vbt_amd import synth
    key = (fmt in PACKED, pr.depth(fmt), matrix, rng)
    if key not in _CLIP:
        bg = synth.background(SEED)
        _CLIP[key] = pr.samples(np.stack([synth.render(bg, SPEED * t) for t in range(T)]), fmt, matrix, rng)
    return _CLIP[key]


def _clip(fmt, matrix, rng, H, W):
    """the clip at H x W in format fmt: the 320 x 320 samples, each plane repeated nearest"""
    y, u, v = _samples_320(fmt, matrix, rng)
    cy = 1 if fmt in PACKED else 2
    near = lambda p, n_out: np.arange(n_out) * p // n_out
    big = lambda p, h_, w_: p[:, near(p.shape[1], h_)[:, None], near(p.shape[2], w_)[None, :]]
    return np.ascontiguousarray(pr.pack(big(y, H, W), big(u, H // cy, W // 2), big(v, H // cy, W // 2), fmt))


def _run_clip(one, pipe, clip, fmt, colour, hw, on_device):
    """track_clip, then the same clip as two staggered clips through step_runs with one source per run (16 frames each, the second
    clip 8 frames ahead).  Returns rows / phases / per-step detections and the bytes uploaded."""
    import torch
    for p in (one, pipe):
        p.set_pixel_format(fmt)
        p.set_colour(*colour)
    src = torch.from_numpy(clip.view(np.int16) if clip.dtype == np.uint16 else clip).cuda() if on_device else clip
    up0 = one.info().h2d_bytes
    out = {"track_clip": one.track_clip(src, src_hw=hw)}
    out["track_clip_phases"] = one.phases(0)
    out["track_clip_h2d"] = int(one.info().h2d_bytes - up0)
    one.reset()
    dets = []
    up0 = pipe.info().h2d_bytes
    for t0 in range(0, T - LEAD - R + 1, R):
        pipe.step_runs([src[t0:t0 + R], src[t0 + LEAD:t0 + LEAD + R]], [(0, 0, R, t0 + 1), (1, R, R, t0 + 1)], src_hw=hw)
        dets.append(pipe.detections())
    out["runs_h2d"] = int(pipe.info().h2d_bytes - up0)
    pipe.finish()
    out["runs_dets"] = dets
    out["runs_rows"] = [pipe.rows(c) for c in range(2)]
    out["runs_phases"] = [pipe.phases(c) for c in range(2)]
    pipe.reset()
    return out


def _compact_bytes(fmt, H, W, size=320):
    """bytes of one host-fed frame as the layouts of the compact upload imply (include/vbt_hip.h, vbt_pipeline_set_pixel_format)"""
    from oracle.preprocess import _axis
    row = {"nv12": W, "i420": W, "p010le": 2 * W, "yuyv422": 2 * W, "uyvy422": 2 * W}[fmt]
    if fmt in PACKED:
        return 2 * size * row                                                        # the row pairs, every row with its own chroma
    p_last = min(int(_axis(size, H)[0][-1]), H - 2)
    return 2 * (size - 1) * row + (H - p_last) * row + H // 2 * row                      # pairs 0..size-2, rows p_last.., the chroma plane whole


VARIANTS = [("yuyv422", "bt601", "limited"), ("uyvy422", "bt709", "limited"), ("p010le", "bt709", "full"), ("nv12", "bt709", "full")]


@pytest.mark.parametrize("compact", [True, False], ids=["row_pairs", "whole_frames"])
@pytest.mark.parametrize("fmt,matrix,rng", VARIANTS, ids=["-".join(v) for v in VARIANTS])
def test_pipeline_clip_equals_decoded_rgb_clip(model_path, fmt, matrix, rng, compact):
    """A clip of a new format (or of nv12 under bt709 / full) gives the detections, rows and phases of the RGB clip decoded from it,
    host-fed and device-resident, and uploads the bytes its layout implies.  compact_rows (pipeline_ingest.hip) uploads row pairs when
    2 * 320 < H: 642 rows is the smallest such even height (643 for 4:2:2, which takes odd heights), 640 the largest that uploads whole
    frames.  322 columns keep the clip close to the synthetic one (the detector finds its plates) and make the frames of 642 and 643
    rows no multiple of 16 bytes: device-resident runs are then assembled by one copy per run, those of 640 rows by the gather kernel."""
    H = (643 if fmt in PACKED else 642) if compact else 640
    W = WIDTH
    assert (H * W * (6 if fmt == "p010le" else 4 if fmt in PACKED else 3) // 2 % 16 != 0) == compact
    one, pipe = _pipes(model_path)
    clip = _clip(fmt, matrix, rng, H, W)
    dec = pr.decode(clip, fmt, matrix, rng)
    assert dec.shape == (T, H, W, 3)
    want = _run_clip(one, pipe, dec, "rgb24", (matrix, rng), (H, W), False)     # (the colour description is kept but not read for rgb24)
    # not vacuous: the RGB run tracks the plates and finds at least one phase
    assert len(want["track_clip"]["id"]) > 0 and len(want["track_clip_phases"][1]) >= 1
    assert all(len(r["id"]) > 0 for r in want["runs_rows"]) and any(int(d[3].sum()) > 0 for d in want["runs_dets"])
    assert want["track_clip_h2d"] == T * (2 * 320 if compact else H) * W * 3
    fb = _compact_bytes(fmt, H, W) if compact else clip[0].nbytes
    for on_device in (False, True):
        got = _run_clip(one, pipe, clip, fmt, (matrix, rng), (H, W), on_device)
        assert _rows_equal(got["track_clip"], want["track_clip"]), on_device
        assert _phases_equal(got["track_clip_phases"], want["track_clip_phases"]), on_device
        assert _dets_equal(got["runs_dets"], want["runs_dets"]), on_device
        for c in range(2):
            assert _rows_equal(got["runs_rows"][c], want["runs_rows"][c]), (on_device, c)
            assert _phases_equal(got["runs_phases"][c], want["runs_phases"][c]), (on_device, c)
        print(f"{fmt} {H}x{W} on_device={on_device}: track_clip {got['track_clip_h2d']} bytes, runs {got['runs_h2d']} bytes, rgb {want['track_clip_h2d']}")
        assert got["track_clip_h2d"] == (0 if on_device else T * fb), on_device
        assert got["runs_h2d"] == (0 if on_device else STEPS * 2 * R * fb), on_device


# ---- 3. format and colour changes between steps, refusals on a live handle ----
def test_format_and_colour_changes_between_steps(model_path):
    import torch
    from vbt_amd import _lib, synth
    from vbt_amd.track import Pipeline
    L = _lib.lib()
    N, S = 24, 320
    rgb = synth.clip_frames(9, 0, N)
    # frames 0..7 nv12 under the default description, 8..15 yuyv422 under bt709 / limited, 16..23 p010le under bt601 / full, then rgb24
    segs = [("nv12", ("bt601", "limited"), 0, 8), ("yuyv422", ("bt709", "limited"), 8, 16), ("p010le", ("bt601", "full"), 16, 20),
            ("rgb24", ("bt601", "full"), 20, 24)]
    enc = [rgb[a:b] if fmt == "rgb24" else pr.encode(rgb[a:b], fmt, *col) for fmt, col, a, b in segs]
    dec = np.concatenate([e if fmt == "rgb24" else pr.decode(e, fmt, *col) for e, (fmt, col, a, b) in zip(enc, segs)])
    st = torch.cuda.current_stream().cuda_stream

    def dev(a):
        return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()

    fresh = Pipeline(model_path, 1, max_frames=N, fps=30.0, rows_per_frame=25)
    dd = dev(dec)
    want_dets = []
    for t in range(N):
        fresh.step(dd[t:t + 1])
        want_dets.append(fresh.detections())
    fresh.finish()
    want = fresh.rows(0)
    assert len(want["id"]) > 0 and any(int(d[3].sum()) > 0 for d in want_dets)

    def refusals(pipe, frame):
        before = (pipe.info().steps_enqueued, pipe.info().frame_count, pipe.info().h2d_bytes)
        with pytest.raises(ValueError):
            pipe.set_colour("bt2020", "limited")
        with pytest.raises(ValueError):
            pipe.set_colour("bt709", "tv")
        assert L.vbt_pipeline_set_colour(pipe._h, 2, 0) == -1 and "matrix" in L.vbt_last_error().decode()
        assert L.vbt_pipeline_set_colour(pipe._h, 0, -1) == -1 and "range" in L.vbt_last_error().decode()
        for code in (3, 15, 19):
            assert L.vbt_pipeline_set_pixel_format(pipe._h, code) == -1 and "unknown" in L.vbt_last_error().decode()
        args = lambda ptr, h, w, swap: (pipe._h, ptr, 1, h, w, swap, None, None, None, 1, st)
        ptr = frame.data_ptr()
        if pipe.pix_fmt != "rgb24":
            assert L.vbt_pipeline_step(*args(ptr, S, S, 1)) == -1 and "swap_rb" in L.vbt_last_error().decode()
            assert L.vbt_pipeline_step(*args(ptr, 0, 0, 0)) == -1
            assert L.vbt_pipeline_step(*args(ptr, S, S - 1, 0)) == -1 and "src_w" in L.vbt_last_error().decode()
            with pytest.raises(ValueError):
                pipe.step(frame, src_hw=(S, S - 1))
        if pipe.pix_fmt == "p010le":
            assert L.vbt_pipeline_step(*args(ptr, S - 1, S, 0)) == -1 and "src_h" in L.vbt_last_error().decode()
        if pipe.pix_fmt in ("yuyv422", "p010le"):
            assert L.vbt_pipeline_step(*args(ptr, S, 16386, 0)) == -1
            assert L.vbt_pipeline_step(*args(ptr + 2, S, S, 0)) == -1 and "aligned" in L.vbt_last_error().decode()
            run1 = (_lib.Run * 1)(_lib.Run(0, 0, 1, 1, 1, 1, 30.0))
            srcs = (ctypes.c_void_p * 1)(ptr + 1)
            assert L.vbt_pipeline_step_runs(pipe._h, None, srcs, 1, run1, 1, S, S, 0, 1, None, None, None, None, st) == -1
            assert "aligned" in L.vbt_last_error().decode()
        assert (pipe.info().steps_enqueued, pipe.info().frame_count, pipe.info().h2d_bytes) == before

    for on_device in (True, False):
        pipe = Pipeline(model_path, 1, max_frames=N, fps=30.0, rows_per_frame=25)
        dets = []
        for e, (fmt, col, a, b) in zip(enc, segs):
            pipe.set_pixel_format(fmt)
            pipe.set_colour(*col)
            src = dev(e) if on_device else e
            for t in range(b - a):
                if t == 1:
                    refusals(pipe, dev(e)[t:t + 1])
                pipe.step(src[t:t + 1], src_hw=None if fmt == "rgb24" else (S, S))
                dets.append(pipe.detections())
        pipe.finish()
        assert _dets_equal(dets, want_dets), on_device
        assert _rows_equal(pipe.rows(0), want), on_device


# ---- 4. CLI ----
def test_cli_tracks_a_raw_uyvy_file_like_the_decoded_npy(tmp_path, model_path):
    import pandas as pd
    from vbt_amd import synth
    from vbt_amd.cli import main
    H = W = 416
    yuv = pr.encode(synth.clip_frames(12, 0, 12, size=416), "uyvy422", "bt709", "limited")
    assert yuv.shape == (12, H, 2 * W)
    for name in ("clip", "other"):
        yuv.tofile(str(tmp_path / f"{name}.yuv"))
        np.save(str(tmp_path / f"{name}.npy"), pr.decode(yuv, "uyvy422", "bt709", "limited"))
    common = ["--model", model_path, "--fps", "60", "--detection_treshold", "0.3"]
    raw = ["--pix_fmt", "uyvy422", "--size", f"{W}x{H}", "--color_matrix", "bt709"]

    def frames_of(out):
        return {f.split("_id")[0]: (f, pd.read_pickle(os.path.join(out, f))) for f in sorted(os.listdir(out))}

    res = CliRunner().invoke(main, ["track", str(tmp_path / "clip.npy"), str(tmp_path / "other.npy"), "--df_dir", str(tmp_path / "df_npy")] + common)
    assert res.exit_code == 0, res.output
    want = frames_of(tmp_path / "df_npy")
    assert sorted(want) == ["clip", "other"] and all(len(df) > 0 for _, df in want.values())
    res = CliRunner().invoke(main, ["track", str(tmp_path / "clip.yuv"), "--df_dir", str(tmp_path / "df_raw")] + common + raw)
    assert res.exit_code == 0, res.output
    got = frames_of(tmp_path / "df_raw")
    assert list(got) == ["clip"] and got["clip"][0] == want["clip"][0]
    pd.testing.assert_frame_equal(got["clip"][1], want["clip"][1], check_exact=True)
    res = CliRunner().invoke(main, ["track", str(tmp_path / "clip.yuv"), str(tmp_path / "other.yuv"), "--concurrent", "2", "--df_dir",
                                    str(tmp_path / "df_two")] + common + raw)
    assert res.exit_code == 0, res.output
    got = frames_of(tmp_path / "df_two")
    assert sorted(got) == ["clip", "other"]
    for name in got:
        assert got[name][0] == want[name][0]
        pd.testing.assert_frame_equal(got[name][1], want[name][1], check_exact=True)
    # --live reads the same file
    res = CliRunner().invoke(main, ["track", str(tmp_path / "clip.yuv"), "--live"] + common + raw)
    assert res.exit_code == 0 and f"{len(want['clip'][1])} rows" in res.output, res.output
