"""Packed 4:2:2, P010 and colour descriptions without a GPU: the numpy statement of the contract (tests/pixfmt_ref.py) against the
header's table and the older 4:2:0 reference, the sizes of frames as rawvideo.py and the library see them, and every refusal that is
made before any device call - through the C ABI and through `cli track`."""
import itertools

import numpy as np
import pytest
from click.testing import CliRunner

import pixfmt_ref as pr
import yuv_ref

CODES = {"rgb24": 0, "nv12": 1, "i420": 2, "yuyv422": 16, "uyvy422": 17, "p010le": 18}


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib
    return _lib, _lib.lib()


def test_coefficient_table_is_the_derivation():
    for (matrix, bits, rng), row in pr.TABLE.items():
        if (matrix, bits, rng) == ("bt601", 8, "limited"):
            # today's constants, rounded from three decimals: kept, and close to the derivation
            assert row == (1220542, 1673527, 409993, 852492, 2116026)
            assert max(abs(a - b) / b for a, b in zip(row, pr.derive(matrix, bits, rng))) < 2e-3
        else:
            assert row == pr.derive(matrix, bits, rng), (matrix, bits, rng)
    assert len(pr.TABLE) == 8
    # int32 holds the largest intermediate of every row
    for (matrix, bits, rng), (cy, crv, cgu, cgv, cbu) in pr.TABLE.items():
        top, half = (1 << bits) - 1, 1 << (bits - 1)
        assert cy * top + max(crv, cbu, cgu + cgv) * half + (1 << 19) < 2 ** 31


def test_colour_codes_and_format_codes():
    from vbt_amd import rawvideo as rv
    assert rv.PIX_FMTS == CODES
    assert [rv.colour_codes(m, r) for m in pr.MATRICES for r in pr.RANGES] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert rv.colour_codes() == (0, 0) and rv.colour_codes("BT709", "Full") == (1, 1)
    for bad in (("bt2020", "limited"), ("bt601", "tv")):
        with pytest.raises(ValueError):
            rv.colour_codes(*bad)
    assert all(rv.is_yuv(f) for f in pr.FMTS) and not rv.is_yuv("rgb24")
    with pytest.raises(ValueError):
        rv.pix_fmt_code("yuyv")


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_default_description_decodes_420_as_before(fmt):
    rng = np.random.default_rng(5)
    f = rng.integers(0, 256, (2, 18 * 3 // 2, 34), dtype=np.uint8)
    assert np.array_equal(pr.decode(f, fmt), yuv_ref.rgb_from_yuv(f, fmt))
    assert np.array_equal(pr.decode(f, fmt, "bt601", "limited"), yuv_ref.rgb_from_yuv(f, fmt))
    assert not np.array_equal(pr.decode(f, fmt, "bt709", "limited"), yuv_ref.rgb_from_yuv(f, fmt))


def test_yuyv_under_the_default_description_decodes_as_nv12_does():
    g = np.arange(0, 256, 3)
    Y, U, V = np.meshgrid(g, g, g, indexing="ij")
    assert np.array_equal(pr.yuv_to_rgb(Y, U, V), yuv_ref.yuv_to_rgb(Y, U, V))


def test_grey_levels_map_as_derived():
    for matrix in pr.MATRICES:
        for bits, lo, hi in ((8, 16, 235), (10, 64, 940)):
            c = 128 << (bits - 8)
            assert pr.yuv_to_rgb(lo, c, c, matrix, "limited", bits).tolist() == [0, 0, 0]
            assert pr.yuv_to_rgb(hi, c, c, matrix, "limited", bits).tolist() == [255, 255, 255]
            assert pr.yuv_to_rgb(0, c, c, matrix, "limited", bits).tolist() == [0, 0, 0]             # below black: not negative
            top = (1 << bits) - 1
            assert pr.yuv_to_rgb(0, c, c, matrix, "full", bits).tolist() == [0, 0, 0]
            assert pr.yuv_to_rgb(top, c, c, matrix, "full", bits).tolist() == [255, 255, 255]
            # full range 8-bit is the identity on greys
            if bits == 8:
                g = np.arange(256)
                assert np.array_equal(pr.yuv_to_rgb(g, 128, 128, matrix, "full")[:, 1], g)


def test_layouts_and_nearest_chroma():
    H, W = 4, 6
    rng = np.random.default_rng(0)
    y = rng.integers(0, 256, (H, W), dtype=np.uint8)
    u = rng.integers(0, 256, (H, W // 2), dtype=np.uint8)
    v = rng.integers(0, 256, (H, W // 2), dtype=np.uint8)
    yuyv = np.stack([y[:, 0::2], u, y[:, 1::2], v], -1).reshape(H, 2 * W)
    uyvy = np.stack([u, y[:, 0::2], v, y[:, 1::2]], -1).reshape(H, 2 * W)
    assert yuyv[1, :8].tolist() == [y[1, 0], u[1, 0], y[1, 1], v[1, 0], y[1, 2], u[1, 1], y[1, 3], v[1, 1]]
    for matrix, r in itertools.product(pr.MATRICES, pr.RANGES):
        want = np.stack([[pr.yuv_to_rgb(y[i, j], u[i, j >> 1], v[i, j >> 1], matrix, r) for j in range(W)] for i in range(H)])
        assert np.array_equal(pr.decode(yuyv, "yuyv422", matrix, r), want)
        assert np.array_equal(pr.decode(uyvy, "uyvy422", matrix, r), want)
    # P010: words, chroma at (y >> 1, x >> 1), U then V
    y10 = rng.integers(0, 1024, (H, W), dtype=np.uint16)
    u10 = rng.integers(0, 1024, (H // 2, W // 2), dtype=np.uint16)
    v10 = rng.integers(0, 1024, (H // 2, W // 2), dtype=np.uint16)
    p010 = (np.concatenate([y10.ravel(), np.stack([u10, v10], -1).ravel()]).reshape(H * 3 // 2, W) << 6).astype(np.uint16)
    for matrix, r in itertools.product(pr.MATRICES, pr.RANGES):
        want = np.stack([[pr.yuv_to_rgb(y10[i, j], u10[i >> 1, j >> 1], v10[i >> 1, j >> 1], matrix, r, 10) for j in range(W)] for i in range(H)])
        assert np.array_equal(pr.decode(p010, "p010le", matrix, r), want)
    # random low 6 bits decode as zeros do
    noisy = p010 | rng.integers(0, 64, p010.shape, dtype=np.uint16)
    assert (noisy != p010).any() and np.array_equal(pr.decode(noisy, "p010le"), pr.decode(p010, "p010le"))


def test_encoder_feeds_the_decoder():
    rgb = np.zeros((4, 8, 3), np.uint8)
    rgb[:, :4] = (200, 30, 30)
    rgb[:, 4:] = (128, 128, 128)
    for fmt, matrix, r in itertools.product(pr.FMTS, pr.MATRICES, pr.RANGES):
        dec = pr.decode(pr.encode(rgb, fmt, matrix, r), fmt, matrix, r).astype(int)
        assert np.abs(dec - rgb).max() <= 3, (fmt, matrix, r, np.abs(dec - rgb).max())


@pytest.mark.parametrize("fmt", list(CODES))
def test_sizes_agree_between_python_and_library(tmp_path, fmt):
    from vbt_amd import rawvideo as rv
    _l, L = _lib()
    sizes = [(6, 8), (18, 34), (1080, 1920)] + ([(7, 8), (1, 2)] if fmt in ("yuyv422", "uyvy422", "rgb24") else [])
    per_pixel = {"rgb24": 3, "nv12": 1.5, "i420": 1.5, "yuyv422": 2, "uyvy422": 2, "p010le": 3}[fmt]
    for H, W in sizes:
        shape = rv.frame_shape(fmt, H, W)
        fb = int(np.prod(shape)) * rv.frame_dtype(fmt).itemsize
        assert fb == int(H * W * per_pixel) == L.vbt_pix_frame_bytes(H, W, CODES[fmt]), (H, W)
        assert rv.source_hw(np.zeros((2,) + shape, rv.frame_dtype(fmt)), fmt) == (H, W)
        if H * W > 1000:
            continue
        f = tmp_path / f"clip_{H}x{W}.raw"
        f.write_bytes(bytes(3 * fb))
        a = rv.open_raw(str(f), fmt, (W, H))
        assert a.shape == (3,) + shape and a.dtype == rv.frame_dtype(fmt) and not a.flags.writeable
        f.write_bytes(bytes(3 * fb - 1))                                   # not a whole number of frames
        with pytest.raises(ValueError):
            rv.open_raw(str(f), fmt, (W, H))
    # what the format refuses: 0 bytes from the library, ValueError from frame_shape
    refused = {"rgb24": [], "nv12": [(7, 8), (8, 7)], "i420": [(7, 8), (8, 7)], "yuyv422": [(8, 7), (8, 16386)], "uyvy422": [(8, 7), (16385, 8)],
               "p010le": [(7, 8), (8, 7), (16386, 8)]}[fmt]
    for H, W in refused + [(0, 8), (8, 0)]:
        assert L.vbt_pix_frame_bytes(H, W, CODES[fmt]) == 0, (H, W)
        if fmt != "rgb24":
            with pytest.raises(ValueError):
                rv.frame_shape(fmt, H, W)
    assert L.vbt_pix_frame_bytes(16384, 16384, CODES[fmt]) == int(16384 * 16384 * per_pixel)
    # the 16384 limit belongs to the 4:2:2 formats and P010: rgb24 / nv12 / i420 sources of the pipeline never had one and keep none
    for H, W in ((2, 16386), (16386, 8)):
        want = 0 if fmt in ("yuyv422", "uyvy422", "p010le") else int(H * W * per_pixel)
        assert L.vbt_pix_frame_bytes(H, W, CODES[fmt]) == want, (H, W)
        if fmt in ("rgb24", "nv12", "i420"):
            assert rv.frame_shape(fmt, H, W) == ((H, W, 3) if fmt == "rgb24" else (H * 3 // 2, W))
    for code in (3, 15, 19, -1):
        assert L.vbt_pix_frame_bytes(8, 8, code) == 0


def test_library_exports_the_new_entry_points():
    _l, L = _lib()
    names = {"vbt_pix_frame_bytes", "vbt_resize_frames_pix", "vbt_pipeline_set_colour"}
    assert all(hasattr(L, n) for n in names) and names <= set(_l.declared_symbols())


def test_resize_frames_pix_refuses_before_any_device_call():
    _l, L = _lib()
    src = np.zeros(8 * 8 * 3 + 64, np.uint8)
    dst = np.zeros(4 * 4 * 3, np.uint8)

    def call(H, W, fmt, matrix=0, rng=0, src_ptr=None, on_device=0, B=1, h=4):
        return L.vbt_resize_frames_pix(src.ctypes.data if src_ptr is None else src_ptr, B, H, W, fmt, matrix, rng, on_device, dst.ctypes.data, h, 4, 0, 0, None)
    cases = [((8, 8, 3), "pix_fmt"), ((8, 8, 15), "pix_fmt"), ((8, 8, 19), "pix_fmt"), ((8, 8, -1), "pix_fmt"), ((8, 8, 0), "vbt_resize_frames"),
             ((8, 8, 16, 2), "matrix"), ((8, 8, 1, -1), "matrix"), ((8, 8, 17, 0, 2), "range"), ((8, 8, 18, 1, -1), "range"),
             ((7, 8, 1), "size"), ((8, 7, 2), "size"), ((8, 7, 16), "size"), ((8, 7, 17), "size"), ((7, 8, 18), "size"), ((8, 7, 18), "size"),
             ((0, 8, 16), "size"), ((8, 16386, 17), "size"), ((16386, 8, 18), "size"),
             ((2, 16386, 1), "size"), ((16386, 8, 2), "size")]              # this entry point takes no side above 16384 in any format
    for args, word in cases:
        assert call(*args) == -1, args                                     # VBT_ERR_ARG, with or without a GPU
        assert word in L.vbt_last_error().decode(), (args, L.vbt_last_error())
    # a device source of a 4:2:2 or P010 format is loaded by dwords
    for fmt in (16, 17, 18):
        for off in (1, 2, 3):
            assert call(8, 8, fmt, src_ptr=0x7f0000001000 + off, on_device=1) == -1, (fmt, off)
            assert "aligned" in L.vbt_last_error().decode() and "src" in L.vbt_last_error().decode()
    assert call(8, 8, 16, B=0) == -1 and call(8, 8, 16, h=0) == -1
    with pytest.raises(_l.VbtArgError):
        _l.check(call(8, 7, 16))
    # the older entry point still takes 1 and 2 only
    for fmt in (16, 17, 18):
        assert L.vbt_resize_frames_yuv(src.ctypes.data, 1, 8, 8, fmt, 0, dst.ctypes.data, 4, 4, 0, 0, None) == -1
        assert "unknown" in L.vbt_last_error().decode()
    assert L.vbt_pipeline_set_colour(None, 0, 0) == -1 and L.vbt_pipeline_set_pixel_format(None, 16) == -1


def test_export_handles_keep_calling_the_new_formats_unknown():
    import ctypes
    _l, L = _lib()
    out = ctypes.c_void_p()
    h, w = ctypes.c_int(), ctypes.c_int()
    for fmt in (16, 17, 18):
        assert L.vbt_overlay_create(0, 8, 8, fmt, None, ctypes.byref(out)) == -1 and "unknown" in L.vbt_last_error().decode()
        assert L.vbt_mjpeg_create(0, 16, 16, fmt, 85, 1, ctypes.byref(out)) == -1 and "unknown" in L.vbt_last_error().decode()
        assert L.vbt_display_size(16, 16, fmt, 8, ctypes.byref(h), ctypes.byref(w)) == -1 and "unknown" in L.vbt_last_error().decode()
        assert L.vbt_scaler_create(0, 16, 16, 8, 8, fmt, ctypes.byref(out)) == -1 and "unknown" in L.vbt_last_error().decode()


def test_python_refusals_need_no_gpu():
    from vbt_amd.track import track_frames, track_many
    rgb = np.zeros((2, 8, 8, 3), np.uint8)
    yuyv = np.zeros((2, 8, 16), np.uint8)
    with pytest.raises(ValueError, match="color_matrix"):
        track_frames(rgb, "none.vbtm", color_matrix="bt709")
    with pytest.raises(ValueError, match="color_range"):
        track_frames(rgb, "none.vbtm", color_range="full")
    with pytest.raises(ValueError, match="unknown colour matrix"):
        track_frames(yuyv, "none.vbtm", pix_fmt="yuyv422", color_matrix="bt2020")
    with pytest.raises(ValueError, match="export"):
        track_frames(yuyv, "none.vbtm", pix_fmt="yuyv422", video_out=np.zeros((2, 8, 16), np.uint8))
    with pytest.raises(ValueError, match="export"):
        track_frames(np.zeros((2, 12, 8), np.uint8), "none.vbtm", pix_fmt="nv12", color_matrix="bt709", video_out=np.zeros((2, 12, 8), np.uint8))
    with pytest.raises(ValueError, match="color_matrix"):
        next(track_many([rgb], "none.vbtm", 1, color_matrix="bt709"))


# ---- cli track: usage errors, exit code 2, before any work ----
def _cli(args):
    from vbt_amd.cli import main
    return CliRunner().invoke(main, ["track"] + args)


def test_cli_refuses_colour_for_rgb24_and_avi(tmp_path):
    for opt, val in (("--color_matrix", "bt709"), ("--color_range", "full")):
        res = _cli(["nothing.npy", opt, val])
        assert res.exit_code == 2 and opt in res.output, res.output
        res = _cli(["nothing.rgb", "--pix_fmt", "rgb24", "--size", "8x8", opt, val])
        assert res.exit_code == 2 and opt in res.output, res.output
        res = _cli(["nothing.avi", "--pix_fmt", "nv12", "--size", "8x8", opt, val])
        assert res.exit_code == 2 and opt in res.output and "nothing.avi" in res.output, res.output
    res = _cli(["nothing.yuv", "--pix_fmt", "nv12", "--size", "8x8", "--color_matrix", "bt2020"])
    assert res.exit_code == 2 and "--color_matrix" in res.output, res.output
    res = _cli(["nothing.yuv", "--pix_fmt", "nv12", "--size", "8x8", "--color_range", "tv"])
    assert res.exit_code == 2 and "--color_range" in res.output, res.output


@pytest.mark.parametrize("fmt", ["yuyv422", "uyvy422", "p010le"])
def test_cli_refuses_new_formats_without_or_with_a_bad_size(fmt):
    res = _cli(["nothing.yuv", "--pix_fmt", fmt])
    assert res.exit_code == 2 and "--size" in res.output, res.output
    bad = ["1920", "17x8", "16386x8"] + (["16x7"] if fmt == "p010le" else [])
    for size in bad:
        res = _cli(["nothing.yuv", "--pix_fmt", fmt, "--size", size])
        assert res.exit_code == 2 and "--size" in res.output, (size, res.output)
    if fmt != "p010le":                                                    # odd height is fine for 4:2:2: the refusal is then the missing file
        res = _cli(["nothing.yuv", "--pix_fmt", fmt, "--size", "16x7"])
        assert res.exit_code != 2 and "--size" not in res.output, res.output


EXPORTS = (["--video_dir", "out"], ["--video_dir", "out", "--one_pass"], ["--video_dir", "out", "--hud"],
           ["--video_dir", "out", "--one_pass", "--live_hud"], ["--video_dir", "out", "--display_image_height", "8"], ["--one_pass"], ["--hud"],
           ["--live_hud"], ["--display_image_height", "8"])


@pytest.mark.parametrize("fmt", ["yuyv422", "uyvy422", "p010le"])
def test_cli_refuses_every_export_option_with_a_new_format(tmp_path, fmt):
    for extra in EXPORTS:
        extra = [str(tmp_path / "out") if a == "out" else a for a in extra]
        res = _cli(["nothing.yuv", "--pix_fmt", fmt, "--size", "16x8"] + extra)
        assert res.exit_code == 2 and fmt in res.output and extra[-1 if extra[-1].startswith("--") else -2] in res.output, (extra, res.output)
        assert "not drawn" in res.output, res.output
    assert not (tmp_path / "out").exists()
    from vbt_amd.cli import main
    res = CliRunner().invoke(main, ["overlay", "nothing.yuv", "nothing.pkl", "--pix_fmt", fmt, "--size", "16x8"])
    assert res.exit_code == 2 and "--pix_fmt" in res.output, res.output


def test_cli_refuses_every_export_option_with_a_non_default_colour(tmp_path):
    for extra in EXPORTS:
        extra = [str(tmp_path / "out") if a == "out" else a for a in extra]
        for opt, val in (("--color_matrix", "bt709"), ("--color_range", "full")):
            res = _cli(["nothing.yuv", "--pix_fmt", "nv12", "--size", "16x8", opt, val] + extra)
            assert res.exit_code == 2 and opt in res.output and "not drawn" in res.output, (extra, res.output)
    assert not (tmp_path / "out").exists()
