"""YUV 4:2:0 ingest without a GPU: the numpy statement of the conversion contract (tests/yuv_ref.py), the two new symbols of the C
ABI, the argument refusals of vbt_resize_frames_yuv (made before any device call) and the raw-file side of `cli track`."""
import numpy as np
import pytest
from click.testing import CliRunner

import yuv_ref


def test_reference_conversion_sanity_values():
    assert yuv_ref.yuv_to_rgb(16, 128, 128).tolist() == [0, 0, 0]
    assert yuv_ref.yuv_to_rgb(235, 128, 128).tolist() == [255, 255, 255]
    # mid grey: (1220542 * 110 + 2^19) >> 20 = 128
    assert yuv_ref.yuv_to_rgb(126, 128, 128).tolist() == [128, 128, 128]


def test_reference_conversion_clips_at_both_ends():
    assert yuv_ref.yuv_to_rgb(0, 128, 128).tolist() == [0, 0, 0]            # Y < 16 is black, not negative
    assert yuv_ref.yuv_to_rgb(15, 128, 128).tolist() == [0, 0, 0]
    assert yuv_ref.yuv_to_rgb(255, 128, 128).tolist() == [255, 255, 255]    # above nominal white saturates
    # extreme chroma, both signs (values worked out by hand from the formula in include/vbt_hip.h)
    assert yuv_ref.yuv_to_rgb(16, 0, 0).tolist() == [0, 154, 0]             # R, B negative -> 0; G = (2^19 + 1262485 * 128) >> 20
    assert yuv_ref.yuv_to_rgb(255, 255, 255).tolist() == [255, 125, 255]    # R, B above 255 -> 255
    assert yuv_ref.yuv_to_rgb(128, 255, 0).tolist() == [0, 185, 255]
    assert yuv_ref.yuv_to_rgb(128, 0, 255).tolist() == [255, 77, 0]
    assert yuv_ref.yuv_to_rgb(235, 0, 0).tolist() == [51, 255, 0]
    assert yuv_ref.yuv_to_rgb(16, 255, 255).tolist() == [203, 0, 255]
    # every byte triple stays inside int32 and inside 0..255
    g = np.arange(0, 256, 5)
    Y, U, V = np.meshgrid(g, g, g, indexing="ij")
    rgb = yuv_ref.yuv_to_rgb(Y, U, V).astype(np.int64)
    y64 = np.maximum(Y.astype(np.int64) - 16, 0) * 1220542 + (1 << 19)
    want = np.stack([(y64 + 1673527 * (V - 128)) >> 20, (y64 - 409993 * (U - 128) - 852492 * (V - 128)) >> 20, (y64 + 2116026 * (U - 128)) >> 20], -1)
    assert np.array_equal(rgb, np.clip(want, 0, 255))
    assert want.min() < 0 and want.max() > 255


def test_reference_plane_layouts_and_nearest_chroma():
    H, W = 4, 6
    rng = np.random.default_rng(0)
    y = rng.integers(0, 256, (H, W), dtype=np.uint8)
    u = rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8)
    v = rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8)
    nv12 = np.concatenate([y.ravel(), np.stack([u, v], -1).ravel()]).reshape(H * 3 // 2, W)
    i420 = np.concatenate([y.ravel(), u.ravel(), v.ravel()]).reshape(H * 3 // 2, W)
    want = np.stack([[yuv_ref.yuv_to_rgb(y[r, c], u[r >> 1, c >> 1], v[r >> 1, c >> 1]) for c in range(W)] for r in range(H)])
    assert np.array_equal(yuv_ref.rgb_from_nv12(nv12), want)
    assert np.array_equal(yuv_ref.rgb_from_i420(i420), want)
    # the test-only encoder feeds the decoder: grey stays grey, primaries keep their order
    grey = np.full((2, 2, 3), 128, np.uint8)
    for fmt in ("nv12", "i420"):
        assert np.abs(yuv_ref.rgb_from_yuv(yuv_ref.encode(grey, fmt), fmt).astype(int) - 128).max() <= 2
        red = yuv_ref.rgb_from_yuv(yuv_ref.encode(np.tile(np.uint8([200, 30, 30]), (2, 2, 1)), fmt), fmt)[0, 0]
        assert red[0] > 150 and red[1] < 80 and red[2] < 80


def test_library_exports_the_yuv_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "vbt_resize_frames_yuv") and hasattr(L, "vbt_pipeline_set_pixel_format")
    assert {"vbt_resize_frames_yuv", "vbt_pipeline_set_pixel_format"} <= set(_lib.declared_symbols())


def test_resize_frames_yuv_refuses_bad_arguments_before_any_device_call():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib
    L = _lib.lib()
    src = np.zeros(8 * 8 * 3 // 2 + 64, np.uint8)
    dst = np.zeros(4 * 4 * 3, np.uint8)

    def call(H, W, fmt):
        return L.vbt_resize_frames_yuv(src.ctypes.data, 1, H, W, fmt, 0, dst.ctypes.data, 4, 4, 0, 0, None)
    for H, W, fmt, word in ((7, 8, 1, "even"), (8, 7, 2, "even"), (8, 8, 3, "unknown"), (8, 8, -1, "unknown"), (8, 8, 0, "vbt_resize_frames")):
        assert call(H, W, fmt) == -1, (H, W, fmt)                       # VBT_ERR_ARG, with or without a GPU
        assert word in L.vbt_last_error().decode(), (H, W, fmt, L.vbt_last_error())
    with pytest.raises(_lib.VbtArgError):
        _lib.check(call(7, 8, 1))
    assert L.vbt_pipeline_set_pixel_format(None, 1) == -1


def test_raw_file_length_check(tmp_path):
    from vbt_amd.cli import main
    W, H = 16, 8
    fb = W * H * 3 // 2
    bad = tmp_path / "short.yuv"
    bad.write_bytes(bytes(2 * fb + 5))
    res = CliRunner().invoke(main, ["track", str(bad), "--pix_fmt", "nv12", "--size", f"{W}x{H}"])
    assert res.exit_code != 0 and "short.yuv" in res.output and str(fb) in res.output and f"{W}x{H}" in res.output, res.output
    from vbt_amd.rawvideo import open_raw
    good = tmp_path / "ok.yuv"
    good.write_bytes(bytes(3 * fb - 1))
    with pytest.raises(ValueError):
        open_raw(str(good), "i420", (W, H))
    good.write_bytes(bytes(3 * fb))
    for fmt, shape in (("nv12", (3, H * 3 // 2, W)), ("i420", (3, H * 3 // 2, W))):
        a = open_raw(str(good), fmt, (W, H))
        assert a.shape == shape and a.dtype == np.uint8 and not a.flags.writeable
    assert open_raw(str(good), "rgb24", (W, H // 2)).shape == (3, H // 2, W, 3)          # packed raw RGB: 3 bytes per pixel


def test_size_parsing():
    from vbt_amd.cli import main
    from vbt_amd.rawvideo import frame_shape, parse_size, source_hw
    assert parse_size("1920x1080") == (1920, 1080) and parse_size(" 64X48 ") == (64, 48)
    for bad in ("1920", "x1080", "1920x", "0x8", "19.2x10", "1920x1080x3", "axb"):
        with pytest.raises(ValueError):
            parse_size(bad)
    assert frame_shape("nv12", 1080, 1920) == (1620, 1920) and frame_shape("rgb24", 1080, 1920) == (1080, 1920, 3)
    with pytest.raises(ValueError):
        frame_shape("i420", 1080, 1921)
    assert source_hw(np.zeros((2, 1620, 1920), np.uint8), "nv12") == (1080, 1920)
    assert source_hw(np.zeros((2, 6, 8, 3), np.uint8), "rgb24") == (6, 8)
    for size in ("1920", "17x8", "16x7"):                                  # malformed, odd width, odd height
        res = CliRunner().invoke(main, ["track", "nothing.yuv", "--pix_fmt", "nv12", "--size", size])
        assert res.exit_code == 2 and "--size" in res.output, res.output


def test_cli_refuses_yuv_without_size(tmp_path):
    from vbt_amd.cli import main
    f = tmp_path / "clip.yuv"
    f.write_bytes(bytes(16 * 8 * 3 // 2))
    for fmt in ("nv12", "i420"):
        res = CliRunner().invoke(main, ["track", str(f), "--pix_fmt", fmt])
        assert res.exit_code == 2 and "--size" in res.output, res.output
    res = CliRunner().invoke(main, ["track", str(f), "--pix_fmt", "yuyv", "--size", "16x8"])
    assert res.exit_code == 2                                              # not a format this library takes
