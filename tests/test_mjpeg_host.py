"""MJPEG export without a GPU: the bitstream contract (include/vbt_hip.h, "MJPEG export") as tests/mjpeg_ref.py states it, pinned
against Pillow's decoder, Pillow's quantisation tables and Pillow's own encoder, and against cases worked out by hand; the AVI writer;
the four entry points of the C ABI and the refusals made before any device call."""
import ctypes
import io
import struct

import numpy as np
import pytest
from click.testing import CliRunner
from PIL import Image

import mjpeg_ref as M

ENTRY_POINTS = ("vbt_mjpeg_create", "vbt_mjpeg_destroy", "vbt_mjpeg_encode", "vbt_mjpeg_read")
# The reference's PSNR minus that of Pillow's encoder on the two 48 x 64 frames below, measured ("MJPEG export"):
#   smooth  q50 -0.047  q85 +0.054  q95 +0.061      noise  q50 -0.003  q85 +0.006  q95 +0.002   dB
# The largest shortfall is 0.047 dB; the test allows max(0.25, 2 x 0.047) = 0.25 dB.
PSNR_MARGIN_DB = 0.25


def smooth_frame(H=48, W=64):
    """a gradient in every channel with a rectangle, a channel step and a disc on it"""
    y, x = np.mgrid[0:H, 0:W]
    im = np.stack([x * 255 // (W - 1), y * 255 // (H - 1), (x + y) * 255 // (H + W - 2)], -1).astype(np.uint8)
    im[10:30, 12:40] = (200, 30, 60)
    im[20:44, 34:60, 1] = 240
    im[(y - 30) ** 2 + (x - 20) ** 2 < 81] = (20, 220, 240)
    return im


def noise_frame(H=48, W=64, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def decode(jpeg):
    im = Image.open(io.BytesIO(jpeg))
    im.load()
    return im


def pillow_jpeg(frame, q, **kw):
    b = io.BytesIO()
    Image.fromarray(frame).save(b, "JPEG", quality=q, subsampling=2, **kw)
    return b.getvalue()


def test_reference_stream_decodes_in_pillow():
    for frame, fmt, size in ((smooth_frame(), "rgb24", (64, 48)), (noise_frame(17, 33), "rgb24", (33, 17)), (noise_frame(1, 1), "rgb24", (1, 1)),
                             (np.random.default_rng(3).integers(0, 256, (72, 64), dtype=np.uint8), "nv12", (64, 48)),
                             (np.random.default_rng(3).integers(0, 256, (72, 64), dtype=np.uint8), "i420", (64, 48))):
        jpeg = M.encode(frame, 85, fmt)
        im = decode(jpeg)
        assert im.size == size and im.mode == "RGB" and im.format == "JPEG"
        assert im.layer == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]              # 4:2:0: Y 2x2, Cb and Cr 1x1
        assert jpeg[:2] == b"\xff\xd8" and jpeg[-2:] == b"\xff\xd9" and len(M.header(size[1], size[0], 85)) == 629


@pytest.mark.parametrize("q", [1, 10, 49, 50, 75, 85, 95, 100])
def test_quantisation_tables_equal_pillows(q):
    want = decode(pillow_jpeg(noise_frame(), q)).quantization                          # natural order in Pillow 12
    got = M.dqt_tables(M.encode(noise_frame(16, 16), q))
    assert got[0] == list(want[0]) and got[1] == list(want[1])
    ql, qc = M.quant_tables(q)
    assert ql.tolist() == got[0] and qc.tolist() == got[1]


def test_huffman_tables_equal_pillows_default_tables():
    """Pillow without optimize=True writes the Annex K.3 tables: the DHT payloads must be the same bytes"""
    def dht(jpeg):
        out = {}
        for m, payload in M.segments(jpeg):
            p = 0
            while m == 0xC4 and p < len(payload):
                n = sum(payload[p + 1:p + 17])
                out[payload[p]] = payload[p + 1:p + 17 + n]
                p += 17 + n
        return out
    got, want = dht(M.encode(noise_frame(16, 16))), dht(pillow_jpeg(noise_frame(), 75))
    assert sorted(got) == [0x00, 0x01, 0x10, 0x11] and got == want


def test_quality_against_pillows_encoder():
    worst = 0.0
    for name, frame in (("smooth", smooth_frame()), ("noise", noise_frame())):
        for q in (50, 85, 95):
            ours = M.psnr(np.asarray(decode(M.encode(frame, q))), frame)
            theirs = M.psnr(np.asarray(decode(pillow_jpeg(frame, q, restart_marker_rows=1))), frame)
            print(f"{name} q{q}: reference {ours:.3f} dB, Pillow {theirs:.3f} dB, difference {ours - theirs:+.3f} dB")
            worst = max(worst, theirs - ours)
            assert ours >= theirs - PSNR_MARGIN_DB, (name, q, ours, theirs)
    assert worst < 0.5


def test_constant_grey_block_is_all_zero():
    assert not M.fdct(np.zeros((8, 8), np.int64)).any()
    info = {}
    M.encode(np.full((16, 16, 3), 128, np.uint8), 85, info=info)
    assert info["symbols"] == [("DC", 0, 0), ("EOB",)] * 6                          # Y = Cb = Cr = 128: every level is 0


def test_checkerboard_energy_sits_at_odd_frequencies_and_the_7_7_basis_block_codes_three_zrl():
    """A plain +-100 checkerboard is not a DCT basis function: (-1)^n has a part in every odd frequency, so its energy sits at the odd
    (v, u), most of it at (7, 7) - checked against the DCT in floating point.  The checkerboard whose energy is at (7, 7) ALONE is the
    one weighted like that basis function, cos((2y+1) 7 pi/16) cos((2x+1) 7 pi/16) scaled to a peak of +-100: quantised, (7, 7) is its only
    level, zigzag position 63 behind 62 zeros, which the stream codes as exactly three ZRL and then (run 14, size)."""
    y, x = np.mgrid[0:8, 0:8]
    plain = 100 * (1 - 2 * ((x + y) & 1))
    F = M.fdct(plain)
    k = np.arange(8)
    C = np.where(k[:, None] == 0, np.sqrt(1 / 8), 0.5) * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)
    assert np.abs(F - C @ plain @ C.T).max() <= 1.0
    odd = (y & 1) & (x & 1)
    assert not F[odd == 0].any() and F[odd == 1].all() and np.abs(F).argmax() == 63 and F[7, 7] == 657
    b = np.cos((2 * k + 1) * 7 * np.pi / 16)
    b /= np.abs(b).max()
    weighted = np.rint(100 * np.outer(b, b)).astype(np.int64)
    assert np.array_equal(np.sign(weighted), np.sign(plain)) and np.abs(weighted).max() == 100
    lv = M.quantise(M.fdct(weighted), M.quant_tables(85)[0])
    assert np.count_nonzero(lv) == 1 and lv[7, 7] == 14
    symbols = []
    M.code_block(M.BitWriter(), lv.reshape(64)[M.ZIGZAG], 0, M.huff_codes(M.DC_LUMA), M.huff_codes(M.AC_LUMA), symbols)
    assert symbols == [("DC", 0, 0), ("ZRL",), ("ZRL",), ("ZRL",), ("AC", 14, 4, 14)]


def test_colour_extremes_and_the_range_expansion_tie():
    assert M.rgb_to_ycc(255, 255, 255) == (255, 128, 128) and M.rgb_to_ycc(0, 0, 0) == (0, 128, 128)
    assert M.rgb_to_ycc(255, 0, 0) == (76, 85, 255) and M.rgb_to_ycc(0, 255, 0) == (150, 44, 21) and M.rgb_to_ycc(0, 0, 255) == (29, 255, 107)
    Y, Cb, Cr = M.planes_rgb(np.array([[[255, 0, 0]]], np.uint8))                    # 1 x 1: the pixel fills the MCU
    assert Y.shape == (16, 16) and Cb.shape == (8, 8) and (Y == 76).all() and (Cb == 85).all() and (Cr == 255).all()
    # (C - 128) 255 / 224 is 127.5 at C = 240 and -127.5 at C = 16, the only ties: away from zero, then the clip
    assert M.expand_chroma([16, 17, 128, 239, 240]).tolist() == [0, 2, 128, 254, 255]
    assert M.expand_chroma(np.arange(256)).tolist() == [min(max(int(np.floor(abs(c - 128) * 255 / 224 + 0.5)) * (1 if c >= 128 else -1) + 128, 0), 255)
                                                        for c in range(256)]
    assert M.expand_luma([0, 16, 17, 125, 235, 255]).tolist() == [0, 0, 1, 127, 255, 255]
    ties = [c for c in range(256) if ((c - 128) * 255 * 2) % 224 == 0 and ((c - 128) * 255 * 2 // 224) % 2]
    assert ties == [16, 240]


def test_restart_intervals_are_independent_units():
    """DRI = ceil(W / 16), RSTm counts mod 8 and an interval's bytes depend on its own MCU row only"""
    frame = noise_frame(160, 32, seed=11)
    info = {}
    jpeg = M.encode(frame, 95, info=info)
    seg = dict((m, p) for m, p in M.segments(jpeg))
    assert struct.unpack(">H", seg[0xDD])[0] == 2 and len(info["bits"]) == 10
    body = jpeg[629:-2]
    marks = [body[i + 1] for i in range(len(body) - 1) if body[i] == 0xFF and 0xD0 <= body[i + 1] <= 0xD7]
    assert marks == [0xD0 + i % 8 for i in range(9)]
    other = frame.copy()
    other[:16] = 255 - other[:16]
    info2 = {}
    M.encode(other, 95, info=info2)
    assert info2["raw"][0] != info["raw"][0] and info2["raw"][1:] == info["raw"][1:]


def _write_avi(path, frames, rate=30, scale=1):
    from vbt_amd.mjpeg import AviWriter
    with AviWriter(str(path), 64, 48, rate, scale) as w:
        for f in frames:
            w.write(f)
    return path.read_bytes()


def test_avi_writer_tree_index_and_rate(tmp_path):
    frames = [M.encode(smooth_frame(), q) for q in (50, 85, 95)]
    data = _write_avi(tmp_path / "a.avi", frames, 30000, 1001)
    avi = M.avi_parse(data)                                                        # (the walker asserts that the chunk sizes add up)
    assert avi["frames"] == frames
    assert avi["avih"]["total_frames"] == 3 and avi["avih"]["streams"] == 1 and avi["avih"]["flags"] & 0x10
    assert (avi["avih"]["width"], avi["avih"]["height"]) == (64, 48) and avi["avih"]["us_per_frame"] == 33367
    assert avi["strh"] == {"type": b"vids", "handler": b"MJPG", "scale": 1001, "rate": 30000, "length": 3}
    assert avi["strf"] == {"width": 64, "height": 48, "compression": b"MJPG"}
    assert len(avi["idx"]) == 3
    for (ckid, flags, off, size), frame, at in zip(avi["idx"], frames, avi["frame_offsets"]):
        p = avi["movi"] + off
        assert ckid == b"00dc" and p == at and data[p:p + 4] == b"00dc" and struct.unpack("<I", data[p + 4:p + 8])[0] == size == len(frame)
        assert data[p + 8:p + 10] == b"\xff\xd8" and data[p + 8 + size - 2:p + 8 + size] == b"\xff\xd9"
        assert p % 2 == 0
    for f in avi["frames"]:
        assert decode(f).size == (64, 48)


def test_avi_writer_pads_odd_frames_and_patches_an_empty_file(tmp_path):
    odd = b"\xff\xd8" + b"\x01" * 3 + b"\xff\xd9"
    data = _write_avi(tmp_path / "odd.avi", [odd, odd])
    avi = M.avi_parse(data)
    assert avi["frames"] == [odd, odd] and avi["idx"][1][2] - avi["idx"][0][2] == 8 + len(odd) + 1
    empty = M.avi_parse(_write_avi(tmp_path / "empty.avi", []))
    assert empty["avih"]["total_frames"] == 0 and empty["frames"] == [] and empty["idx"] == []


def test_avi_writer_refuses_to_pass_the_size_limit(tmp_path, monkeypatch):
    from vbt_amd import mjpeg
    frame = M.encode(smooth_frame(), 85)
    monkeypatch.setattr(mjpeg, "AVI_MAX_BYTES", 4000)
    w = mjpeg.AviWriter(str(tmp_path / "big.avi"), 64, 48, 30)
    written = 0
    with pytest.raises(ValueError) as e:
        for _ in range(10):
            w.write(frame)
            written += 1
    assert "4000" in str(e.value) and "quality" in str(e.value) and "shorter" in str(e.value) and 0 < written < 10
    w.close()
    data = (tmp_path / "big.avi").read_bytes()
    assert len(data) <= 4000 and len(M.avi_parse(data)["frames"]) == written        # what was written before is a valid file


def test_frame_rate_is_fps_over_stride():
    from vbt_amd.mjpeg import frame_rate
    assert frame_rate(30.0, 1) == (30, 1) and frame_rate(30.0, 16) == (15, 8) and frame_rate(29.97, 1) == (2997, 100) and frame_rate(60, 4) == (15, 1)


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib
    return _lib, _lib.lib()


def test_entry_points_are_exported_declared_and_bound():
    import os
    import re
    from conftest import ROOT
    _lib_mod, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "vbt_hip.h")).read()
    assert "MJPEG export" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in _lib_mod.declared_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def test_create_refuses_bad_arguments_before_any_device_call():
    _lib_mod, L = _lib()

    def create(H, W, fmt, quality=85, max_batch=4):
        h = ctypes.c_void_p()
        rc = L.vbt_mjpeg_create(0, H, W, fmt, quality, max_batch, ctypes.byref(h))
        assert rc != 0 and not h.value
        return rc, L.vbt_last_error().decode()
    for args, kw, word in (((71, 104, 1), {}, "even"), ((72, 103, 2), {}, "even"), ((16385, 64, 0), {}, "16384"), ((0, 64, 0), {}, "16384"),
                           ((72, 104, 3), {}, "unknown"), ((72, 104, 0), {"quality": 0}, "quality"), ((72, 104, 0), {"quality": 101}, "quality"),
                           ((72, 104, 0), {"max_batch": 0}, "max_batch")):
        rc, msg = create(*args, **kw)
        assert rc == -1 and word in msg, (args, kw, rc, msg)
    assert L.vbt_mjpeg_create(0, 72, 104, 0, 85, 4, None) == -1
    with pytest.raises(_lib_mod.VbtArgError):
        _lib_mod.check(create(71, 104, 1)[0])
    off = (ctypes.c_uint64 * 2)()
    assert L.vbt_mjpeg_encode(None, None, 1, None) == -1 and L.vbt_mjpeg_read(None, None, 0, off, None) == -1
    L.vbt_mjpeg_destroy(None)


def test_commands_list_the_video_format_options():
    from vbt_amd.cli import main
    for cmd in ("track", "overlay"):
        res = CliRunner().invoke(main, [cmd, "--help"])
        assert res.exit_code == 0 and "--video_format" in res.output and "--video_quality" in res.output and "mjpeg" in res.output
    res = CliRunner().invoke(main, ["overlay", "a", "b", "--video_quality", "0"])
    assert res.exit_code == 2
