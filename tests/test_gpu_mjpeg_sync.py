"""MJPEG import on the GPU, entropy decoding by subsequences that synchronise (include/vbt_hip.h, "Entropy decoding": SYNC): the frames
and the status must EQUAL what the numpy statement (tests/mjpeg_dec_ref.py) and the one-lane-per-interval path give, at every
subsequence size, across chunks of lanes, over stuffed bytes on a subsequence boundary, for periodic scans, in batches, for a damaged
scan (which one lane must finish) and through a file.  The bit-for-bit claim itself is walked on the host under ASan / UBSan by
tests/test_mjpeg_sync_host.py."""
import functools
import os

import numpy as np
import pytest
from click.testing import CliRunner

import mjpeg_dec_ref as D
import mjpeg_ref as M

pytestmark = pytest.mark.gpu

NAMES = sorted(D.vectors())
INTERVAL, SYNC = 1, 2


def gpu_decode(jpegs, mode="sync", subseq=0, dec=None, max_batch=None):
    """-> (frames uint8 [B, H, W, 3], status int32 [B], entropy_info dict)"""
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.mjpeg import Decoder
    d = D.parse(jpegs[0])
    H, W = d["H"], d["W"]
    if dec is None:
        dec = Decoder(H, W, max_batch=max_batch or len(jpegs), entropy=mode, subseq_bytes=subseq)
    buf = DeviceBuffer(len(jpegs) * H * W * 3)
    dec.decode(jpegs, buf.ptr)
    status = dec.status()
    return buf.to_host((len(jpegs), H, W, 3), np.uint8), status, dec.entropy_info()


def assert_same_frame(got, want, what=""):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        y, x, c = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {want.size} samples differ; first at (y {y}, x {x}, c {c}): got {got[y, x, c]}, want {want[y, x, c]}")


def scan_of(jpeg):
    off, n = D.parse(jpeg)["scan"]
    return jpeg[off:off + n]


@functools.lru_cache(maxsize=None)
def reference(key):
    """(jpeg, the numpy statement's frame) of the frames the tests below share; computed once, read-only"""
    jpeg = {"noise-q100": lambda: D.pil_jpeg(D.noise((64, 64, 3), 7), quality=100, subsampling=2),
            "const-444": lambda: D.pil_jpeg(np.full((128, 128, 3), 90, np.uint8), subsampling=0),
            "const-420": lambda: D.pil_jpeg(np.full((128, 128, 3), 90, np.uint8), subsampling=2),
            "smooth-256": lambda: D.pil_jpeg(D.smooth(256, 256, 3), quality=85)}[key]()
    img, status = D.decode(jpeg, with_status=True)
    assert status == 0
    img.setflags(write=False)
    return jpeg, img


# ---- 1: every vector, three subsequence sizes
@pytest.mark.parametrize("S", [4, 32, 128])
@pytest.mark.parametrize("name", NAMES)
def test_every_vector_equals_the_numpy_statement(name, S):
    frames, status, info = gpu_decode([D.vectors()[name]], subseq=S)
    assert status.tolist() == [0]
    assert_same_frame(frames[0], D.expected(name), f"{name}, S = {S}")
    assert info["path"] == SYNC and info["subseq_bytes"] == S and info["single"] == 0, info


# ---- 2: a subsequence boundary between FF and its stuffed 00
@pytest.mark.parametrize("S", [4, 16, 32, 128])
def test_a_boundary_between_ff_and_its_stuffed_zero(S):
    jpeg, want = reference("noise-q100")
    scan = scan_of(jpeg)
    split = [i for i in range(S, len(scan), S) if scan[i - 1] == 0xFF and scan[i] == 0]
    assert len(split) >= 1, "no subsequence of this scan begins on a stuffed 00"
    frames, status, info = gpu_decode([jpeg], subseq=S)
    assert status.tolist() == [0] and info["path"] == SYNC and info["single"] == 0, (status, info)
    assert_same_frame(frames[0], want, f"S = {S}, {len(split)} split FF 00 pairs")


# ---- 3: periodic scans: a lane can hold the right bit position and zigzag index in the wrong block slot
@pytest.mark.parametrize("key", ["const-444", "const-420"])
def test_constant_frames_synchronise_in_the_block_slot_too(key):
    jpeg, want = reference(key)
    lanes = (len(scan_of(jpeg)) + 3) // 4
    frames, status, info = gpu_decode([jpeg], subseq=4)
    assert status.tolist() == [0] and info["single"] == 0
    assert_same_frame(frames[0], want, key)
    assert 1 <= info["rounds"] <= lanes + 1, (info, lanes)


# ---- 4: the lanes do synchronise
def test_a_smooth_frame_takes_few_rounds_over_two_chunks():
    """324 subsequences of 128 bytes, two chunks of lanes.  One round per lane (256) would mean that no guess ever meets the true state;
    the host run of the same schedule takes 12"""
    jpeg, want = reference("smooth-256")
    assert (len(scan_of(jpeg)) + 127) // 128 == 324
    frames, status, info = gpu_decode([jpeg], subseq=128)
    assert status.tolist() == [0] and info["single"] == 0
    assert_same_frame(frames[0], want, "smooth 256 x 256")
    assert 2 <= info["rounds"] <= 64, info


# ---- 5: batches
def mixed_batch():
    """five frames of 40 x 56, five kinds: 4:2:0, 4:4:4, grey, constant, noise"""
    v = D.vectors()
    return [v["pil-40x56-no-restarts"], D.pil_jpeg(D.smooth(40, 56, 5), quality=85, subsampling=0), D.pil_jpeg(D.smooth(40, 56, 6)[..., 1], quality=85),
            M.encode(np.full((40, 56, 3), 90, np.uint8), 85), M.encode(D.noise((40, 56, 3), 22), 85)]


@pytest.fixture(scope="module")
def mixed():
    jpegs = mixed_batch()
    return jpegs, [D.decode(j) for j in jpegs]


def test_batch_of_five_kinds_is_independent_per_frame(mixed):
    jpegs, want = mixed
    for what, order in (("in order", [0, 1, 2, 3, 4]), ("reversed", [4, 3, 2, 1, 0]), ("alone", [2])):
        frames, status, info = gpu_decode([jpegs[i] for i in order], max_batch=8, subseq=32)
        assert not status.any() and info["path"] == SYNC and info["single"] == 0, (what, status, info)
        for k, i in enumerate(order):
            assert_same_frame(frames[k], want[i], f"{what}, frame {i}")


def test_smaller_and_larger_batches_and_a_change_of_mode_on_one_handle(mixed):
    from vbt_amd.mjpeg import Decoder
    jpegs, want = mixed
    dec = Decoder(40, 56, max_batch=5, entropy="sync", subseq_bytes=16)
    assert dec.entropy[:2] == ("sync", 16)
    for first, n, mode, S in ((0, 5, None, 16), (1, 3, None, 16), (4, 1, "interval", 0), (0, 5, "sync", 4), (2, 2, "interval", 0), (0, 5, "sync", 64)):
        if mode:
            dec.set_entropy(mode, S)
        frames, status, info = gpu_decode(jpegs[first:first + n], dec=dec)
        assert not status.any()
        assert (info["path"], info["subseq_bytes"]) == ((SYNC, S) if S else (INTERVAL, 0)), info
        for k in range(n):
            assert_same_frame(frames[k], want[first + k], f"{n} frames from {first} ({mode}, {S}), frame {k}")


# ---- 6: a damaged scan is finished by one lane, exactly as the interval path decodes it
def test_a_damaged_scan_takes_the_single_lane_and_spoils_its_own_frame_only():
    v = D.vectors()
    good0, good2 = v["pil-40x56-restart-rows-1"], v["pil-40x56-420-optimize"]
    bad = D.damaged_frame(good0)
    want_status = D.decode(bad, with_status=True)[1]
    assert want_status != 0
    frames, status, info = gpu_decode([good0, bad, good2], subseq=32)
    old, old_status, old_info = gpu_decode([good0, bad, good2], mode="interval")
    assert info["path"] == SYNC and old_info["path"] == INTERVAL and info["single"] >= 1, (info, old_info)
    assert status.tolist() == [0, want_status, 0] and old_status.tolist() == status.tolist(), (status, old_status)
    assert_same_frame(frames[0], D.expected("pil-40x56-restart-rows-1"))
    assert_same_frame(frames[2], D.expected("pil-40x56-420-optimize"))
    assert_same_frame(frames[1], old[1], "the damaged frame against the interval path")


# ---- 7: AUTO
def test_auto_takes_the_new_path_for_long_intervals_only():
    from vbt_amd.mjpeg import Decoder
    mode, S, T = Decoder(16, 16, max_batch=1).entropy
    assert mode == "auto" and 2 * S <= T <= 131072, (mode, S, T)             # a 1080p camera frame (about 470 KB, one interval) takes SYNC
    side = min(1024, max(16, -(-int(np.ceil(np.sqrt(2.0 * T))) // 16) * 16))
    jpeg = D.pil_jpeg(D.noise((side, side, 3), 5), quality=75)
    d = D.parse(jpeg)
    assert d["ri"] == 0 and d["scan"][1] >= T, (side, d["scan"][1], T)
    frames, status, info = gpu_decode([jpeg], mode="auto")
    assert status.tolist() == [0] and info["path"] == SYNC and info["subseq_bytes"] == S and info["single"] == 0, info
    assert_same_frame(frames[0], D.pil_decode(jpeg), "the long scan (against libjpeg-turbo, which the numpy statement equals)")
    frames, status, info = gpu_decode([D.vectors()["own-16x16"]], mode="auto")
    assert status.tolist() == [0] and info["path"] == INTERVAL, info
    assert_same_frame(frames[0], D.expected("own-16x16"))


# ---- 8: ABI
def test_set_entropy_refuses_bad_arguments_and_info_needs_a_decode():
    import ctypes
    from vbt_amd import _lib
    from vbt_amd.mjpeg import Decoder
    L = _lib.lib()
    dec = Decoder(16, 16, max_batch=1)
    info = np.zeros(4, np.int32)
    assert L.vbt_mjpeg_decode_entropy_info(dec._h, info.ctypes.data, None) == -5       # VBT_ERR_STATE: nothing decoded yet
    dec.set_entropy("sync", 64)
    before = dec.entropy
    assert before[:2] == ("sync", 64)
    for mode, S in ((3, 0), (-1, 0), (2, 3), (2, 6), (2, 8192), (0, 2)):
        assert L.vbt_mjpeg_decoder_set_entropy(dec._h, mode, S) == -1, (mode, S)          # VBT_ERR_ARG
        assert dec.entropy == before
    v = [ctypes.c_int(-7) for _ in range(3)]
    assert L.vbt_mjpeg_decoder_get_entropy(dec._h, None, ctypes.byref(v[1]), None) == 0 and v[1].value == 64
    with pytest.raises(ValueError):
        Decoder(16, 16, entropy="fast")
    frames, status, info = gpu_decode([D.vectors()["own-16x16"]], dec=dec)
    assert status.tolist() == [0] and (info["path"], info["subseq_bytes"]) == (SYNC, 64)
    assert_same_frame(frames[0], D.expected("own-16x16"))


# ---- 9: through a file
def test_an_avi_without_restart_markers_tracks_the_same_in_both_modes(tmp_path, model_path):
    import pandas as pd
    from vbt_amd import synth
    from vbt_amd.cli import main
    clip = synth.clip_frames(12, 0, 12, size=416)
    jpegs = [D.pil_jpeg(f, quality=85) for f in clip]
    assert all(D.parse(j)["ri"] == 0 for j in jpegs)
    path = tmp_path / "clip.avi"
    path.write_bytes(D.build_avi([(b"00dc", j) for j in jpegs], 416, 416, rate=60))
    dfs = {}
    for mode in ("sync", "interval"):
        res = CliRunner().invoke(main, ["track", str(path), "--model", model_path, "--df_dir", str(tmp_path / mode), "--detection_treshold", "0.3",
                                        "--mjpeg_entropy", mode])
        assert res.exit_code == 0, res.output
        files = os.listdir(tmp_path / mode)
        assert len(files) == 1, res.output
        dfs[mode] = pd.read_pickle(str(tmp_path / mode / files[0]))
    assert len(dfs["sync"]) > 0
    pd.testing.assert_frame_equal(dfs["sync"], dfs["interval"], check_exact=True)
    np.save(str(tmp_path / "clip.npy"), clip[:2])
    res = CliRunner().invoke(main, ["track", str(tmp_path / "clip.npy"), "--model", model_path, "--mjpeg_entropy", "sync"])
    assert res.exit_code == 2 and "does not apply" in res.output, res.output
    res = CliRunner().invoke(main, ["overlay", str(tmp_path / "clip.npy"), str(tmp_path / "sync" / os.listdir(tmp_path / "sync")[0]), "--mjpeg_entropy", "interval"])
    assert res.exit_code == 2 and "does not apply" in res.output, res.output
