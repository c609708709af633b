"""Scaled export without a GPU (include/vbt_hip.h, "Scaled export"): the entry points of the C ABI and their bindings, the refusals
made before any device call, the size rule, the numpy statement (tests/scale_ref.py) against two cases worked out by hand, against
torch's bilinear filter in double within the derived bound, the shared core (vbt_amd/csrc/scale_core.h) as a stand-alone host program
under -fsanitize=address,undefined (tests/fuzz/scale_check.cc, run as a program, never loaded into Python) against the numpy statement
for every case of the GPU test, and the CLI's usage errors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from click.testing import CliRunner

import scale_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vbt_display_size", "vbt_scaler_create", "vbt_scaler_run", "vbt_scaler_tables", "vbt_scaler_destroy", "vbt_mjpeg_create_scaled")
ARG = -1
FMT = {"rgb24": 0, "nv12": 1, "i420": 2}
BOUND = 0.5 + 255.0 / 2048.0      # one rounding, plus two axes of weight quantisation at 255 * 0.5 / 2048 each


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib
    return _lib, _lib.lib()


def test_entry_points_are_exported_declared_and_bound():
    _lib_mod, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "vbt_hip.h")).read()
    assert "Scaled export" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in _lib_mod.declared_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, code), name
    from vbt_amd import scale
    assert callable(scale.display_size) and callable(scale.Scaler.run) and callable(scale.Scaler.tables)


def test_refusals_come_before_any_device_call_and_name_the_argument():
    _lib_mod, L = _lib()

    def err():
        return L.vbt_last_error().decode()

    def scaler(H, W, h, w, fmt):
        p = ctypes.c_void_p()
        return L.vbt_scaler_create(0, H, W, h, w, fmt, ctypes.byref(p)), err(), p.value

    assert L.vbt_scaler_create(0, 8, 8, 4, 4, 0, None) == ARG and "out" in err()
    for args, word in (((8, 8, 4, 4, 3), "pix_fmt"), ((8, 8, 4, 4, -1), "pix_fmt"), ((0, 8, 4, 4, 0), "H and W"), ((8, 16385, 4, 4, 0), "H and W"),
                       ((8, 8, 0, 4, 0), "h and w"), ((8, 8, 4, 16385, 0), "h and w"), ((7, 8, 4, 4, 1), "even H and W"), ((8, 8, 4, 3, 2), "even h and w"),
                       ((8, 8, 5, 4, 1), "even h and w")):
        rc, msg, h = scaler(*args)
        assert rc == ARG and word in msg and "vbt_scaler_create" in msg and not h, (args, msg)
    assert L.vbt_scaler_run(None, 1, 1, 1, None) == ARG and "handle" in err()
    n = ctypes.c_int()
    assert L.vbt_scaler_tables(None, 0, 0, None, None, 0, ctypes.byref(n)) == ARG and "handle" in err()
    L.vbt_scaler_destroy(None)

    def enc(H, W, h, w, fmt, q=85, mb=4):
        p = ctypes.c_void_p()
        return L.vbt_mjpeg_create_scaled(0, H, W, h, w, fmt, q, mb, ctypes.byref(p)), err(), p.value
    assert L.vbt_mjpeg_create_scaled(0, 8, 8, 4, 4, 0, 85, 4, None) == ARG and "out" in err()
    for args, word in (((8, 8, 4, 4, 7), "pixel format"), ((8, 0, 4, 4, 0), "16384"), ((8, 8, 4, 0, 0), "h and w"), ((8, 8, 16385, 4, 0), "h and w"),
                       ((8, 8, 4, 5, 1), "even h and w"), ((8, 8, 3, 4, 2), "even h and w"), ((6, 9, 4, 4, 1), "even H and W")):
        rc, msg, h = enc(*args)
        assert rc == ARG and word in msg and "vbt_mjpeg_create_scaled" in msg and not h, (args, msg)
    rc, msg, _ = enc(8, 8, 4, 4, 0, q=0)
    assert rc == ARG and "quality" in msg
    rc, msg, _ = enc(8, 8, 4, 4, 0, mb=0)
    assert rc == ARG and "max_batch" in msg


def test_display_size_is_the_references_expression():
    _lib_mod, L = _lib()
    from vbt_amd.scale import display_size
    assert display_size(1080, 1920, "rgb24", 720) == (720, 1280) == S.display_size(1080, 1920, "rgb24", 720)
    assert display_size(1920, 1080, "rgb24", 720) == (720, 405)                     # a portrait source: int(720 * 0.5625)
    assert display_size(1920, 1080, "nv12", 720) == (720, 404) == S.display_size(1920, 1080, "nv12", 720)
    assert display_size(1920, 1080, "i420", 720) == (720, 404)
    rng = np.random.default_rng(5)
    for H, W, d in rng.integers(1, 4000, (200, 3)):
        for fmt in ("rgb24", "nv12"):
            H2, W2, d2 = (int(H), int(W), int(d)) if fmt == "rgb24" else (2 * int(H), 2 * int(W), 2 * int(d))
            try:
                want = S.display_size(H2, W2, fmt, d2)
            except ValueError:
                want = None
            try:
                got = display_size(H2, W2, fmt, d2)
            except _lib_mod.VbtArgError:
                got = None
            assert got == want, (H2, W2, fmt, d2)
    h, w = ctypes.c_int(), ctypes.c_int()
    for args, word in (((1080, 1920, 1, 721), "display_height"), ((1080, 1920, 0, 0), "display_height"), ((1080, 1920, 0, 16385), "display_height"),
                       ((2, 16384, 0, 4), "width"), ((16384, 1, 0, 100), "width"), ((16384, 2, 1, 100), "width"), ((0, 8, 0, 4), "H and W"),
                       ((9, 8, 1, 4), "H and W"), ((8, 8, 5, 4), "pix_fmt")):
        assert L.vbt_display_size(*args, ctypes.byref(h), ctypes.byref(w)) == ARG, args
        msg = L.vbt_last_error().decode()
        assert word in msg and "vbt_display_size" in msg, (args, msg)
    assert L.vbt_display_size(8, 8, 0, 4, None, ctypes.byref(w)) == ARG
    with pytest.raises(ValueError):
        display_size(1080, 1920, "nv12", 721)


def test_two_cases_by_hand():
    """1 x 4 -> 1 x 2: step 2, f = 0.5 and 2.5: taps (0, 1) and (2, 3) at weight 1024 each: the means 15.0 and 35.5, and 35.5 + 0.5
    floors to 36 (halves round up).
    2 x 2 -> 3 x 3: step 2 / 3, f = max(-1 / 6, 0) = 0, 0.5 and 7 / 6: (i0, a) = (0, 0), (0, 1024), (1, rint(2048 / 6) = 341) and the last
    one's i1 clamps to 1, so its weight does not matter: corners stay, edges are means of two, the centre the mean of four."""
    i0, i1, a = S.axis_table(4, 2)
    assert (i0.tolist(), i1.tolist(), a.tolist()) == ([0, 2], [1, 3], [1024, 1024])
    p = np.array([10, 20, 30, 41], np.uint8).reshape(1, 1, 4, 1)
    assert S.scale_plane(p, 1, 2).reshape(-1).tolist() == [15, 36]
    i0, i1, a = S.axis_table(2, 3)
    assert (i0.tolist(), i1.tolist(), a.tolist()) == ([0, 0, 1], [1, 1, 1], [0, 1024, 341])
    p = np.array([[0, 100], [200, 255]], np.uint8).reshape(1, 2, 2, 1)
    assert S.scale_plane(p, 3, 3)[0, :, :, 0].tolist() == [[0, 50, 100], [100, 139, 178], [200, 228, 255]]


def test_identity_is_a_copy():
    for fmt, shape in (("rgb24", (2, 16, 16, 3)), ("nv12", (2, 24, 16)), ("i420", (2, 24, 16))):
        f = S.noise(shape, 3)
        assert np.array_equal(S.scale_frames(f, fmt, 16, 16), f), fmt
    i0, _, a = S.axis_table(16, 16)
    assert i0.tolist() == list(range(16)) and not a.any()


@pytest.mark.parametrize("case", S.TORCH_CASES, ids=lambda c: "%dx%d-%dx%d" % c)
def test_reference_is_within_the_derived_bound_of_double_bilinear(case):
    import torch
    H, W, h, w = case
    p = S.noise((1, H, W, 3), 7)
    if (H, W) == (1080, 1920):
        p[:, :540] = 255                                                            # the largest sums
    r = S.scale_plane(p, h, w)
    t = torch.nn.functional.interpolate(torch.from_numpy(p).permute(0, 3, 1, 2).double(), size=(h, w), mode="bilinear", align_corners=False, antialias=False)
    d = np.abs(r.astype(np.float64) - t.permute(0, 2, 3, 1).numpy()).max()
    print(case, "max |ref - double bilinear| = %.4f, bound %.4f" % (d, BOUND))
    assert d <= BOUND


def test_yuv_planes_use_their_own_tables():
    """nv12 and i420 of the same samples scale to the same samples; chroma uses the tables of the half-size planes"""
    H, W, h, w = 36, 52, 24, 34
    nv12 = S.noise((2, H * 3 // 2, W), 8)
    uv = nv12[:, H:].reshape(2, H // 2, W // 2, 2)
    i420 = np.concatenate([nv12[:, :H].reshape(2, -1), uv[..., 0].reshape(2, -1), uv[..., 1].reshape(2, -1)], axis=1).reshape(2, H * 3 // 2, W)
    a, b = S.scale_frames(nv12, "nv12", h, w), S.scale_frames(i420, "i420", h, w)
    assert a.shape == b.shape == (2, h * 3 // 2, w)
    assert np.array_equal(a[:, :h], b[:, :h])
    auv = a[:, h:].reshape(2, h // 2, w // 2, 2)
    assert np.array_equal(auv[..., 0].reshape(2, -1), b[:, h:].reshape(2, -1)[:, :(h // 2) * (w // 2)])
    assert np.array_equal(auv[..., 1].reshape(2, -1), b[:, h:].reshape(2, -1)[:, (h // 2) * (w // 2):])
    assert np.array_equal(auv[..., :1], S.scale_plane(uv[..., :1], h // 2, w // 2))


# ---- the shared core under sanitizers ----

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scale") / "scale_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "fuzz", "scale_check.cc"), "-o", exe])
    return exe


def write_case(path, fmt, H, W, h, w, src, want):
    with open(path, "wb") as f:
        f.write(np.array([FMT[fmt], H, W, h, w, len(src)], np.int32).tobytes())
        pairs = [(H, h), (W, w)] + ([(H // 2, h // 2), (W // 2, w // 2)] if S.is_yuv(fmt) else [])
        for n_src, n_dst in pairs:
            i0, _, a = S.axis_table(n_src, n_dst)
            f.write(i0.astype(np.int32).tobytes() + a.astype(np.int32).tobytes())
        f.write(np.ascontiguousarray(src).tobytes() + np.ascontiguousarray(want).tobytes())


@pytest.mark.parametrize("case", S.cases() + [c for c in S.enc_cases() if c not in S.cases()],
                         ids=lambda c: "%s-%dx%d-%dx%d" % c)
def test_host_program_equals_the_numpy_statement(harness, tmp_path, case):
    fmt, H, W, h, w = case
    src = S.noise((2,) + S.frame_shape(fmt, H, W), 11)
    path = str(tmp_path / "case.bin")
    write_case(path, fmt, H, W, h, w, src, S.scale_frames(src, fmt, h, w))
    p = subprocess.run([harness, path], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok" and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, (p.stdout[-1000:], p.stderr[-3000:])


def test_host_program_sees_a_wrong_byte(harness, tmp_path):
    src = S.noise((1, 9, 13, 3), 12)
    want = S.scale_frames(src, "rgb24", 31, 40).copy()
    want[0, 30, 39, 2] ^= 1
    path = str(tmp_path / "case.bin")
    write_case(path, "rgb24", 9, 13, 31, 40, src, want)
    p = subprocess.run([harness, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 1 and "byte %d" % (31 * 40 * 3 - 1) in p.stdout, (p.stdout, p.stderr[-2000:])


# ---- CLI ----

def test_cli_usage_errors_come_before_any_output(tmp_path):
    from vbt_amd.cli import main
    src = tmp_path / "clip.npy"
    np.save(str(src), np.zeros((2, 1, 40, 3), np.uint8))
    out = tmp_path / "out"
    for cmd in ("track", "overlay"):
        res = CliRunner().invoke(main, [cmd, "--help"])
        assert res.exit_code == 0 and "--display_image_height" in res.output and "720" in res.output and "window" in res.output, res.output
    res = CliRunner().invoke(main, ["track", str(src), "--display_image_height", "20"])
    assert res.exit_code == 2 and "--video_dir" in res.output, res.output
    for bad in ("0", "16385", "-4"):
        res = CliRunner().invoke(main, ["track", str(src), "--video_dir", str(out), "--display_image_height", bad])
        assert res.exit_code == 2 and "1..16384" in res.output, res.output
    res = CliRunner().invoke(main, ["track", str(src), "--video_dir", str(out), "--display_image_height", "1000"])     # 1000 * 40 = 40000 wide
    assert res.exit_code == 2 and "width" in res.output and "--display_image_height" in res.output, res.output
    res = CliRunner().invoke(main, ["track", str(src), "--video_dir", str(out), "--video_format", "mjpeg", "--display_image_height", "1000", "--concurrent", "2"])
    assert res.exit_code == 2 and "width" in res.output, res.output
    yuv = tmp_path / "clip.yuv"
    np.zeros((2, 12, 8), np.uint8).tofile(str(yuv))
    res = CliRunner().invoke(main, ["track", str(yuv), "--pix_fmt", "nv12", "--size", "8x8", "--video_dir", str(out), "--display_image_height", "5"])
    assert res.exit_code == 2 and "odd" in res.output and "nv12" in res.output, res.output
    df = tmp_path / "clip_id1_m.pkl.gz"
    df.write_bytes(b"")
    res = CliRunner().invoke(main, ["overlay", str(src), str(df), "--video_dir", str(out), "--display_image_height", "0"])
    assert res.exit_code == 2 and "1..16384" in res.output, res.output
    res = CliRunner().invoke(main, ["overlay", str(yuv), str(df), "--pix_fmt", "i420", "--size", "8x8", "--video_dir", str(out), "--display_image_height", "7"])
    assert res.exit_code == 2 and "odd" in res.output, res.output
    assert not out.exists()                                                         # nothing was created on the way
