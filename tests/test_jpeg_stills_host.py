"""JPEG stills, the part that needs no GPU (include/vbt_hip.h, "JPEG stills"): the block count a file takes of a handle's budget, every
refusal of an argument, a header or a batch over the budget - all made before any device call - and the sanitizer run of the statement
the resize kernel runs per output pixel (jpeg_core.h: jpeg_resized_pixel), built host-only with g++ -fsanitize=address,undefined
(tests/fuzz/jpeg_stills_check.cc) over every vector at the GPU test's target sizes.  This is the only sanitizer run of the stills; nothing
loaded into Python is run under a sanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mjpeg_dec_ref as D
from oracle.preprocess import preprocess_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(D.vectors())
TARGETS = ((20, 28), (32, 32))
ERR_ARG, ERR_IO, ERR_CAPACITY = -1, -2, -4


def layout_blocks(jpeg):
    """jpeg_layout().blocks restated: whole MCUs, luma hs x vs blocks per MCU, each chroma component one"""
    d = D.parse(jpeg)
    hs, vs = d["comps"][0][:2]
    MW, MH = -(-d["W"] // (8 * hs)), -(-d["H"] // (8 * vs))
    return MW * MH * (hs * vs + 2) if len(d["comps"]) == 3 else MW * MH


def edge_vectors():
    """what the 15 vectors leave out: sources exactly at the targets (identity), W <= 4 beside W = 1 (the replicate rule at 4:2:0 and
    4:2:2), and a 2 x 2"""
    return {"pil-20x28-420": D.pil_jpeg(D.smooth(20, 28, 31), quality=85, subsampling=2), "pil-32x32-444": D.pil_jpeg(D.smooth(32, 32, 32), quality=85, subsampling=0),
            "pil-7x3-420": D.pil_jpeg(D.smooth(7, 3, 33), quality=85, subsampling=2), "pil-5x4-422": D.pil_jpeg(D.smooth(5, 4, 34), quality=85, subsampling=1),
            "pil-2x2-420": D.pil_jpeg(D.smooth(2, 2, 35), quality=85, subsampling=2)}


def expected_resized(jpeg, hw, swap):
    return preprocess_image(D.decode(jpeg), hw, swap_rb=bool(swap))[0]


@pytest.fixture(scope="module")
def L():
    from vbt_amd import _lib
    return _lib.lib()


def _blocks(L, jpeg):
    buf = np.frombuffer(jpeg, np.uint8)
    n = ctypes.c_uint32(0xFFFFFFFF)
    rc = L.vbt_jpeg_blocks(buf.ctypes.data, buf.nbytes, ctypes.byref(n))
    return rc, n.value


def test_blocks_helper_equals_the_layout(L):
    for name, jpeg in list(D.vectors().items()) + list(edge_vectors().items()):
        assert _blocks(L, jpeg) == (0, layout_blocks(jpeg)), name
    want = {"own-16x16": 6, "own-1x1": 6, "own-17x33": 2 * 3 * 6, "pil-24x40-444": 3 * 5 * 3, "pil-17x33-422": 3 * 3 * 4, "pil-9x23-grey": 2 * 3,
            "pil-40x56-no-restarts": 3 * 4 * 6, "own-16x2064-one-interval": 129 * 6}
    for name, n in want.items():
        assert layout_blocks(D.vectors()[name]) == n, name
    from vbt_amd import stills
    assert stills.blocks(D.vectors()["own-160x32-noise-q95"]) == 10 * 2 * 6
    assert L.vbt_jpeg_blocks(None, 0, None) == ERR_ARG
    rc, _ = _blocks(L, D.pil_jpeg(D.smooth(24, 40, 1), quality=85, progressive=True))
    assert rc == ERR_IO and "SOF2 (progressive)" in L.vbt_last_error().decode()


def test_plan_cuts_in_order_by_count_and_budget():
    from vbt_amd.stills import plan
    assert plan([], 4, 100) == []
    assert plan([10, 10, 10, 10, 10], 2, 100) == [(0, 2), (2, 4), (4, 5)]
    assert plan([60, 40, 1, 99, 100, 5], 8, 100) == [(0, 2), (2, 4), (4, 5), (5, 6)]
    with pytest.raises(ValueError, match="file 1 needs 101 blocks"):
        plan([1, 101], 8, 100)


def _handle(L, max_batch, budget):
    h = ctypes.c_void_p()
    assert L.vbt_jpeg_stills_create(0, max_batch, budget, ctypes.byref(h)) == 0
    return h


def _pack(jpegs):
    off = np.zeros(len(jpegs) + 1, np.uint64)
    off[1:] = np.cumsum([len(j) for j in jpegs])
    return np.frombuffer(b"".join(jpegs), np.uint8), off


def test_create_refuses_bad_arguments_without_a_device(L):
    h = ctypes.c_void_p()
    assert L.vbt_jpeg_stills_create(0, 4, 100, None) == ERR_ARG
    for args in ((0, 0, 100), (0, 1025, 100), (0, 4, 0), (0, 4, (1 << 24) + 1), (-1, 4, 100)):
        assert L.vbt_jpeg_stills_create(*args, ctypes.byref(h)) == ERR_ARG and not h.value, args
    h = _handle(L, 4, 100)
    assert L.vbt_jpeg_stills_set_entropy(h, 3, 0) == ERR_ARG and L.vbt_jpeg_stills_set_entropy(h, 2, 100) == ERR_ARG
    assert L.vbt_jpeg_stills_set_entropy(h, 2, 64) == 0
    v = [ctypes.c_int() for _ in range(3)]
    assert L.vbt_jpeg_stills_get_entropy(h, *(ctypes.byref(x) for x in v)) == 0 and [x.value for x in v] == [2, 64, 13920]
    st = np.zeros(4, np.int32)
    assert L.vbt_jpeg_stills_status(h, st.ctypes.data, None) == -5                       # VBT_ERR_STATE: nothing decoded yet
    L.vbt_jpeg_stills_destroy(h)


def test_decode_refusals_come_before_any_device_call(L):
    """The pointers given as device memory are not device memory: a call that got as far as the device would fail otherwise (or
    touch them).  Every case must return its own code with its own text."""
    v = D.vectors()
    good = [v["own-17x33"], v["pil-24x40-444"], v["pil-9x23-grey"]]
    budget = sum(layout_blocks(j) for j in good)
    h = _handle(L, 3, budget)
    data, off = _pack(good)
    dst = np.full(3 * 20 * 28 * 3, 0xA5, np.uint8)
    oo = np.zeros(4, np.uint64)

    def resized(hh=h, d=data.ctypes.data, o=off.ctypes.data, B=3, out=dst.ctypes.data, th=20, tw=28):
        return L.vbt_jpeg_stills_decode_resized(hh, d, o, B, out, th, tw, 0, None), L.vbt_last_error().decode()

    def full(hh=h, d=data.ctypes.data, o=off.ctypes.data, B=3, out=dst.ctypes.data, outs=oo.ctypes.data):
        return L.vbt_jpeg_stills_decode(hh, d, o, B, out, outs, None), L.vbt_last_error().decode()

    for call in (resized, full):
        for kw in (dict(hh=None), dict(d=None), dict(o=None), dict(out=None), dict(B=0), dict(B=-1)):
            assert call(**kw)[0] == ERR_ARG, (call.__name__, kw)
        rc, text = call(B=4)
        assert rc == ERR_CAPACITY and "4 frames, the handle was created for 3" in text
        desc = off.copy()
        desc[2] = desc[1] - 1
        rc, text = call(o=desc.ctypes.data)
        assert rc == ERR_ARG and "offsets[1] > offsets[2]" in text
    assert full(outs=None)[0] == ERR_ARG
    for kw in (dict(th=0), dict(tw=0), dict(th=-3), dict(tw=4097)):
        assert resized(**kw)[0] == ERR_ARG, kw
    # a batch over the block budget: the same three files on a handle one block short
    small = _handle(L, 3, budget - 1)
    for call in (resized, full):
        rc, text = call(hh=small)
        assert rc == ERR_CAPACITY and f"the batch takes {budget} blocks, the handle's budget is {budget - 1}" in text, text
    # a refused header names the frame of the batch and the reason
    bad = [good[0], good[1], D.pil_jpeg(D.smooth(24, 40, 1), quality=85, progressive=True)]
    bdata, boff = _pack(bad)
    for call in (resized, full):
        rc, text = call(d=bdata.ctypes.data, o=boff.ctypes.data)
        assert rc == ERR_IO and "frame 2 of the batch" in text and "SOF2 (progressive)" in text, text
    assert (dst == 0xA5).all()
    st = np.zeros(4, np.int32)
    assert L.vbt_jpeg_stills_status(h, st.ctypes.data, None) == -5                       # still nothing decoded
    L.vbt_jpeg_stills_destroy(h)
    L.vbt_jpeg_stills_destroy(small)


# ---- the sanitizer run
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jstills") / "jpeg_stills_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-ffp-contract=off", os.path.join(ROOT, "tests", "fuzz", "jpeg_stills_check.cc"), "-o", exe])
    return exe


def test_the_resized_pixel_statement_on_the_cpu_gives_the_numpy_frames(harness, tmp_path):
    """jpeg_resized_pixel over planes held in exactly blocks * 64 bytes: no tap reads outside them, and every (file, target, channel
    order) equals preprocess_image of the numpy statement's frame, bit for bit"""
    files = dict(D.vectors(), **edge_vectors())
    for name, jpeg in files.items():
        (tmp_path / name).write_bytes(jpeg)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([harness, str(tmp_path)] + [str(v) for hw in TARGETS for v in hw], capture_output=True, text=True, errors="replace", env=env, timeout=600)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    got = {}
    for ln in p.stdout.splitlines():
        f = ln.split()
        assert f[0] == "ok", ln
        got[(os.path.basename(f[1]), f[2], f[3])] = (f[4], f[5])
    assert len(got) == len(files) * len(TARGETS) * 2
    for name, jpeg in files.items():
        for hw in TARGETS:
            for swap in (0, 1):
                want = (f"blocks={layout_blocks(jpeg)}", f"fnv={D.fnv1a(expected_resized(jpeg, hw, swap)):08x}")
                assert got[(name, f"{hw[0]}x{hw[1]}", f"swap={swap}")] == want, (name, hw, swap)
