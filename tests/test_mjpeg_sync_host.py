"""MJPEG import, the decode by subsequences that synchronise (include/vbt_hip.h, "Entropy decoding": SYNC), without a GPU: the schedule
of mjpegd_entropy_sync_kernel run on the host with the functions the kernel calls (tests/fuzz/jpeg_sync_fuzz.cc), built with
g++ -fsanitize=address,undefined like tests/fuzz/jpeg_fuzz.cc, against that program - the one-lane-per-interval walk - on the same files:
every vector, every truncation and every bit flip must give the same status and the same frame, with no sanitizer report and within
the round bound.  Nothing loaded into Python is run under a sanitizer."""
import os
import re
import subprocess

import numpy as np
import pytest

import mjpeg_dec_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(D.vectors())
SIZES = [(4, 256), (16, 8), (128, 256)]          # (S, N): N = 8 carries state from chunk to chunk on every vector


def _build(tmp, name):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "fuzz", name + ".cc"), "-o", exe])
    return exe


def _run(cmd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run(cmd, capture_output=True, text=True, errors="replace", env=env, timeout=600)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln]
    assert all(ln.startswith(("ok ", "refused ")) for ln in lines)
    return {os.path.basename(ln.split()[1].rstrip(":")): ln for ln in lines}


def _write_vectors(d):
    for name in NAMES:
        (d / name).write_bytes(D.vectors()[name])


def _write_damage(d):
    """the files of test_truncated_and_bit_flipped_streams_end_cleanly (tests/test_mjpeg_decode_host.py): 600 single-bit flips, the
    truncations, and the damaged frame of the GPU tests"""
    rng = np.random.default_rng(3)
    n = 0
    for name in ("own-17x33", "pil-40x56-restart-blocks-1", "pil-17x33-422", "pil-40x56-420-optimize", "pil-9x23-grey"):
        raw = np.frombuffer(D.vectors()[name], np.uint8)
        scan0 = D.parse(raw.tobytes())["scan"][0]
        for i in range(120):
            m = raw.copy()
            pos = int(rng.integers(2, scan0)) if i % 2 == 0 else int(rng.integers(scan0, len(raw)))
            m[pos] ^= np.uint8(1 << int(rng.integers(0, 8)))
            (d / f"{name}_b{i:03d}").write_bytes(m.tobytes())
            n += 1
        for i, cut in enumerate(sorted(set([0, 1, 2, 3, 4, 20, scan0 - 1, scan0, scan0 + 1, len(raw) - 3, len(raw) - 1] + list(range(0, len(raw), max(1, len(raw) // 25)))))):
            (d / f"{name}_t{i:03d}").write_bytes(raw[:cut].tobytes())
            n += 1
    (d / "damaged").write_bytes(D.damaged_frame(D.vectors()["pil-40x56-restart-rows-1"]))
    return n + 1


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """both programs over both sets of files: {"vectors" | "damage": (lines of jpeg_fuzz, {(S, N): lines of jpeg_sync_fuzz})}"""
    tmp = tmp_path_factory.mktemp("jsync")
    old, new = _build(tmp, "jpeg_fuzz"), _build(tmp, "jpeg_sync_fuzz")
    out = {}
    for kind, fill in (("vectors", _write_vectors), ("damage", _write_damage)):
        d = tmp / kind
        d.mkdir()
        fill(d)
        out[kind] = (_run([old, str(d)]), {(S, N): _run([new, str(d), str(S), str(N)]) for S, N in SIZES})
    return out


def _fields(line):
    return {k: v for k, v in re.findall(r"(\w+)=(\w+)", line)}


def _same(old, new, N):
    assert old.keys() == new.keys()
    for name, ln in old.items():
        if ln.startswith("refused "):
            assert new[name] == ln
            continue
        want, got = _fields(ln), _fields(new[name])
        assert new[name].startswith("ok ") and (got["status"], got["fnv"]) == (want["status"], want["fnv"]), (name, ln, new[name])
        assert int(got["rounds"]) <= min(int(got["lanes"]), N) + 1, new[name]


@pytest.mark.parametrize("S,N", SIZES)
def test_every_vector_decodes_to_the_same_frame_in_parallel(runs, S, N):
    """status 0, the reference frame, and no interval left to the single lane: clean scans stay on the parallel path"""
    old, new = runs["vectors"]
    _same(old, new[(S, N)], N)
    for name in NAMES:
        got = _fields(new[(S, N)][name])
        assert got["status"] == "0" and got["fnv"] == f"{D.fnv1a(D.expected(name)):08x}" and got["single"] == "0", new[(S, N)][name]
    lanes = int(_fields(new[(S, N)]["own-16x2064-one-interval"])["lanes"])
    assert lanes == {4: 3952, 16: 988, 128: 124}[S]                   # at S = 4: 16 chunks of 256; at N = 8 every vector carries state between chunks


@pytest.mark.parametrize("S,N", SIZES)
def test_truncated_and_bit_flipped_streams_decode_as_one_lane_decodes_them(runs, S, N):
    old, new = runs["damage"]
    assert len(old) > 600
    _same(old, new[(S, N)], N)
    oks = [n for n, ln in old.items() if ln.startswith("ok ")]
    assert sum("status=0" not in old[n] for n in oks) > 50
    assert sum(int(_fields(new[(S, N)][n])["single"]) > 0 for n in oks) > 50          # damaged scans do reach the single lane
    assert "status=0" not in new[(S, N)]["damaged"] and int(_fields(new[(S, N)]["damaged"])["single"]) >= 1
