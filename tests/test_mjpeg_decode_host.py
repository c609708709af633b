"""MJPEG import, the part that needs no GPU (include/vbt_hip.h, "MJPEG import"): the numpy statement of the reconstruction
(tests/mjpeg_dec_ref.py) against Pillow's libjpeg-turbo; the header refusals of the library's parser with their reasons; vbt_jpeg_probe;
the AVI reader; and the sanitizer run of the parser and the decoding core (vbt_amd/csrc/jpeg_parse.h, jpeg_core.h) - the statements
the kernels run - built host-only with g++ -fsanitize=address,undefined (tests/fuzz/jpeg_fuzz.cc) and fed valid, truncated and
bit-flipped streams.  This is the only sanitizer run of the import; nothing loaded into Python is run under a sanitizer."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import mjpeg_dec_ref as D
import mjpeg_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(D.vectors())


# ---- the numpy statement is what libjpeg-turbo computes
@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_pillow(name):
    """integer algorithms on both sides: array_equal (measured: every vector is equal, no residue)"""
    jpeg = D.vectors()[name]
    got, status = D.decode(jpeg, with_status=True)
    assert status == 0
    assert np.array_equal(got, D.pil_decode(jpeg))


def test_vectors_are_what_they_claim():
    v = D.vectors()
    kinds = {name: (d["comps"][0][:2], len(d["comps"]), d["ri"]) for name, d in ((n, D.parse(v[n])) for n in NAMES)}
    assert kinds["pil-24x40-444"][:2] == ((1, 1), 3) and kinds["pil-17x33-422"][:2] == ((2, 1), 3) and kinds["pil-9x23-grey"][:2] == ((1, 1), 1)
    assert kinds["pil-40x56-no-restarts"] == ((2, 2), 3, 0) and kinds["pil-40x56-restart-blocks-1"] == ((2, 2), 3, 1)
    assert kinds["pil-40x56-restart-rows-1"] == ((2, 2), 3, 4)
    assert D.parse(v["pil-40x56-420-optimize"])["huff"] != D.STD_TABLES                    # tables of its own, with absent symbols
    assert sum(len(t[1]) for t in D.parse(v["pil-40x56-420-optimize"])["huff"].values()) < 2 * (12 + 162)
    d = D.parse(v["pil-40x56-restart-blocks-1"])
    scan = v["pil-40x56-restart-blocks-1"][d["scan"][0]:sum(d["scan"])]
    assert [m for _, _, m in D.intervals(scan)] == [k % 8 for k in range(11)] + [None]       # RSTm wraps past 7
    assert b"\xff\xc4" not in v["own-17x33-no-dht"] and np.array_equal(D.expected("own-17x33-no-dht"), D.expected("own-17x33"))
    d = D.parse(v["own-16x2064-one-interval"])
    assert d["ri"] == 129 and len(D.intervals(v["own-16x2064-one-interval"][d["scan"][0]:sum(d["scan"])])) == 1


# ---- the library's parser
def _probe(jpeg):
    from vbt_amd import _lib
    L = _lib.lib()
    buf = np.frombuffer(jpeg, np.uint8)
    v = [ctypes.c_int(-1) for _ in range(4)]
    rc = L.vbt_jpeg_probe(buf.ctypes.data, buf.nbytes, *(ctypes.byref(x) for x in v))
    return rc, tuple(x.value for x in v), L.vbt_last_error().decode()


def test_probe_needs_no_device():
    want = {"own-17x33": (17, 33, 3, 0x22), "pil-24x40-444": (24, 40, 3, 0x11), "pil-17x33-422": (17, 33, 3, 0x21), "pil-9x23-grey": (9, 23, 1, 0x11),
            "own-16x2064-one-interval": (16, 2064, 3, 0x22), "own-17x33-no-dht": (17, 33, 3, 0x22)}
    for name, w in want.items():
        rc, got, _ = _probe(D.vectors()[name])
        assert rc == 0 and got == w, (name, rc, got)
    from vbt_amd.mjpeg import probe
    assert probe(D.vectors()["own-1x1"]) == (1, 1, 3, 0x22)
    from vbt_amd import _lib
    assert _lib.lib().vbt_jpeg_probe(None, 0, None, None, None, None) == -1


def _patch_dqt16(jpeg):
    """table 0 rewritten as a 16-bit table: Pq = 1, 128 bytes of values"""
    p = jpeg.index(b"\xff\xdb")
    n = struct.unpack(">H", jpeg[p + 2:p + 4])[0]
    vals = jpeg[p + 5:p + 69]
    rest = jpeg[p + 69:p + 2 + n]
    body = bytes([0x10 | (jpeg[p + 4] & 15)]) + b"".join(bytes([0, v]) for v in vals) + rest
    return jpeg[:p] + b"\xff\xdb" + struct.pack(">H", len(body) + 2) + body + jpeg[p + 2 + n:]


def refusals():
    good = D.vectors()["own-17x33"]
    sos = good.index(b"\xff\xda")
    dht = good.index(b"\xff\xc4")
    sof = good.index(b"\xff\xc0")
    return {
        "progressive": (D.pil_jpeg(D.smooth(24, 40, 1), quality=85, progressive=True), "SOF2 (progressive)"),
        "dqt16": (_patch_dqt16(good), "16-bit DQT"),
        "length-past-end": (good[:dht + 2] + b"\xff\xf0" + good[dht + 4:], "segment length past the end"),
        "missing-sos": (good[:sos] + b"\xff\xd9", "missing SOS"),
        "truncated-in-headers": (good[:dht + 1], "missing SOS"),
        "twelve-bit": (good[:sof + 4] + b"\x0c" + good[sof + 5:], "12-bit precision"),
        "sampling-1x2": (good[:sof + 11] + b"\x12" + good[sof + 12:], "sampling 1x2"),
        "adobe-rgb": (good[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + good[2:], "Adobe APP14 transform 0"),
        "second-scan": (good[:-2] + good[sos:sos + 14] + b"\x00\xff\xd9", "more than one scan"),
        "missing-dqt": (good[:good.index(b"\xff\xdb")] + good[good.index(b"\xff\xdb") + 69:], "missing DQT"),
        "not-jpeg": (b"RIFF" + good[4:], "no SOI"),
    }


@pytest.mark.parametrize("case", sorted(refusals()))
def test_header_refusals_name_their_reason(case):
    jpeg, reason = refusals()[case]
    with pytest.raises(D.Refused, match=reason.replace("(", r"\(").replace(")", r"\)")):
        D.parse(jpeg)
    rc, _, text = _probe(jpeg)
    assert rc == -2 and reason in text, (rc, text)


def test_fill_bytes_app_and_com_segments_are_skipped():
    good = D.vectors()["own-17x33"]
    sof = good.index(b"\xff\xc0")
    padded = good[:2] + b"\xff\xfe\x00\x05abc" + b"\xff\xe1\x00\x04\xff\xd8" + good[2:sof] + b"\xff\xff\xff" + good[sof:]
    assert np.array_equal(D.decode(padded), D.expected("own-17x33"))
    assert _probe(padded)[:2] == (0, (17, 33, 3, 0x22))


# ---- the sanitizer run
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jfuzz") / "jpeg_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "fuzz", "jpeg_fuzz.cc"), "-o", exe])
    return exe


def _run(cmd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run(cmd, capture_output=True, text=True, errors="replace", env=env, timeout=600)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln]
    assert all(ln.startswith(("ok ", "refused ")) for ln in lines)
    return {os.path.basename(ln.split()[1].rstrip(":")): ln for ln in lines}


def test_the_core_on_the_cpu_gives_the_reference_frames(harness, tmp_path):
    """jpeg_core.h, walked the way the kernels walk it, computes the numpy statement: every vector, bit for bit"""
    for name in NAMES:
        (tmp_path / name).write_bytes(D.vectors()[name])
    out = _run([harness, str(tmp_path)])
    for name in NAMES:
        assert out[name].startswith("ok ") and "status=0" in out[name] and f"fnv={D.fnv1a(D.expected(name)):08x}" in out[name], out[name]


def test_truncated_and_bit_flipped_streams_end_cleanly(harness, tmp_path):
    """truncations at every kind of place and single-bit flips spread over headers and scan: "ok" (with a scan status) or "refused <reason>",
    never a sanitizer report.  A cut inside the last interval padded with zeros - the damaged frame of the GPU test - is among them."""
    rng = np.random.default_rng(3)
    n = 0
    for name in ("own-17x33", "pil-40x56-restart-blocks-1", "pil-17x33-422", "pil-40x56-420-optimize", "pil-9x23-grey"):
        raw = np.frombuffer(D.vectors()[name], np.uint8)
        scan0 = D.parse(raw.tobytes())["scan"][0]
        for i in range(120):                                                           # half in the headers, half in the scan
            m = raw.copy()
            pos = int(rng.integers(2, scan0)) if i % 2 == 0 else int(rng.integers(scan0, len(raw)))
            m[pos] ^= np.uint8(1 << int(rng.integers(0, 8)))
            (tmp_path / f"{name}_b{i:03d}").write_bytes(m.tobytes())
            n += 1
        for i, cut in enumerate(sorted(set([0, 1, 2, 3, 4, 20, scan0 - 1, scan0, scan0 + 1, len(raw) - 3, len(raw) - 1] + list(range(0, len(raw), max(1, len(raw) // 25)))))):
            (tmp_path / f"{name}_t{i:03d}").write_bytes(raw[:cut].tobytes())
            n += 1
    damaged = D.damaged_frame(D.vectors()["pil-40x56-restart-rows-1"])
    (tmp_path / "damaged").write_bytes(damaged)
    out = _run([harness, str(tmp_path)])
    assert len(out) == n + 1
    assert out["damaged"].startswith("ok ") and "status=0" not in out["damaged"]
    assert f"status={D.decode(damaged, with_status=True)[1]} " in out["damaged"]
    for name, ln in out.items():                                                       # the core and the numpy statement agree on every status
        if ln.startswith("ok ") and "_b" in name:
            data = (tmp_path / name).read_bytes()
            assert f"status={D.decode(data, with_status=True)[1]} " in ln, (name, ln)
    verdicts = [ln.split()[0] for ln in out.values()]
    assert verdicts.count("refused") > 50 and verdicts.count("ok") > 50
    assert sum("status=0" not in ln for ln in out.values() if ln.startswith("ok ")) > 50       # damaged scans that ran to a status


def test_a_frame_of_another_size_is_refused(harness, tmp_path):
    (tmp_path / "a").write_bytes(D.vectors()["own-17x33"])
    assert _run([harness, str(tmp_path), "17", "33"])["a"].startswith("ok ")
    line = _run([harness, str(tmp_path), "33", "17"])["a"]
    assert line.startswith("refused ") and "size 33x17, the handle is for 17x33" in line
    with pytest.raises(D.Refused, match="the handle is for 17x33"):
        D.parse(D.vectors()["own-17x33"], size=(33, 17))


# ---- the AVI reader
def test_avi_reader_on_avi_writer_output(tmp_path):
    from vbt_amd.mjpeg import AviReader, AviWriter
    names = ["pil-40x56-no-restarts", "pil-40x56-restart-rows-1", "pil-40x56-420-optimize"]
    path = tmp_path / "w.avi"
    with AviWriter(str(path), 56, 40, 2997, 100) as w:
        for k in names:
            w.write(D.vectors()[k])
    ref = M.avi_parse(path.read_bytes())
    r = AviReader(str(path))
    assert len(r) == 3 and [r.frame(k) for k in range(3)] == ref["frames"] == [D.vectors()[k] for k in names]
    assert [p - 8 for p, _ in r.chunks] == ref["frame_offsets"]
    assert (r.width, r.height, r.rate, r.scale) == (56, 40, 2997, 100) and r.fps == 29.97 and r.total_frames == 3


def test_avi_reader_without_index_and_with_an_empty_chunk(tmp_path):
    from vbt_amd.mjpeg import AviReader
    a, b = D.vectors()["pil-40x56-no-restarts"], D.vectors()["pil-40x56-restart-rows-1"]
    chunks = [(b"00dc", a), (b"01wb", b"\x01\x02\x03"), (b"00dc", b""), (b"00db", b), (b"01wb", b"")]
    path = tmp_path / "h.avi"
    path.write_bytes(D.build_avi(chunks, 56, 40, rate=60))
    r = AviReader(str(path))
    assert [r.frame(k) for k in range(len(r))] == [a, a, b] and r.fps == 60.0          # the empty chunk repeats the frame before it; audio is skipped
    path.write_bytes(D.build_avi(chunks, 56, 40, rate=60, idx1=True))
    assert [AviReader(str(path)).frame(k) for k in range(3)] == [a, a, b]


def test_files_that_are_not_mjpeg_avi_are_refused_with_the_reason(tmp_path):
    from vbt_amd.mjpeg import AviReader
    good = D.build_avi([(b"00dc", D.vectors()["own-16x16"])], 16, 16)
    cases = {"not-riff": (b"JUNK" + good[4:], "not a RIFF / AVI file"), "wave": (good[:8] + b"WAVE" + good[12:], "not a RIFF / AVI file"),
             "h264": (good.replace(b"MJPG", b"H264"), "not MJPG"), "short": (good[:10], "not a RIFF file"),
             "chunk-past-end": (good[:16] + struct.pack("<I", 1 << 20) + good[20:], "bytes, ")}
    for name, (data, reason) in cases.items():
        path = tmp_path / (name + ".avi")
        path.write_bytes(data)
        with pytest.raises(ValueError, match=reason):
            AviReader(str(path))


def test_cli_refuses_size_and_yuv_with_avi(tmp_path):
    from click.testing import CliRunner
    from vbt_amd.cli import main
    path = tmp_path / "c.avi"
    path.write_bytes(D.build_avi([(b"00dc", D.vectors()["own-16x16"])], 16, 16))
    for extra in (["--size", "16x16"], ["--pix_fmt", "nv12", "--size", "16x16"]):
        res = CliRunner().invoke(main, ["track", str(path)] + extra)
        assert res.exit_code == 2 and "do not apply" in res.output, res.output
