"""The owners of device and pinned memory (vbt_amd/csrc/dev_mem.h: DevBuf, PinnedBuf, Mirror) and of HIP events and streams
(vbt_amd/csrc/hip_handles.h: Event, Stream) under -fsanitize=address,undefined: a stand-alone host program
(tests/fuzz/dev_mem_check.cc) with every device hidden, so that each allocation fails as it does on a machine without a GPU.  Checked:
a failed alloc leaves the buffer null, a move leaves the source empty, a Mirror is usable after a failed reserve, a failed create leaves
an event / stream owner empty, empty and moved-from objects destruct cleanly, pinned allocation flags keep the same books, and owners
held in a std::vector (events; a ring slot of a buffer and two events) survive resize, move and destruction.  Nothing loaded into Python is run under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devmem") / "dev_mem_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "fuzz", "dev_mem_check.cc"), "-o", exe])
    return exe


def test_owners_keep_their_books_when_every_allocation_fails(harness):
    # (no leak check: the owners allocate nothing on the host heap, and what the HIP runtime keeps from its own start-up differs by machine)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([harness], capture_output=True, text=True, errors="replace", env=env, timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, (p.stdout[-2000:], p.stderr[-3000:])
    lines = p.stdout.split("\n")[:3]          # "no-device" with the devices hidden; a runtime that shows one anyway gives "allocated"
    assert [ln.rsplit(" ", 1)[0] for ln in lines] == ["ok DevBuf", "ok PinnedBuf", "ok Mirror"], p.stdout
    assert all(ln.endswith((" no-device", " allocated")) for ln in lines), p.stdout
    handles = p.stdout.split("\n")[3:5]       # the event and stream owners: "created" where a device showed
    assert [ln.rsplit(" ", 1)[0] for ln in handles] == ["ok Event", "ok Stream"], p.stdout
    assert all(ln.endswith((" no-device", " created")) for ln in handles), p.stdout
    more = p.stdout.split("\n")[5:7]          # pinned allocation flags; owners as std::vector elements (resize, move, destruction)
    assert [ln.rsplit(" ", 1)[0] for ln in more] == ["ok PinnedBuf-flags", "ok vectors"], p.stdout
    assert more[0].endswith((" no-device", " allocated")) and more[1].endswith((" no-device", " created")), p.stdout
