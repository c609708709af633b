"""Slot close and reopen, host side (no GPU): the entry points are exported and declared, vbt_closed_clip as the C compiler lays it out
is the ctypes structure the wrappers read, and the schedule of track_many (shard.stream_schedule) hands out every frame once, in order,
to at most `concurrent` open clips of one resolution at a time."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

RECYCLE_SYMBOLS = ("vbt_tracker_reset_clips", "vbt_pipeline_close_clips_enable", "vbt_pipeline_close_clips", "vbt_pipeline_closed_clip")
HEADER = os.path.join(ROOT, "include", "vbt_hip.h")


def test_recycle_symbols_are_exported_and_declared():
    from vbt_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    text = open(HEADER).read()
    for name in RECYCLE_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
        assert re.search(r"\bint " + name + r"\(", text), name


def test_closed_clip_layout_matches_ctypes(tmp_path):
    from vbt_amd._lib import ClosedClip
    src = tmp_path / "layout.c"
    fields = [f for f, _ in ClosedClip._fields_]
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"vbt_hip.h\"\nint main(void) {\n"
                   "  printf(\"size %zu\\n\", sizeof(vbt_closed_clip));\n" +
                   "".join(f"  printf(\"{f} %zu\\n\", offsetof(vbt_closed_clip, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(ClosedClip) == 24
    for f in fields:
        assert int(out[f]) == getattr(ClosedClip, f).offset, f


def _replay(lengths, concurrent, n_slots, groups):
    """Walks a schedule and checks every rule on the way; returns the frames each clip received, in the order received."""
    from vbt_amd.shard import stream_schedule
    steps = stream_schedule(lengths, concurrent, n_slots, groups=groups)
    got = {c: [] for c in range(len(lengths))}
    open_ = {}                       # slot -> clip
    ever_opened = set()
    for opens, runs, closes in steps:
        for slot, c in opens:
            assert 0 <= slot < concurrent
            assert slot not in open_, "a slot reopens only after its close"
            assert c not in ever_opened, "a clip opens once"
            open_[slot] = c
            ever_opened.add(c)
        assert len(open_) <= concurrent
        assert runs, "every step carries frames"
        assert len({groups[c] for c in open_.values()}) == 1, "clips of different resolutions never share a step"
        slot0 = 0
        for slot, s0, n, f0 in runs:
            assert s0 == slot0 and n >= 1, "runs cover the batch slots 0..B-1 without a hole"
            slot0 += n
            c = open_[slot]
            got[c].extend(range(f0, f0 + n))
        assert slot0 <= n_slots
        assert len({r[0] for r in runs}) == len(runs), "one run per clip and step"
        for slot in closes:
            c = open_.pop(slot)
            assert len(got[c]) == lengths[c], "a clip closes when its frames are used up"
    assert not open_
    return got


@pytest.mark.parametrize("concurrent,n_slots", [(1, 1), (1, 64), (3, 16), (16, 64), (5, 4), (8, 8)])
def test_stream_schedule_hands_out_every_frame_once_in_order(concurrent, n_slots):
    rng = np.random.default_rng(concurrent * 100 + n_slots)
    lengths = [int(x) for x in rng.integers(0, 300, 23)] + [1, 0, 700]
    groups = [("a", "b", "c")[int(x)] for x in rng.integers(0, 3, len(lengths))]
    got = _replay(lengths, concurrent, n_slots, groups)
    for c, n in enumerate(lengths):
        assert got[c] == list(range(1, n + 1)), c


def test_stream_schedule_groups_open_in_order_of_first_appearance():
    from vbt_amd.shard import stream_schedule
    lengths, groups = [10, 20, 5, 7, 9], [(320, 320), (240, 427), (320, 320), (240, 427), (320, 320)]
    order = [c for opens, _, _ in stream_schedule(lengths, 2, 8, groups=groups) for _, c in opens]
    assert order == [0, 2, 4, 1, 3]
    _replay(lengths, 2, 8, groups)


def test_stream_schedule_reuses_the_freed_slot_and_keeps_the_batch_full():
    from vbt_amd.shard import stream_schedule
    steps = stream_schedule([4, 100, 100, 100], 2, 8)
    assert steps[0][0] == [(0, 0), (1, 1)]
    assert steps[0][2] == [0]                       # clip 0 (4 frames) ends in the first step ...
    assert steps[1][0] == [(0, 2)]                  # ... and clip 2 opens in its slot right after
    assert all(sum(r[2] for r in runs) == 8 for _, runs, _ in steps[:-1] if len(runs) == 2)


def test_stream_schedule_refuses_bad_arguments():
    from vbt_amd.shard import stream_schedule
    with pytest.raises(ValueError):
        stream_schedule([3], 0, 4)
    with pytest.raises(ValueError):
        stream_schedule([3], 1, 0)
    with pytest.raises(ValueError):
        stream_schedule([-1], 1, 4)
    assert stream_schedule([], 2, 4) == [] and stream_schedule([0, 0], 2, 4) == []


def test_cli_refuses_live_with_concurrent():
    from click.testing import CliRunner
    from vbt_amd.cli import main
    r = CliRunner().invoke(main, ["track", "--concurrent", "2", "--live", "x.npy"])
    assert r.exit_code == 2 and "--live" in r.output
