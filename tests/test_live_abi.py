"""Live rep analysis, host side (no GPU): the new entry points are exported and declared, and vbt_live_clip as the C compiler lays
it out is the ctypes structure the Python wrappers read."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

LIVE_SYMBOLS = ("vbt_tracker_live_enable", "vbt_tracker_live_poll", "vbt_tracker_live_tracks", "vbt_pipeline_live_enable",
                "vbt_pipeline_live_poll")
HEADER = os.path.join(ROOT, "include", "vbt_hip.h")


def test_live_symbols_are_exported_and_declared():
    from vbt_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    text = open(HEADER).read()
    for name in LIVE_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
        assert re.search(r"\bint " + name + r"\(", text), name


def test_live_clip_layout_matches_ctypes(tmp_path):
    from vbt_amd._lib import LiveClip
    src = tmp_path / "layout.c"
    fields = [f for f, _ in LiveClip._fields_]
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"vbt_hip.h\"\nint main(void) {\n"
                   "  printf(\"size %zu\\n\", sizeof(vbt_live_clip));\n" +
                   "".join(f"  printf(\"{f} %zu\\n\", offsetof(vbt_live_clip, {f}));\n" for f in fields) +
                   "  printf(\"flags %d %d %d\\n\", VBT_LIVE_PATH_FULL, VBT_LIVE_PHASES_FULL, VBT_LIVE_ROWS_LOST);\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(LiveClip) == 32
    for f in fields:
        assert int(out[f]) == getattr(LiveClip, f).offset, f
    from vbt_amd import ocsort
    assert out["flags"].split() == [str(ocsort.LIVE_PATH_FULL), str(ocsort.LIVE_PHASES_FULL), str(ocsort.LIVE_ROWS_LOST)]
