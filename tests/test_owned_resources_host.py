"""Every device buffer, pinned buffer, event and stream of the library is made and released by an owner (vbt_amd/csrc/dev_mem.h:
DevBuf, PinnedBuf, Mirror; vbt_amd/csrc/hip_handles.h: Event, Stream), so that a handle's destroy is `delete` and an entry point that
returns early releases what it had made.  This is a plain text scan of vbt_amd/csrc/*.hip and *.h: outside the places listed below, with
one reason each, no line of code calls the runtime's allocation, event-creation or stream-creation functions itself.  Comment lines
and the text of string literals are skipped (error texts name hipMalloc)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbt_amd", "csrc")

TOKENS = ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(", "hipEventCreate", "hipEventDestroy", "hipStreamCreate", "hipStreamDestroy")

# file -> (reason, what a line must contain to be let through; None: the whole file)
ALLOWED = {
    "dev_mem.h": ("the owners of device and pinned memory: the one place that allocates and frees", None),
    "hip_handles.h": ("the owners of events and streams: the one place that creates and destroys them", None),
    "runtime.hip": ("the ABI's own allocation and stream entry points (vbt_host_alloc, vbt_device_alloc, vbt_stream_create and their "
                    "counterparts): what they give belongs to the caller", None),
    "detector_plan.hip": ("the four autotune streams of time_step live for the process: an owner's destructor would run during the "
                          "runtime's teardown", "(void)hipStreamCreateWithFlags(&cs[i], hipStreamNonBlocking)"),
}


def code_of(line):
    """The line without the text of its string and character literals and without a trailing // comment; "" for a comment line."""
    out, i, n = [], 0, len(line)
    while i < n:
        c = line[i]
        if c == "/" and line[i:i + 2] == "//":
            break
        if c in "\"'":
            i += 1
            while i < n and line[i] != c:
                i += 2 if line[i] == "\\" else 1
            i += 1
            out.append(c + c)
            continue
        out.append(c)
        i += 1
    return "".join(out)


def scan(path):
    """[(line number, token, line)] of the raw calls in the code of one file (block comments skipped too)."""
    hits, in_block = [], False
    for no, line in enumerate(open(path, encoding="utf-8", errors="replace").read().split("\n"), 1):
        if in_block:
            if "*/" not in line:
                continue
            line, in_block = line.split("*/", 1)[1], False
        code = code_of(line)
        code = re.sub(r"/\*.*?\*/", "", code)
        if "/*" in code:
            code, in_block = code.split("/*", 1)[0], True
        hits += [(no, t, line.strip()) for t in TOKENS if t in code]
    return hits


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def test_raw_runtime_calls_only_where_listed():
    assert len(sources()) > 20
    bad = []
    for path in sources():
        name = os.path.basename(path)
        for no, token, line in scan(path):
            reason, must = ALLOWED.get(name, (None, "\0"))
            if must is not None and must not in line:
                bad.append("%s:%d: %s    [%s]" % (name, no, line[:140], token))
    assert not bad, "raw allocation / event / stream calls outside the owners:\n" + "\n".join(bad)


def test_the_allow_list_is_alive():
    # every entry still names a file with such a call in it: an entry that outlived its reason goes
    for name, (reason, must) in ALLOWED.items():
        hits = scan(os.path.join(CSRC, name))
        assert reason and hits, name
        if must is not None:
            assert len([h for h in hits if must in h[2]]) == 1, (name, hits)


def test_comments_and_error_texts_are_not_flagged():
    # the scanner itself: code is seen, comments and string literals are not
    assert code_of('  x = hipMalloc(&p, n);  // hipFree( later') == "  x = hipMalloc(&p, n);  "
    assert code_of('  set_error("hipMalloc(%zu) failed: \\"%s\\"", n, s);') == '  set_error("", n, s);'
    assert code_of("  // (fenced) a hipMalloc( here") == "  "
    plan = open(os.path.join(CSRC, "detector_plan.hip"), encoding="utf-8").read().split("\n")
    # the comment in pool_alloc and the error texts of detector_plan.hip mention hipMalloc; neither is code
    mentions = [ln for ln in plan if "hipMalloc" in ln]
    assert any("alignment, like hipMalloc" in ln for ln in mentions) and any("set_error(" in ln for ln in mentions), mentions
    assert all("hipMalloc" not in code_of(ln) for ln in mentions)
    flagged = {h[2] for h in scan(os.path.join(CSRC, "detector_plan.hip"))}
    assert all("(void)hipStreamCreateWithFlags(&cs[i], hipStreamNonBlocking)" in ln for ln in flagged) and len(flagged) == 1, flagged
