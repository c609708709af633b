"""Where kernels may live under vbt_amd/csrc, as a text scan (no compiler, no GPU):
the detector's host units hold no kernel and no launch, and neither they nor launchers.h / plan_geom.h reach a header with a kernel or a
device builtin; no #include sits inside an open namespace or extern "C" block, so a name's scope never depends on who included a header
first; a header with kernel bodies belongs to exactly one translation unit - but for fused_block.h, whose users are the fused units its
top comment lists; and no *_block.h reaches another."""
import functools
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "vbt_amd", "csrc")
HOST_UNITS = ["detector.hip", "planner.hip", "detector_plan.hip", "detector_profile.hip"]


def _sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".hip")))


def _strip_comments(text):
    """Comments out, string and character literals emptied (an #include's file name and the "C" of extern "C" stay)."""
    text = re.sub(r'extern\s+"C"', "extern_C", text)
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if text.startswith("//", i):
            while i < n and text[i] != "\n":
                i += 1 + (text[i] == "\\" and i + 1 < n)   # (a continued // comment takes the next line with it)
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
            out.append("\n" * text.count("\n", i, j))
            i = j
        elif c in "\"'":
            line_start = text.rfind("\n", 0, i) + 1
            keep = text[line_start:i].lstrip().startswith("#include")
            j = i + 1
            while j < n and text[j] != c and text[j] != "\n":
                j += 1 + (text[j] == "\\")
            out.append(text[i:j + 1] if keep else c + c)
            i = j + 1
        else:
            out.append(c)
            i += 1
    return "".join(out)


@functools.lru_cache(maxsize=None)
def _stripped(name):
    return _strip_comments(open(os.path.join(CSRC, name)).read())


def _logical_lines(text):
    """(line number, text) with backslash continuations joined"""
    lines, buf, start = [], "", 1
    for k, ln in enumerate(text.split("\n"), 1):
        if not buf:
            start = k
        if ln.endswith("\\"):
            buf += ln[:-1] + " "
            continue
        lines.append((start, buf + ln))
        buf = ""
    return lines


def includes_in_open_scope(text):
    """[(line, include line, what is open)] for every #include behind an unclosed `namespace ... {` or `extern "C" {` of a
    comment-stripped text"""
    bad, stack = [], []   # stack: one entry per open brace, the scope's name or None for any other brace
    pending = None        # a namespace / extern "C" head seen, its brace not yet
    for no, ln in _logical_lines(text):
        s = ln.strip()
        if s.startswith("#"):
            if re.match(r"#\s*include\b", s):
                scopes = [x for x in stack if x]
                if scopes:
                    bad.append((no, s, scopes[-1]))
            continue   # (other directives: a macro body's braces are balanced in themselves and open no scope here)
        for tok in re.finditer(r"\bnamespace\b(\s+[\w:]+)?|\bextern_C\b|[{};]", s):
            t = tok.group(0)
            if t == "{":
                stack.append(pending)
                pending = None
            elif t == "}":
                if stack:
                    stack.pop()
            elif t == ";":
                pending = None   # `using namespace x;`, `namespace a = b;`, `extern "C" int f();`
            else:
                pending = " ".join(t.split()).replace("extern_C", 'extern "C"')
    return bad


def _scan(raw):
    return includes_in_open_scope(_strip_comments(raw))


def test_scanner_sees_an_include_inside_a_namespace():
    """the scan itself, on the shapes it must tell apart"""
    assert _scan('namespace vbt {\n#include "a.h"\n}\n') == [(2, '#include "a.h"', "namespace vbt")]
    assert _scan('extern "C" {\nint f();\n#include <b.h>\n}\n')[0][2] == 'extern "C"'
    assert _scan('namespace vbt {\nvoid f() { if (1) { } }\n#include "a.h"\n}  // namespace vbt\n')
    assert _scan('namespace {\n#include "a.h"\n}\n')
    for ok in ('namespace vbt {\nint x;\n}  // namespace vbt\n#include "a.h"\n',
               'using namespace vbt;\n#include "a.h"\n',
               'extern "C" int f(int);\n#include "a.h"\n',
               '// namespace vbt {\n/* extern "C" {\n*/\n#include "a.h"\n',
               'const char* s = "namespace x {";\nchar c = \'{\';\n#include "a.h"\n',
               '#define M(x) do { x; \\\n  } while (0)\nnamespace vbt { }\n#include "a.h"\n'):
        assert _scan(ok) == [], ok


def test_host_units_hold_no_kernel_and_no_launch():
    for name in HOST_UNITS:
        text = _stripped(name)
        assert "__global__" not in text, f"{name} defines a kernel: kernels live in the k_*.hip units"
        assert "<<<" not in text, f"{name} launches a kernel itself: launches go through launchers.h"


def test_no_include_inside_an_open_namespace_or_extern_c():
    bad = {name: includes_in_open_scope(_stripped(name)) for name in _sources()}
    bad = {k: v for k, v in bad.items() if v}
    assert not bad, bad


def _direct_includes(name):
    return [m for m in re.findall(r'^\s*#\s*include\s+"([^"]+)"', _stripped(name), re.M) if os.path.exists(os.path.join(CSRC, m))]


def _closure(name):
    seen, todo = set(), [name]
    while todo:
        for inc in _direct_includes(todo.pop()):
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    return seen


def _device_headers(names):
    return sorted(h for h in names if "__global__" in _stripped(h) or "__builtin_amdgcn_" in _stripped(h))


def test_host_units_and_launchers_reach_no_kernel_header():
    for name in HOST_UNITS + ["launchers.h", "plan_geom.h"]:
        bad = _device_headers(_closure(name))
        assert not bad, f"{name} includes {bad}: argument headers only on the host side"
    assert _device_headers(["dev_common.h", "fused_block.h"]) == ["dev_common.h", "fused_block.h"], "the scan finds no device code at all"


def test_a_header_with_kernels_belongs_to_one_unit():
    units = {u: _closure(u) for u in _sources() if u.endswith(".hip")}
    with_kernels = [h for h in _sources() if h.endswith(".h") and "__global__" in _stripped(h)]
    assert with_kernels, "the scan found no header with a kernel at all"
    assert "fused_block.h" in with_kernels
    for h in with_kernels:
        users = sorted(u for u, inc in units.items() if h in inc)
        if h == "fused_block.h":   # the one kernel header several units instantiate: the units its top comment names
            raw = open(os.path.join(CSRC, h)).read()
            listed = sorted(set(re.findall(r"\bk_\w+\.hip\b", raw[:raw.index("#pragma once")])))
            assert listed and users == listed, f"{h} is reached by {users}, its top comment lists {listed}"
            continue
        assert len(users) == 1, f"{h} holds kernel bodies and is reached by {users or 'no unit'}: exactly one unit may include it"


def test_no_block_header_reaches_another():
    blocks = [h for h in _sources() if h.endswith("_block.h")]
    assert len(blocks) >= 6
    for h in blocks:
        inner = sorted(x for x in _closure(h) if x.endswith("_block.h") and x != h)
        assert not inner, f"{h} includes {inner}"
