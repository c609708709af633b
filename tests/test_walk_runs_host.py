"""The walk builder of the pipeline's held-back block, host side (no GPU): next_walk_call of vbt_amd/csrc/walk_runs.h turns the per-clip
(slot, frame) lists of a block into the run lists of successive vbt_tracker_update_from_detections_seq calls.  A plain block must give
the one call the deferred small-batch path always launched; the irregular scenarios of tests/test_gpu_step_groups.py (masks, clip maps,
detector-only steps in the middle) are checked for the properties the walk relies on."""
import os
import subprocess

import pytest

from conftest import ROOT

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "walk_runs.h"
// stdin: n_clips, then per clip: fps, count, count x (slot frame).  stdout: one line per call, "clip slot0 stride n frame0 step fps" per run.
int main() {
  int nc = 0;
  if (scanf("%d", &nc) != 1 || nc < 0) return 2;
  std::vector<std::vector<vbt::WalkFrame>> per((size_t)nc);
  std::vector<double> fps((size_t)nc);
  for (int c = 0; c < nc; c++) {
    int cnt = 0;
    if (scanf("%lf %d", &fps[c], &cnt) != 2) return 3;
    for (int j = 0; j < cnt; j++) {
      vbt::WalkFrame f;
      if (scanf("%d %d", &f.slot, &f.frame) != 2) return 4;
      per[c].push_back(f);
    }
  }
  std::vector<size_t> cur((size_t)nc, 0);
  std::vector<vbt_run> runs;
  while (vbt::next_walk_call(per, fps.data(), cur, runs)) {
    for (const vbt_run& r : runs) printf("%d %d %d %d %d %d %.17g;", r.clip, r.slot0, r.slot_stride, r.n_frames, r.frame0, r.frame_step, r.fps);
    printf("\n");
  }
  return 0;
}
"""

N, T, G = 3, 7, 3
FPS = [60.0, 30.0, 23.976]


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    d = tmp_path_factory.mktemp("walk_runs")
    src, exe = d / "walk.cpp", d / "walk"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "vbt_amd", "csrc"), str(src), "-o", str(exe)])

    def run(per, fps=FPS):
        """per[c]: [(slot, frame), ...] -> calls: [[(clip, slot0, stride, n, frame0, step, fps), ...], ...]"""
        text = f"{len(per)}\n" + "".join(f"{fps[c]!r} {len(v)} " + " ".join(f"{s} {f}" for s, f in v) + "\n" for c, v in enumerate(per))
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout
        return [[tuple(int(x) for x in r.split()[:6]) + (float(r.split()[6]),) for r in line.split(";") if r] for line in out.splitlines()]
    return run


def _plain_block(steps, fc0, fstep, fc_base):
    """what a block of plain steps holds: clip c in batch slot c of every step, frame = frame_count - fc_base[c]"""
    return [[(g * N + c, fc0 + g * fstep - fc_base[c]) for g in range(steps)] for c in range(N)]


@pytest.mark.parametrize("fc0,fstep,fc_base", [(1, 1, [0, 0, 0]), (5, 1, [0, 0, 0]), (3, 3, [0, 0, 0]), (9, 1, [0, 4, 7]), (12, 3, [2, 0, 11])])
def test_plain_block_is_one_call(walk, fc0, fstep, fc_base):
    """4 steps x 3 clips: the call {c, c, n, size, fc0 - fc_base[c], fstep, fps[c]} of a deferred group"""
    calls = walk(_plain_block(4, fc0, fstep, fc_base))
    assert calls == [[(c, c, N, 4, fc0 - fc_base[c], fstep, FPS[c]) for c in range(N)]]


def test_single_step_and_empty_block(walk):
    assert walk(_plain_block(1, 7, 1, [0, 0, 0])) == [[(c, c, 1, 1, 7, 1, FPS[c]) for c in range(N)]]
    assert walk([[], [], []]) == []
    assert walk([[], [(1, 4), (4, 5)], []]) == [[(1, 1, 3, 2, 4, 1, FPS[1])]]


def test_broken_patterns_continue_in_further_calls(walk):
    """a block of 5 steps, n = 3: clip 0 misses step 2 and then changes its frame step, clip 1 changes its slot, clip 2 ends after two steps"""
    per = [[(0, 1), (3, 2), (9, 3), (12, 5)],
           [(1, 1), (4, 2), (8, 3), (11, 4), (14, 5)],
           [(2, 4), (5, 5)]]
    assert walk(per) == [[(0, 0, 3, 2, 1, 1, FPS[0]), (1, 1, 3, 2, 1, 1, FPS[1]), (2, 2, 3, 2, 4, 1, FPS[2])],
                         [(0, 9, 3, 2, 3, 2, FPS[0]), (1, 8, 3, 3, 3, 1, FPS[1])]]
    # a frame number that does not increase starts a run of its own (frame step 1, never 0 or negative)
    assert walk([[(0, 5), (3, 5), (6, 4)]], [25.0]) == [[(0, 0, 1, 1, 5, 1, 25.0)], [(0, 3, 1, 1, 5, 1, 25.0)], [(0, 6, 1, 1, 4, 1, 25.0)]]


def _blocks(steps):
    """steps[t]: None (detector only) or [(clip, frame) or None per batch slot]; cut into blocks of G steps as a group=3 pipeline holds
    them -> per block the per-clip (slot, frame) lists"""
    out = []
    for t0 in range(0, len(steps), G):
        per = [[] for _ in range(N)]
        for g, st in enumerate(steps[t0:t0 + G]):
            for i, cf in enumerate(st or []):
                if cf is not None:
                    per[cf[0]].append((g * N + i, cf[1]))
        out.append(per)
    return out


def _masks_steps():
    masks = [[1, 1, 1], [1, 0, 1], [0, 1, 1], [1, 1, 0], [1, 1, 1], [0, 0, 1], [1, 1, 1]]
    seen, steps = [0] * N, []
    for m in masks:
        st = []
        for c in range(N):
            seen[c] += m[c]
            st.append((c, seen[c]) if m[c] else None)
        steps.append(st)
    return steps


def _maps_steps():
    maps = [[0, 1, 2], [2, 0, 1], [2, 0, -1], [1, 2, 0], [0, 1, 2], [0, -1, 2], [1, 0, 2]]
    seen, steps = [0] * N, []
    for m in maps:
        st = []
        for c in m:
            if c >= 0:
                seen[c] += 1
            st.append((c, seen[c]) if c >= 0 else None)
        steps.append(st)
    return steps


def _detector_only_steps():
    return [None if t in (2, 3, 4) else [(c, t + 1) for c in range(N)] for t in range(T)]


def _runs_needed(v):
    """runs the greedy rule cuts a (slot, frame) list into, as index ranges"""
    cuts, a = [], 0
    while a < len(v):
        b = a + 1
        if b < len(v) and v[b][1] > v[a][1]:
            ss, fs = v[b][0] - v[a][0], v[b][1] - v[a][1]
            b += 1
            while b < len(v) and v[b][0] - v[b - 1][0] == ss and v[b][1] - v[b - 1][1] == fs:
                b += 1
        cuts.append((a, b))
        a = b
    return cuts


@pytest.mark.parametrize("scenario", [_masks_steps, _maps_steps, _detector_only_steps])
def test_irregular_blocks(walk, scenario):
    blocks = _blocks(scenario())
    assert len(blocks) == 3
    if scenario is _maps_steps:   # a clip that changes its batch slot does break its pattern inside a block of three
        assert any(len(_runs_needed(v)) > 1 for per in blocks for v in per)
    for per in blocks:
        calls = walk(per)
        got = [[] for _ in range(N)]
        for call in calls:
            assert call, "an empty call"
            clips = [r[0] for r in call]
            assert len(set(clips)) == len(clips) and clips == sorted(clips), "a clip twice in a call"
            for c, slot0, ss, nf, f0, fs, fps in call:
                assert nf >= 1 and fps == FPS[c]
                got[c].append([(slot0 + j * ss, f0 + j * fs) for j in range(nf)])
        for c in range(N):
            # the runs of a clip, concatenated over the calls, are its list: in order and complete
            assert [sf for run in got[c] for sf in run] == per[c], c
            # no run could have taken the next element: the cuts are those of the greedy rule, and a run of one is followed by a frame
            # number that does not increase, a longer one by a change of slot stride or frame step
            assert [len(r) for r in got[c]] == [b - a for a, b in _runs_needed(per[c])], c
            pos = 0
            for r in got[c]:
                nxt = per[c][pos + len(r)] if pos + len(r) < len(per[c]) else None
                if nxt is not None:
                    if len(r) == 1:
                        assert nxt[1] <= r[0][1]
                    else:
                        assert (nxt[0] - r[-1][0], nxt[1] - r[-1][1]) != (r[1][0] - r[0][0], r[1][1] - r[0][1])
                pos += len(r)
        assert len(calls) == max(len(_runs_needed(v)) for v in per)
