"""The band-Toeplitz depthwise of the fused MBConv tile kernels (fused_block.h: TPZ, variant bit 32 of fused_mbconv) against the oracle.

A case runs in a child process: it reads the plan space, writes a plan file that puts every MBConv step able to take the form on its
tile kernel with a variant that has bit 32 set, loads it - the file must load unchanged - and returns every materialised tensor, the
detections and the plan space of the model that ran.  Lite0 at three frames under the mixed assignment covers 8 x 8 and 16 x 8 tiles,
a 40 x 40 map on 16-wide tiles (a partial last tile column), border tiles whose halo lies outside the image, 48- and 64-channel chunks
and one and two K steps in the expand; each case asserts these from the plan space.  The pinned assignment is that of
profiles/plan_lite0.b256.f0.  Lite2 covers 112 x 112 and 56 x 56 maps (seven tiles of 8, three and a half of 16) and its own widths."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_band_chain import _oracle
from test_gpu_plan_space import LITE2, _lite2_frames, _noise_and_checkerboard

pytestmark = pytest.mark.gpu

OP_PW, OP_DW = 2, 3
MIXED = (41, 57, 33, 49)       # b1-b4: 48-channel chunks on 8 x 8 and on 16 x 8 tiles, 64-channel chunks on 8 x 8 and on 16 x 8
PINNED = (41, 57, 41, 57)      # the variants of b1-b4 in profiles/plan_lite0.b256.f0 (9 25 9 25) | 32

CHILD = r"""
import os, pickle, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from plan_cover import plan_text, current_plan
from vbt_amd.interpreter import Interpreter
model, frames, max_batch, choice, prefix = pickle.load(open(sys.argv[1], "rb"))
os.environ.pop("VBT_PLAN_FILE", None)
space = Interpreter(model, max_batch=max_batch, flags=8).plan_space()     # (no autotuning: the groups and alternatives are those of flags 0)
plan = [list(p) for p in current_plan(space)]
support = [e for e in space if e["family"] == "fused_mbconv" and 33 in e["variants"]]
if choice is None:   # 48-channel chunks on 16 x 8 tiles where they fit, else on 8 x 8
    choice = [57 if 57 in e["variants"] else 41 for e in support]
assert len(support) == len(choice), ([(e["first_op"], e["variants"]) for e in space if e["family"] == "fused_mbconv"], choice)
for e, v in zip(support, choice):
    assert e["step"] == 0 and v in e["variants"], (v, e)
    assert not [u for u in e["variants"] if u >= 32 and u not in (33, 41, 49, 57)], e["variants"]
    assert sum(1 for x in space if (x["group"], x["alt"]) == (e["group"], e["alt"])) == 1      # the block is the one step of its alternative
    plan[e["group"]] = [e["alt"], (("fused_mbconv", v),)]
text = plan_text([(a, tuple(s)) for a, s in plan])
fn = "%s.b%d.f0" % (prefix, max_batch)
open(fn, "w").write(text)
os.environ["VBT_PLAN_FILE"] = prefix
it = Interpreter(model, max_batch=max_batch, flags=0)
assert open(fn).read() == text, "the plan was refused (re-tuned and re-written)"
B = len(frames)
det = it.detect(frames)
ten = {t: it.read_tensor(t, B) for t in range(1, it.num_tensors() - 1) if it.materialized(t)}
pickle.dump((det, ten, it.plan_space()), open(sys.argv[2], "wb"))
"""

REFUSAL_CHILD = r"""
import os, pickle, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from plan_cover import plan_text, current_plan
from vbt_amd.interpreter import Interpreter
model, prefix = sys.argv[1], sys.argv[2]
os.environ.pop("VBT_PLAN_FILE", None)
space = Interpreter(model, max_batch=1, flags=8).plan_space()
plan = [list(p) for p in current_plan(space)]
e = next(e for e in space if e["family"] == "fused_mbconv" and 33 not in e["variants"] and e["step"] == 0
         and sum(1 for x in space if (x["group"], x["alt"]) == (e["group"], e["alt"])) == 1)
assert not [u for u in e["variants"] if u >= 32], e["variants"]
plan[e["group"]] = [e["alt"], (("fused_mbconv", 33),)]
text = plan_text([(a, tuple(s)) for a, s in plan])
open(prefix + ".b1.f0", "w").write(text)
os.environ["VBT_PLAN_FILE"] = prefix
it = Interpreter(model, max_batch=1, flags=0)
assert open(prefix + ".b1.f0").read() != text                           # tuned afresh and re-written
assert all(not (x["variant"] & 32) or 33 in x["variants"] for x in it.plan_space() if x["family"] == "fused_mbconv" and x["variant"] >= 0)
"""


@pytest.fixture(scope="module")
def frames():
    from vbt_amd import synth
    return np.concatenate([synth.clip_frames(0, 0, 2), _noise_and_checkerboard(320, 31)[:1]])   # two synth frames and noise


@pytest.fixture(scope="module")
def oracle_run(oracle_lib, model_path, frames):
    return _oracle(oracle_lib, model_path, frames)


@pytest.fixture(scope="module")
def clamped(tmp_path_factory, oracle_lib, model_path, frames):
    """The narrowed-range model of test_gpu_band_chain (the explicit-clamp requantisation flavours) and the oracle's run of it."""
    from step_cases import write_clamped          # the one writer of that container
    path = write_clamped(model_path, str(tmp_path_factory.mktemp("models") / "clamped.vbtm"))
    return path, _oracle(oracle_lib, path, frames)


def _toeplitz_blocks(path, space):
    """The MBConv blocks the plan that ran holds on the Toeplitz form: [(variant, kernel, stride, input channels, (out h, out w))]."""
    from vbt_amd.container import Container
    c = Container(path)
    out = []
    for e in space:
        if e["chosen"] and e["family"] == "fused_mbconv" and e["variant"] >= 32:
            dw = [i for i in range(e["first_op"], e["last_op"] + 1) if int(c.ops[i]["type"]) == OP_DW]
            assert len(dw) == 1 and int(c.ops[dw[0] - 1]["type"]) == OP_PW
            d, t_in, t_out = c.ops[dw[0]], c.tensors[int(c.ops[dw[0] - 1]["inputs"][0])], c.tensors[int(c.ops[dw[0] + 1]["output"])]
            out.append((e["variant"], int(d["k"]), int(d["stride"]), int(t_in["c"]), (int(t_out["h"]), int(t_out["w"]))))
    return out


def _run_case(tmp_path, path, frames, oracle, choice, max_batch, env=None):
    outs, tensors = oracle
    src, dst = str(tmp_path / "in.pkl"), str(tmp_path / "out.pkl")
    with open(src, "wb") as f:
        pickle.dump((path, frames, max_batch, choice, str(tmp_path / "plan")), f)
    child_env = {k: v for k, v in os.environ.items() if k not in ("VBT_NO_KBIAS", "VBT_PLAN_FILE", "VBT_FUSION_FLAGS")}
    subprocess.run([sys.executable, "-c", CHILD, src, dst], check=True, cwd=ROOT, env={**child_env, **(env or {})}, timeout=300)
    (boxes, scores, classes, counts), ten, space = pickle.load(open(dst, "rb"))
    blocks = _toeplitz_blocks(path, space)
    assert blocks and (choice is None or [b[0] for b in blocks] == list(choice)), blocks       # every block ran the form it was given
    assert len(ten) > 60
    for tid, got in ten.items():
        for b in range(len(frames)):
            assert np.array_equal(got[b], tensors[b][tid - 1]), f"tensor {tid} of frame {b} differs under {choice}, {env}"
    for b in range(len(frames)):
        ob, os_, oc, on = outs[b]
        assert counts[b] == on and np.array_equal(scores[b], os_) and np.array_equal(boxes[b], ob) and np.array_equal(classes[b], oc), (choice, env, b)
    return blocks


def _assert_lite0_shapes(blocks, chunks=(False, True)):
    """What the Lite0 cases are about, read from the plan that ran (variant bit 16: 16 x 8 tiles, bit 8: 48-channel chunks)."""
    assert {(k, s) for _, k, s, _, _ in blocks} == {(3, 1), (3, 2), (5, 1), (5, 2)}, blocks
    assert {bool(v & 16) for v, *_ in blocks} == {False, True}, blocks                       # 8 x 8 and 16 x 8 tiles
    assert any(v & 16 and hw == (40, 40) for v, _, _, _, hw in blocks), blocks               # 40 = 2.5 tiles of 16: a partial last column
    assert {bool(v & 8) for v, *_ in blocks} == set(chunks), blocks                          # 48- and 64-channel chunks
    assert {(cin + 31) // 32 for _, _, _, cin, _ in blocks} == {1, 2}, blocks                # K steps of the expand
    assert all(hw[0] % 8 == 0 for *_, hw in blocks)                                          # (every map has border tiles; rows are whole tiles)


@pytest.mark.parametrize("choice", [MIXED, PINNED], ids=["mixed", "pinned"])
def test_lite0_bit_exact(tmp_path, model_path, frames, oracle_run, choice):
    _assert_lite0_shapes(_run_case(tmp_path, model_path, frames, oracle_run, choice, len(frames)), (False, True) if choice is MIXED else (True,))


def test_lite2_bit_exact(tmp_path, oracle_lib):
    f2 = _lite2_frames()
    blocks = _run_case(tmp_path, LITE2, f2, _oracle(oracle_lib, LITE2, f2), None, len(f2))
    assert {(112, 112), (56, 56)} <= {hw for *_, hw in blocks}, blocks
    assert {cin for _, _, _, cin, _ in blocks} == {16, 24, 48}, blocks
    assert any(v & 16 and hw == (56, 56) for v, _, _, _, hw in blocks), blocks


def test_explicit_clamps(tmp_path, frames, clamped):
    path, oracle = clamped
    _assert_lite0_shapes(_run_case(tmp_path, path, frames, oracle, MIXED, len(frames)))


def test_without_biased_accumulators(tmp_path, model_path, frames, oracle_run):
    """VBT_NO_KBIAS=1: no conv starts its accumulators at bias + 0x4B400000, every stage takes the converting flavours."""
    _assert_lite0_shapes(_run_case(tmp_path, model_path, frames, oracle_run, MIXED, len(frames), {"VBT_NO_KBIAS": "1"}))


def test_partial_batch(tmp_path, model_path, frames, oracle_run):
    """max_batch 4 running three frames: the grids are those of the frames given."""
    _assert_lite0_shapes(_run_case(tmp_path, model_path, frames, oracle_run, MIXED, 4))


def test_refused_where_the_step_cannot_take_it(tmp_path, model_path):
    """Lite0's later blocks expand from 80 and more channels (three K steps): 33 does not resolve there, so a plan file naming it is
    refused with the loader's usual message and the model tuned afresh."""
    child_env = {k: v for k, v in os.environ.items() if k not in ("VBT_PLAN_FILE", "VBT_FUSION_FLAGS")}
    p = subprocess.run([sys.executable, "-c", REFUSAL_CHILD, model_path, str(tmp_path / "plan")], cwd=ROOT, env=child_env, timeout=300,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "variant 33 is not one the planner offers for this step - plan refused, re-tuning" in p.stderr, p.stderr[-3000:]
