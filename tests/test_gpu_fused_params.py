"""The chunk parameters of the fused MBConv tile kernels fetched once per workgroup and handed over through LDS (fused_block.h: PLDS - a
property of the step, on by default wherever the resolved launch is built that way and its tile fits with the parameter area;
VBT_FUSED_PARAMS=0 turns it off, a list such as b1,b4 names the blocks that run it) against the oracle.

A case runs in a child process (the knobs are read once per process): it writes a plan file that puts b1-b4 on the tile kernels
profiles/plan_lite0.b256.f0 pins (9 57 9 57: the diagonal depthwise on 8 x 8 tiles for the two stride-2 blocks, the Toeplitz depthwise on
16 x 8 tiles for the other two) and the first other MBConv block with a part-filled output (Lite0: b5) on the generic matrix-pipe tile
kernel (variant 1, which is not built with the form: its parameter area would cost the CU a workgroup), loads it - the file must load
unchanged - and returns every materialised tensor, the detections and, for every step of the plan that ran, whether it runs the form
(Interpreter.fused_params) and its live-tile count.  Every tensor and every detection must equal the oracle's.

The shapes: b1 has two chunks (the prologue's fetch and the clamped last fetch meet), b4 five; every map has border tiles; the 80 x 80
and 40 x 40 maps of Lite0 are whole tiles of 8 and 16, Lite2's 56 x 56 map is three and a half tiles of 16 wide."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_band_chain import _oracle
from test_gpu_mbconv_toeplitz import clamped  # noqa: F401  (fixture: the narrowed-range model and the oracle's run of it)
from test_gpu_plan_space import LITE2, _lite2_frames, _noise_and_checkerboard

pytestmark = pytest.mark.gpu

PINNED = (9, 57, 9, 57)      # the variants of b1-b4 in profiles/plan_lite0.b256.f0

CHILD = r"""
import os, pickle, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from plan_cover import plan_text, current_plan
from vbt_amd.container import Container
from vbt_amd.interpreter import Interpreter
model, frames, max_batch, choice, prefix = pickle.load(open(sys.argv[1], "rb"))
os.environ.pop("VBT_PLAN_FILE", None)
c = Container(model)
width = lambda e: int(c.tensors[int(c.ops[e["last_op"]]["output"])]["c"])
space = Interpreter(model, max_batch=max_batch, flags=8).plan_space()     # (no autotuning: the groups and alternatives are those of flags 0)
plan = [list(p) for p in current_plan(space)]
alone = lambda e: e["step"] == 0 and sum(1 for x in space if (x["group"], x["alt"]) == (e["group"], e["alt"])) == 1
tiles = [e for e in space if e["family"] == "fused_mbconv" and alone(e)]
support = [e for e in tiles if 33 in e["variants"]]
assert len(support) == len(choice), ([(e["first_op"], e["variants"]) for e in tiles], choice)
for e, v in zip(support, choice):
    assert v in e["variants"], (v, e)
    plan[e["group"]] = [e["alt"], (("fused_mbconv", v),)]
generic = next((e for e in tiles if 33 not in e["variants"] and 1 in e["variants"] and width(e) % 64), None)
if generic:
    plan[generic["group"]] = [generic["alt"], (("fused_mbconv", 1),)]
text = plan_text([(a, tuple(s)) for a, s in plan])
fn = "%s.b%d.f0" % (prefix, max_batch)
open(fn, "w").write(text)
os.environ["VBT_PLAN_FILE"] = prefix
it = Interpreter(model, max_batch=max_batch, flags=0)
assert open(fn).read() == text, "the plan was refused (re-tuned and re-written)"
B = len(frames)
det = it.detect(frames)
ten = {t: it.read_tensor(t, B) for t in range(1, it.num_tensors() - 1) if it.materialized(t)}
ran = [(e["variant"], width(e), it.proj_tail(e["group"], e["alt"], e["step"]), it.fused_params(e["group"], e["alt"], e["step"]))
       for e in it.plan_space() if e["chosen"] and e["family"] == "fused_mbconv"]
other = [it.fused_params(e["group"], e["alt"], e["step"]) for e in it.plan_space() if e["chosen"] and e["family"] != "fused_mbconv"]
assert not any(other), "a step of another family reports the form"
pickle.dump((det, ten, ran), open(sys.argv[2], "wb"))
"""


@pytest.fixture(scope="module")
def frames():
    from vbt_amd import synth
    return np.concatenate([synth.clip_frames(0, 0, 2), _noise_and_checkerboard(320, 31)[:1]])   # two synth frames and noise


@pytest.fixture(scope="module")
def oracle_run(oracle_lib, model_path, frames):
    return _oracle(oracle_lib, model_path, frames)


def _run_case(tmp_path, path, frames, oracle, max_batch, env=None, choice=PINNED):
    """[(variant, output channels, live tiles, form on)] of the fused_mbconv steps of the plan that ran, in graph order, after comparing
    every materialised tensor and the detections with the oracle's"""
    outs, tensors = oracle
    src, dst = str(tmp_path / "in.pkl"), str(tmp_path / "out.pkl")
    with open(src, "wb") as f:
        pickle.dump((path, frames, max_batch, choice, str(tmp_path / "plan")), f)
    drop = ("VBT_NO_KBIAS", "VBT_PLAN_FILE", "VBT_FUSION_FLAGS", "VBT_PROJ_TAIL", "VBT_PW_VARIANT", "VBT_FUSED_PARAMS")
    child_env = {k: v for k, v in os.environ.items() if k not in drop}
    subprocess.run([sys.executable, "-c", CHILD, src, dst], check=True, cwd=ROOT, env={**child_env, **(env or {})}, timeout=300)
    (boxes, scores, classes, counts), ten, ran = pickle.load(open(dst, "rb"))
    assert len(ten) > 60
    for tid, got in ten.items():
        for b in range(len(frames)):
            assert np.array_equal(got[b], tensors[b][tid - 1]), f"tensor {tid} of frame {b} differs under {env}"
    for b in range(len(frames)):
        ob, os_, oc, on = outs[b]
        assert counts[b] == on and np.array_equal(scores[b], os_) and np.array_equal(boxes[b], ob) and np.array_equal(classes[b], oc), (env, b)
    return ran


# b1-b4 on the pinned tile kernels with their live-tile counts and the form; b5 (80 = 64 + one tile) on the generic one, without it
LITE0_ON = [(9, 24, 2, True), (57, 24, 2, True), (9, 40, 3, True), (57, 40, 3, True), (1, 80, 1, False)]


def _only(blocks):
    return [(v, n, ntl, on and i in blocks) for i, (v, n, ntl, on) in enumerate(LITE0_ON)]


def test_lite0_form_on(tmp_path, model_path, frames, oracle_run):
    """Three frames at max_batch 4.  The form is on by default on every block that is built with it."""
    assert _run_case(tmp_path, model_path, frames, oracle_run, 4) == LITE0_ON


def test_lite0_knob_off(tmp_path, model_path, frames, oracle_run):
    """VBT_FUSED_PARAMS=0: the same plan with every wave loading its parameters from global memory."""
    assert _run_case(tmp_path, model_path, frames, oracle_run, 4, {"VBT_FUSED_PARAMS": "0"}) == _only(())


def test_lite0_knob_names_blocks(tmp_path, model_path, frames, oracle_run):
    """VBT_FUSED_PARAMS=b1,b4: those two blocks only."""
    assert _run_case(tmp_path, model_path, frames, oracle_run, 4, {"VBT_FUSED_PARAMS": "b1,b4"}) == _only((0, 3))


def test_lite0_block_major_twins(tmp_path, model_path, frames, oracle_run):
    """With VBT_PROJ_TAIL=0 the launches are block-major: the form runs where it is built block-major too (b1, b3, b4; the Toeplitz
    3x3 kernel on 16 x 8 tiles would lose a wave per SIMD with it and keeps the other form)."""
    got = _run_case(tmp_path, model_path, frames, oracle_run, 4, {"VBT_PROJ_TAIL": "0"})
    assert got == [(v, n, 0, on and i != 1) for i, (v, n, _, on) in enumerate(LITE0_ON)]


def test_without_biased_accumulators(tmp_path, model_path, frames, oracle_run):
    """VBT_NO_KBIAS=1: every stage takes the converting requantisation flavours."""
    assert _run_case(tmp_path, model_path, frames, oracle_run, 4, {"VBT_NO_KBIAS": "1"}) == LITE0_ON


def test_explicit_clamps(tmp_path, frames, clamped):  # noqa: F811
    path, oracle = clamped
    assert _run_case(tmp_path, path, frames, oracle, 4) == LITE0_ON


def test_single_frame(tmp_path, model_path, frames, oracle_run):
    """One frame at max_batch 1."""
    outs, tensors = oracle_run
    assert _run_case(tmp_path, model_path, frames[:1], (outs[:1], tensors[:1]), 1) == LITE0_ON


def test_lite2_bit_exact(tmp_path, oracle_lib):
    """Lite2 at two frames, its six tile-kernel blocks on 9 57 57 9 57 57: 112 x 112 and 56 x 56 maps (seven tiles of 8, three and a half
    of 16: part-filled border tiles), tails of 24 and 48 channels, six chunks on the 288-channel blocks.  The two diagonal blocks and the
    two 3x3 Toeplitz blocks run the form; the 5x5 Toeplitz blocks (48 input channels: a larger tile) would lose a workgroup per CU to
    the parameter area and keep the other form."""
    f2 = _lite2_frames()
    ran = _run_case(tmp_path, LITE2, f2, _oracle(oracle_lib, LITE2, f2), len(f2), None, (9, 57, 57, 9, 57, 57))
    assert [(v, n, on) for v, n, _, on in ran[:6]] == [(9, 24, True), (57, 24, True), (57, 24, True), (9, 48, True), (57, 48, False), (57, 48, False)], ran
    assert not any(on for _, _, _, on in ran[6:]), ran
