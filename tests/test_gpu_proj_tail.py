"""The tile-major part-filled last projection block (pack_weights64_tail) against the oracle: the fused MBConv tile kernels built with a
live-tile count (fused_block.h: NTL - a property of the step, on by default, VBT_PROJ_TAIL=0 turns it off) and variants 9 / 10 of
pw_conv_mfma_i8 (pw_f_kernel with a tile-major last block).

A case runs in a child process (the knobs are read once per process): it writes a plan file that puts b1-b4 on their Toeplitz tile kernels
as profiles/plan_lite0.b256.f0 does (41 57 41 57: 8 x 8 and 16 x 8 tiles; Lite2: 57 where it resolves, else 41) and the first other MBConv block with a part-filled
output (Lite0: b5, 40 -> 80 on 20 x 20) on the generic matrix-pipe tile kernel (variant 1), loads it - the file must load unchanged - and
returns every materialised tensor, the detections and, for every step of the plan that ran, the live-tile count it runs with
(Interpreter.proj_tail).  Every tensor and every detection must equal the oracle's."""
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

PINNED = (41, 57, 41, 57)      # the variants of b1-b4 in profiles/plan_lite0.b256.f0 (9 25 9 25) | 32

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
if choice is None:   # 48-channel chunks on 16 x 8 tiles where they fit, else on 8 x 8
    choice = [57 if 57 in e["variants"] else 41 for e in support]
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
def depth(e):    # input channels of the step's last conv
    convs = [i for i in range(e["first_op"], e["last_op"] + 1) if int(c.ops[i]["type"]) in (1, 2)]
    return int(c.tensors[int(c.ops[convs[-1]]["inputs"][0])]["c"]) if convs else 0
ran = [(e["family"], e["variant"], width(e), depth(e), it.proj_tail(e["group"], e["alt"], e["step"]), e["variants"])
       for e in it.plan_space() if e["chosen"]]
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
    """[(family, variant, output channels, K of the step's last conv, live tiles, offered variants)] of the plan that ran, after comparing
    every materialised tensor and the detections with the oracle's"""
    outs, tensors = oracle
    src, dst = str(tmp_path / "in.pkl"), str(tmp_path / "out.pkl")
    with open(src, "wb") as f:
        pickle.dump((path, frames, max_batch, choice, str(tmp_path / "plan")), f)
    drop = ("VBT_NO_KBIAS", "VBT_PLAN_FILE", "VBT_FUSION_FLAGS", "VBT_PROJ_TAIL", "VBT_PW_VARIANT")
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


def _fused_tails(ran):
    """(variant, output channels, live tiles) of the tile-kernel steps with a part-filled last projection block"""
    return [(v, n, ntl) for fam, v, n, _, ntl, _ in ran if fam == "fused_mbconv" and n % 64]


# b1-b4 on the Toeplitz tile kernels (24, 24, 40, 40 channels: two and three live tiles), b5 (80 = 64 + one tile) on the generic one
LITE0_ON = [(41, 24, 2), (57, 24, 2), (41, 40, 3), (57, 40, 3), (1, 80, 1)]


def test_lite0_form_on(tmp_path, model_path, frames, oracle_run):
    """Three frames at max_batch 4.  The form is on by default: every one of b1-b5 runs with its live-tile count."""
    assert _fused_tails(_run_case(tmp_path, model_path, frames, oracle_run, 4)) == LITE0_ON


def test_lite0_pinned_variants(tmp_path, model_path, frames, oracle_run):
    """b1-b4 exactly as profiles/plan_lite0.b256.f0 pins them (9 57 9 57): the two stride-2 blocks on the diagonal 16x16x64 depthwise, which is
    built with a live-tile count for them too."""
    got = _fused_tails(_run_case(tmp_path, model_path, frames, oracle_run, 4, None, (9, 57, 9, 57)))
    assert got == [(9, 24, 2), (57, 24, 2), (9, 40, 3), (57, 40, 3), (1, 80, 1)]


def test_lite0_knob_off(tmp_path, model_path, frames, oracle_run):
    """VBT_PROJ_TAIL=0: the same plan on the block-major kernels."""
    assert _fused_tails(_run_case(tmp_path, model_path, frames, oracle_run, 4, {"VBT_PROJ_TAIL": "0"})) == [(v, n, 0) for v, n, _ in LITE0_ON]


def test_lite0_knob_names_blocks(tmp_path, model_path, frames, oracle_run):
    """VBT_PROJ_TAIL=b2,b3: those two blocks only."""
    got = _fused_tails(_run_case(tmp_path, model_path, frames, oracle_run, 4, {"VBT_PROJ_TAIL": "b2,b3"}))
    assert got == [(v, n, ntl if i in (1, 2) else 0) for i, (v, n, ntl) in enumerate(LITE0_ON)]


def test_explicit_clamps(tmp_path, frames, clamped):  # noqa: F811
    path, oracle = clamped
    assert _fused_tails(_run_case(tmp_path, path, frames, oracle, 4)) == LITE0_ON


def test_without_biased_accumulators(tmp_path, model_path, frames, oracle_run):
    """VBT_NO_KBIAS=1: every stage takes the converting requantisation flavours."""
    assert _fused_tails(_run_case(tmp_path, model_path, frames, oracle_run, 4, {"VBT_NO_KBIAS": "1"})) == LITE0_ON


def test_single_frame(tmp_path, model_path, frames, oracle_run):
    """One frame at max_batch 1: 100 pixels on the 10 x 10 maps - a partial last pixel group in every projection."""
    outs, tensors = oracle_run
    ran = _run_case(tmp_path, model_path, frames[:1], (outs[:1], tensors[:1]), 1)
    assert _fused_tails(ran) == LITE0_ON


@pytest.mark.parametrize("nframes", [3, 1])
@pytest.mark.parametrize("variant", [9, 10])
def test_forced_pw_tail(tmp_path, model_path, frames, oracle_run, variant, nframes):
    """VBT_PW_VARIANT=9 / 10 on Lite0: the large-K projections of b6-b10 (480 / 672 -> 80 and 112 channels, with and without the residual)
    run the all-blocks form with one and three live tiles in the last block; M = 1200 / 400 pixels on the 20 x 20 maps, neither a
    multiple of 128.  The refusal: where N % 64 == 0 (192, 320) the forced variant leaves the conv on its plan's variant, and the plan
    space does not offer 9 / 10 there."""
    outs, tensors = oracle_run
    ran = _run_case(tmp_path, model_path, frames[:nframes], (outs[:nframes], tensors[:nframes]), nframes, {"VBT_PW_VARIANT": str(variant)})
    big = [(n, k, ntl, offered) for fam, _, n, k, ntl, offered in ran if fam == "pw_conv_mfma_i8" and k > 256 and n > 64]
    assert sorted((n, ntl) for n, _, ntl, _ in big if n % 64) == [(80, 1), (80, 1), (112, 3), (112, 3), (112, 3)], big
    assert len([1 for n, _, ntl, _ in big if n % 64 == 0]) >= 4, big
    for n, _, ntl, offered in big:
        assert (9 in offered and 10 in offered) == bool(n % 64) and (ntl > 0) == bool(n % 64), big
    assert [t[2] for t in _fused_tails(ran)][:4] == [2, 2, 3, 3]


def test_lite2_bit_exact(tmp_path, oracle_lib):
    """Lite2 at two frames: the tile kernels with tails of 24 (two tiles) and 48 channels (three full tiles), and under VBT_PW_VARIANT=10
    the projections to 88 (64 + 24: two tiles), 120 (64 + 56: four tiles, the last part-filled), 208 (3 x 64 + 16) and 352 (5 x 64 + 32)
    channels, and the 352 -> 112 lateral conv of its 112-channel BiFPN (64 + 48: three tiles)."""
    f2 = _lite2_frames()
    ran = _run_case(tmp_path, LITE2, f2, _oracle(oracle_lib, LITE2, f2), len(f2), {"VBT_PW_VARIANT": "10"}, None)
    assert {(n, ntl) for _, n, ntl in _fused_tails(ran) if ntl} == {(24, 2), (48, 3)}, ran
    pw = {(n, ntl) for fam, _, n, k, ntl, _ in ran if fam == "pw_conv_mfma_i8" and k > 256 and ntl}
    assert pw == {(88, 2), (112, 3), (120, 4), (208, 1), (352, 2)}, ran
