"""The pass of the chained row-band kernels (band_block.h: the depthwise operands rebuilt in registers from the compact array, output
addresses as a scalar base plus 32-bit offsets, the head kernels' problem record in registers and global-address-space loads and
stores) against the oracle, on Lite0's own pyramid levels - the smallest maps at which the kernels can go wrong:

  - 3 x 3 and 5 x 5 levels: bands of one and two pixel groups, the one-unit tail pass, a part-filled pixel group (predicated stores);
  - 18- and 36-channel head outputs: byte stores (18) and dword stores of a part-filled last tile (36); the BiFPN nodes and the
    64 -> 64 head layers: four whole tiles of dwords;
  - 40 x 40 in 240-pixel head bands (15 pixel groups on 8 waves: two-unit passes and a tail) and in 64- / 320-pixel node bands.

Frames: uniform noise, all 0 and all 255 (on a constant frame every interior pixel of a map holds one value and the border holds the
zero points: a misplaced tap or a wrong operand byte changes the first row or column).  Each case runs in a child process (the variant
override is read once per process) and compares every materialised tensor and the detections with the oracle's.

Which form ran: VBT_BAND_VARIANT is applied at launch and the plan space does not report it, so a case that wants a form also PINS it:
the child writes the heuristic plan with every row-band step on that variant, loads it as a plan file and the case asserts that the plan
that ran holds the variant on every row-band step (a refused plan file would be tuned afresh and fail that).  A pinned variant 1 is the
chained form at any batch (detector.hip: resolve_band).  The case without a knob asserts what resolve_band's default rule reads: the plan
leaves the steps at -1, every one of them offers variant 1, and max_batch is above 8."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_band_chain import _band_shapes, _oracle
from test_gpu_mbconv_toeplitz import clamped  # noqa: F401  (fixture: the narrowed-range model and the oracle's run of it on `frames`)
from test_gpu_plan_space import _noise_and_checkerboard

pytestmark = pytest.mark.gpu

CHILD = (
    "import os, pickle, sys, numpy as np\n"
    "sys.path.insert(0, os.path.join(os.getcwd(), 'tests'))\n"
    "from plan_cover import current_plan, plan_text\n"
    "from vbt_amd.interpreter import Interpreter\n"
    "model, frames, max_batch, pin = pickle.load(open(sys.argv[1], 'rb'))\n"
    "it = Interpreter(model, max_batch=max_batch, flags=8)\n"
    "if pin is not None:\n"
    "    plan = [(alt, tuple((fam, pin if fam == 'fused_sepconv_band' else v) for fam, v in steps)) for alt, steps in current_plan(it.plan_space())]\n"
    "    prefix = sys.argv[2] + '.plan'\n"
    "    open(f'{prefix}.b{max_batch}.f0', 'w').write(plan_text(plan))\n"
    "    os.environ['VBT_PLAN_FILE'] = prefix\n"
    "    del it\n"
    "    it = Interpreter(model, max_batch=max_batch, flags=0)\n"
    "runs = []\n"
    "for i in range(0, len(frames), max_batch):\n"
    "    part = frames[i:i + max_batch]\n"
    "    det = it.detect(part)\n"
    "    runs.append((det, {t: it.read_tensor(t, len(part)) for t in range(1, it.num_tensors() - 1) if it.materialized(t)}))\n"
    "pickle.dump((runs, it.plan_space()), open(sys.argv[2], 'wb'))\n")


@pytest.fixture(scope="module")
def frames():
    return np.concatenate([_noise_and_checkerboard(320, 53)[:1], np.zeros((1, 320, 320, 3), np.uint8), np.full((1, 320, 320, 3), 255, np.uint8)])


@pytest.fixture(scope="module")
def oracle_run(oracle_lib, model_path, frames):
    return _oracle(oracle_lib, model_path, frames)


def _run_case(tmp_path, path, frames, oracle, env, max_batch, order=None):
    """Runs frames[order] (default: all, in order) through a model of `max_batch` in a child process, max_batch frames per call.  The form
    VBT_BAND_VARIANT names in `env` is also pinned by a plan file and asserted on the plan that ran."""
    outs, tensors = oracle
    order = list(range(len(frames))) if order is None else order
    src, dst = str(tmp_path / "in.pkl"), str(tmp_path / "out.pkl")
    with open(src, "wb") as f:
        pin = int(env["VBT_BAND_VARIANT"]) if "VBT_BAND_VARIANT" in env else None
        pickle.dump((path, frames[order], max_batch, pin), f)
    child_env = {k: v for k, v in os.environ.items() if k not in ("VBT_BAND_VARIANT", "VBT_BAND_PX", "VBT_NO_KBIAS", "VBT_PLAN_FILE")}
    subprocess.run([sys.executable, "-c", CHILD, src, dst], check=True, cwd=ROOT, env={**child_env, **env}, timeout=300)
    runs, space = pickle.load(open(dst, "rb"))
    # the shapes this file is about are on row bands in the plan that ran
    maps, couts, adds = _band_shapes(path, space)
    assert {(3, 3), (5, 5), (20, 20), (40, 40)} <= maps, maps
    assert {18, 36, 64} <= couts, couts
    assert {1, 2} <= adds, adds
    # the form that ran (see the module docstring)
    bands = [e for e in space if e["chosen"] and e["family"] == "fused_sepconv_band"]
    assert len(bands) >= 10, len(bands)
    if pin is not None:
        assert all(e["variant"] == pin for e in bands), [e["variant"] for e in bands]
    else:
        assert max_batch > 8 and all(e["variant"] == -1 and 1 in e["variants"] for e in bands), [(e["variant"], e["variants"]) for e in bands]
    assert len(runs) == -(-len(order) // max_batch)
    for k, ((boxes, scores, classes, counts), ten) in enumerate(runs):
        assert len(ten) > 60
        for j in range(len(counts)):
            b = order[k * max_batch + j]
            for tid, got in ten.items():
                assert np.array_equal(got[j], tensors[b][tid - 1]), f"tensor {tid} of frame {b} differs under {env}, max_batch {max_batch}"
            ob, os_, oc, on = outs[b]
            assert counts[j] == on and np.array_equal(scores[j], os_) and np.array_equal(boxes[j], ob) and np.array_equal(classes[j], oc), (env, max_batch, b)


def test_chained_form_small_batch(tmp_path, model_path, frames, oracle_run):
    """max_batch 2, the chained form forced (64-pixel node bands): noise + all 0 in one call, all 255 as a partial batch."""
    _run_case(tmp_path, model_path, frames, oracle_run, {"VBT_BAND_VARIANT": "1"}, 2)


def test_chained_form_single_frame(tmp_path, model_path, frames, oracle_run):
    """The same model at max_batch 1: three calls of one frame."""
    _run_case(tmp_path, model_path, frames, oracle_run, {"VBT_BAND_VARIANT": "1"}, 1)


def test_chained_form_without_biased_accumulators(tmp_path, model_path, frames, oracle_run):
    """VBT_NO_KBIAS=1: both stages take the converting requantisation flavours."""
    _run_case(tmp_path, model_path, frames, oracle_run, {"VBT_BAND_VARIANT": "1", "VBT_NO_KBIAS": "1"}, 2)


def test_chained_form_explicit_clamps(tmp_path, frames, clamped):  # noqa: F811
    """The clamped model: the explicitly clamped requantisation flavours."""
    path, oracle = clamped
    _run_case(tmp_path, path, frames, oracle, {"VBT_BAND_VARIANT": "1"}, 2)


def test_default_form_at_batch_12(tmp_path, model_path, frames, oracle_run):
    """max_batch 12 with no knob: the default resolves to the chained form (max_batch > 8), node bands of 320 pixels; twelve frames, the
    three of the oracle run four times over."""
    _run_case(tmp_path, model_path, frames, oracle_run, {}, 12, order=[0, 1, 2, 2, 1, 0, 1, 0, 2, 0, 2, 1])


def test_two_stage_form_untouched(tmp_path, model_path, frames, oracle_run):
    """VBT_BAND_VARIANT=0: the two-stage form, which shares the load stage with the chained one."""
    _run_case(tmp_path, model_path, frames, oracle_run, {"VBT_BAND_VARIANT": "0"}, 2)
