"""The small-map instantiation of the expand + depthwise kernel (expdw2_block.h: NPGB = XD2S_NPG, variants 300 + chunks per workgroup; two
workgroups resident per CU) and the chunk counts 9 and 18 per workgroup, against the oracle on Lite0's own 10 x 10 blocks (b12-b15:
192 -> 1152 channels, 5 x 5 and 3 x 3 depthwise, stride 1, 18 chunks of 64 channels).

  - max_batch 1, 2 and 3 with three frames: whole and partial batches, and with a per-image grid the image / chunk-group split of blockIdx
    (18 chunks as 3, 2 and 1 workgroups per image; as 4 + 4 + 4 + 4 + 2 with 4 per workgroup: a short last group, whose parameter
    prefetch is clamped to its own last chunk);
  - frames of uniform noise, all 0 and all 255 (on a constant frame every interior pixel of a map holds one value and the border holds the
    zero points: a misplaced tap, position group or output offset changes the first row or column);
  - VBT_NO_KBIAS=1 (the converting requantisation flavours) and the clamped model (the explicitly clamped ones);
  - the 16-wave form at 6 (what the pinned plan ran before), 9 and 18 chunks per workgroup.

Each case runs in a child process: it creates the model once to read its plan space, writes a plan file that puts every step offering
the small-map form on the expand + depthwise alternative with the wanted variant, loads that file and runs.  The case asserts the
variant on the plan that RAN (a refused plan file would be tuned afresh and fail that), that exactly the four 10 x 10 blocks offer the form,
and compares every materialised tensor and the detections with the oracle's."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_band_chain import OP_DW, _oracle
from test_gpu_mbconv_toeplitz import clamped  # noqa: F401  (fixture: the narrowed-range model and the oracle's run of it on `frames`)
from test_gpu_plan_space import _noise_and_checkerboard

pytestmark = pytest.mark.gpu

SMALL = 300   # first variant of the small-map range
CHILD = (
    "import os, pickle, sys, numpy as np\n"
    "sys.path.insert(0, os.path.join(os.getcwd(), 'tests'))\n"
    "from plan_cover import current_plan, plan_text\n"
    "from vbt_amd.interpreter import Interpreter\n"
    "model, frames, max_batch, pin = pickle.load(open(sys.argv[1], 'rb'))\n"
    "it = Interpreter(model, max_batch=max_batch, flags=8)\n"
    "space = it.plan_space()\n"
    "plan = current_plan(space)\n"
    "small = lambda e: e['family'] == 'fused_expand_dw' and any(v >= 300 for v in e['variants'])\n"
    "for g in sorted({e['group'] for e in space if small(e)}):\n"
    "    alt = min(e['alt'] for e in space if e['group'] == g and small(e))\n"
    "    steps = [e for e in space if e['group'] == g and e['alt'] == alt]\n"
    "    plan[g] = (alt, tuple((e['family'], pin if small(e) else e['variant'] if e['variant'] in e['variants'] else e['variants'][0]) for e in steps))\n"
    "prefix = sys.argv[2] + '.plan'\n"
    "open(f'{prefix}.b{max_batch}.f0', 'w').write(plan_text(plan))\n"
    "os.environ['VBT_PLAN_FILE'] = prefix\n"
    "del it\n"
    "it = Interpreter(model, max_batch=max_batch, flags=0)\n"
    "runs = []\n"
    "for i in range(0, len(frames), max_batch):\n"
    "    part = frames[i:i + max_batch]\n"
    "    det = it.detect(part)\n"
    "    runs.append((det, {t: it.read_tensor(t, len(part)) for t in range(1, it.num_tensors() - 1) if it.materialized(t)}))\n"
    "pickle.dump((runs, it.plan_space()), open(sys.argv[2], 'wb'))\n")


@pytest.fixture(scope="module")
def frames():
    return np.concatenate([_noise_and_checkerboard(320, 61)[:1], np.zeros((1, 320, 320, 3), np.uint8), np.full((1, 320, 320, 3), 255, np.uint8)])


@pytest.fixture(scope="module")
def oracle_run(oracle_lib, model_path, frames):
    return _oracle(oracle_lib, model_path, frames)


def _small_steps(path, space, chosen_only):
    """The entries of the plan space that offer the small-map form, with the (h, w, channels) of their depthwise input."""
    from vbt_amd.container import Container
    c = Container(path)
    found = []
    for e in space:
        if e["family"] != "fused_expand_dw" or not any(v >= SMALL for v in e["variants"]) or (chosen_only and not e["chosen"]):
            continue
        dws = [r for r in c.ops[e["first_op"]:e["last_op"] + 1] if int(r["type"]) == OP_DW]
        assert len(dws) == 1
        t = c.tensors[int(dws[0]["inputs"][0])]
        found.append((e, (int(t["h"]), int(t["w"]), int(t["c"]))))
    return found


def _run_case(tmp_path, path, frames, oracle, pin, max_batch, env=None):
    outs, tensors = oracle
    src, dst = str(tmp_path / "in.pkl"), str(tmp_path / "out.pkl")
    with open(src, "wb") as f:
        pickle.dump((path, frames, max_batch, pin), f)
    child_env = {k: v for k, v in os.environ.items() if k not in ("VBT_XD_VARIANT", "VBT_NO_KBIAS", "VBT_PLAN_FILE")}
    subprocess.run([sys.executable, "-c", CHILD, src, dst], check=True, cwd=ROOT, env={**child_env, **(env or {})}, timeout=300)
    runs, space = pickle.load(open(dst, "rb"))
    # the form is offered on the four 10 x 10 blocks and nowhere else, with 6, 9 and 18 chunks per workgroup among its variants ...
    offered = _small_steps(path, space, chosen_only=False)
    assert sorted(shape for _, shape in offered) == [(10, 10, 1152)] * 4, [shape for _, shape in offered]
    for e, _ in offered:
        assert {SMALL + 6, SMALL + 9, SMALL + 18, 206, 209, 218} <= set(e["variants"]), e["variants"]
    # ... and the plan that ran holds the pinned variant on all four
    ran = _small_steps(path, space, chosen_only=True)
    assert len(ran) == 4 and all(e["variant"] == pin for e, _ in ran), [e["variant"] for e, _ in ran]
    assert len(runs) == -(-len(frames) // max_batch)
    for k, ((boxes, scores, classes, counts), ten) in enumerate(runs):
        assert len(ten) > 60
        for j in range(len(counts)):
            b = k * max_batch + j
            for tid, got in ten.items():
                assert np.array_equal(got[j], tensors[b][tid - 1]), f"tensor {tid} of frame {b} differs under variant {pin}, max_batch {max_batch}, {env}"
            ob, os_, oc, on = outs[b]
            assert counts[j] == on and np.array_equal(scores[j], os_) and np.array_equal(boxes[j], ob) and np.array_equal(classes[j], oc), (pin, max_batch, b)


@pytest.mark.parametrize("max_batch, cpw", [(1, 6), (2, 9), (3, 18), (3, 6), (3, 4)], ids=["b1_cpw6", "b2_cpw9", "b3_cpw18", "b3_cpw6", "b3_cpw4_short_group"])
def test_small_map_form(tmp_path, model_path, frames, oracle_run, max_batch, cpw):
    _run_case(tmp_path, model_path, frames, oracle_run, SMALL + cpw, max_batch)


def test_small_map_form_without_biased_accumulators(tmp_path, model_path, frames, oracle_run):
    """VBT_NO_KBIAS=1: both stages take the converting requantisation flavours."""
    _run_case(tmp_path, model_path, frames, oracle_run, SMALL + 9, 2, {"VBT_NO_KBIAS": "1"})


def test_small_map_form_explicit_clamps(tmp_path, frames, clamped):  # noqa: F811
    """The clamped model: the explicitly clamped requantisation flavours."""
    path, oracle = clamped
    _run_case(tmp_path, path, frames, oracle, SMALL + 6, 3)


@pytest.mark.parametrize("max_batch, variant", [(3, 206), (3, 209), (2, 218)], ids=["b3_cpw6", "b3_cpw9", "b2_cpw18"])
def test_sixteen_wave_form_on_the_same_blocks(tmp_path, model_path, frames, oracle_run, max_batch, variant):
    """The general 16-wave form on b12-b15: 6 chunks per workgroup (what ran before, for contrast) and the new 9 and 18."""
    _run_case(tmp_path, model_path, frames, oracle_run, variant, max_batch)
