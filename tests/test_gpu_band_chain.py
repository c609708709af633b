"""The two forms of the row-band SeparableConv kernels (band_block.h) against the oracle: depthwise and projection as two stages around an
LDS tile (VBT_BAND_VARIANT=0) and chained through registers (1), forced through the test-only override (read once per process, hence a
child process per case).  Lite0's own pyramid levels are the smallest shapes at which the kernels can go wrong, and every case asserts
that the plan it ran holds them on row bands: 3x3 (one partial pixel group), 5x5 (a pixel group straddling rows), 20x20 in 64-pixel
bands (a short last band), 40x40 in 320-pixel bands (20 pixel groups on 16 waves), 18 and 36 output channels (partial output tiles) and
BiFPN nodes with two and with three sources."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from plan_cover import current_plan, plan_text
from test_gpu_plan_space import LITE2, _noise_and_checkerboard

pytestmark = pytest.mark.gpu

OP_PW, OP_DW, OP_ADD = 2, 3, 4

CHILD = (
    "import pickle, sys, numpy as np\n"
    "from vbt_amd.interpreter import Interpreter\n"
    "model, frames, max_batch, flags = pickle.load(open(sys.argv[1], 'rb'))\n"
    "B = len(frames)\n"
    "it = Interpreter(model, max_batch=max_batch, flags=flags)\n"
    "det = it.detect(frames)\n"
    "ten = {t: it.read_tensor(t, B) for t in range(1, it.num_tensors() - 1) if it.materialized(t)}\n"
    "pickle.dump((det, ten, it.plan_space()), open(sys.argv[2], 'wb'))\n")


@pytest.fixture(scope="module")
def frames():
    from vbt_amd import synth
    return np.concatenate([synth.clip_frames(0, 0, 2), _noise_and_checkerboard(320, 31)[:1]])   # two synth frames and noise


def _oracle(oracle_lib, path, frames):
    det = oracle_lib.OracleDetector(path)
    outs, tensors = [], []
    for f in frames:
        outs.append(det.run(f))
        tensors.append([det.tensor(t) for t in range(1, det.num_tensors - 1)])
    return outs, tensors


@pytest.fixture(scope="module")
def oracle_run(oracle_lib, model_path, frames):
    return _oracle(oracle_lib, model_path, frames)


@pytest.fixture(scope="module")
def clamped(tmp_path_factory, oracle_lib, model_path, frames):
    """The narrowed-range model of test_gpu_detector.test_explicit_clamps_bit_exact (the explicit-clamp requantisation flavours) and
    the oracle's run of it."""
    from step_cases import write_clamped          # the one writer of that container
    path = write_clamped(model_path, str(tmp_path_factory.mktemp("models") / "clamped.vbtm"))
    return path, _oracle(oracle_lib, path, frames)


def _band_shapes(path, space):
    """What the chosen plan runs on row bands: {(h, w) of the maps}, {output channels}, {ADDs in front of a one-problem step}."""
    from vbt_amd.container import Container
    c = Container(path)
    chosen = [e for e in space if e["chosen"]]
    maps, couts, adds = set(), set(), set()
    for i, r in enumerate(c.ops):
        if int(r["type"]) != OP_DW:
            continue
        owners = [e for e in chosen if e["first_op"] <= i <= e["last_op"]]
        if not owners or any(e["family"] != "fused_sepconv_band" for e in owners):
            continue
        assert int(c.ops[i + 1]["type"]) == OP_PW
        t = c.tensors[int(r["inputs"][0])]
        maps.add((int(t["h"]), int(t["w"])))
        couts.add(int(c.tensors[int(c.ops[i + 1]["output"])]["c"]))
    producer = {int(r["output"]): i for i, r in enumerate(c.ops)}
    is_add = lambda i: int(c.ops[i]["type"]) == OP_ADD
    covered = lambda i: any(e["first_op"] <= i <= e["last_op"] for e in chosen)
    for e in chosen:
        if e["family"] == "fused_sepconv_band" and e["last_op"] - e["first_op"] <= 3:   # one problem: [ADD] depthwise pointwise
            n = 0
            for i in range(e["first_op"], e["last_op"] + 1):
                if is_add(i):
                    n += 1
                    # a three-source node: the first of its two chained ADDs is evaluated inside the step too (its output never reaches
                    # HBM), and no step of the plan names it
                    srcs = [producer.get(int(t)) for t in c.ops[i]["inputs"][:int(c.ops[i]["n_inputs"])]]
                    n += sum(j is not None and is_add(j) and not covered(j) for j in srcs)
            adds.add(n)
    return maps, couts, adds


def _run_case(tmp_path, path, frames, oracle, env, flags, max_batch, px):
    outs, tensors = oracle
    src, dst = str(tmp_path / "in.pkl"), str(tmp_path / "out.pkl")
    with open(src, "wb") as f:
        pickle.dump((path, frames, max_batch, flags), f)
    child_env = {k: v for k, v in os.environ.items() if k not in ("VBT_BAND_VARIANT", "VBT_BAND_PX", "VBT_NO_KBIAS", "VBT_PLAN_FILE")}
    subprocess.run([sys.executable, "-c", CHILD, src, dst], check=True, cwd=ROOT, env={**child_env, **env}, timeout=300)
    (boxes, scores, classes, counts), ten, space = pickle.load(open(dst, "rb"))
    # the shapes this case is about are in the plan that ran
    maps, couts, adds = _band_shapes(path, space)
    assert {(3, 3), (5, 5), (20, 20), (40, 40)} <= maps, maps
    assert {18, 36, 64} <= couts, couts
    assert adds == {0} if flags & 16 else {1, 2} <= adds, adds         # plain inputs (no node fusion); nodes of two and of three sources
    # What VBT_BAND_PX makes of those maps.  The plan space does not report rows or bands, so this is NOT read from the launch that ran:
    # it restates make_band's formula for the one-problem (node) bands - ceil(h * w / px) bands of ceil(h / bands) rows, 16 waves - and
    # says why the two band sizes are the cases.  The head grids take their rows from BD_HEAD_MAXPX = 240 whatever VBT_BAND_PX says
    # (40x40: 7 bands of 6 rows = 15 pixel groups on 8 waves and a 4-row last band; 20x20: 2 bands of 10 rows = 13 pixel groups).
    rows = lambda h, w: -(-h // max(1, -(-h * w // px)))
    if px == 64:
        assert 20 % rows(20, 20) != 0                                     # a short last band
    else:
        assert (rows(40, 40) * 40 // 16) % 16 != 0                        # pixel groups not divisible by the sixteen waves
    assert len(ten) > 60
    for tid, got in ten.items():
        for b in range(len(frames)):
            assert np.array_equal(got[b], tensors[b][tid - 1]), f"tensor {tid} of frame {b} differs under {env}, flags {flags}"
    for b in range(len(frames)):
        ob, os_, oc, on = outs[b]
        assert counts[b] == on and np.array_equal(scores[b], os_) and np.array_equal(boxes[b], ob) and np.array_equal(classes[b], oc), (env, flags, b)


@pytest.mark.parametrize("px", [64, 320])
@pytest.mark.parametrize("flags", [8, 8 | 16])
@pytest.mark.parametrize("variant", [0, 1])
def test_both_band_forms_bit_exact(tmp_path, model_path, frames, oracle_run, variant, flags, px):
    _run_case(tmp_path, model_path, frames, oracle_run, {"VBT_BAND_VARIANT": str(variant), "VBT_BAND_PX": str(px)}, flags, len(frames), px)


def test_chained_form_without_biased_accumulators(tmp_path, model_path, frames, oracle_run):
    """VBT_NO_KBIAS=1: no conv starts its accumulators at bias + 0x4B400000, both stages take the converting flavours."""
    _run_case(tmp_path, model_path, frames, oracle_run, {"VBT_BAND_VARIANT": "1", "VBT_BAND_PX": "320", "VBT_NO_KBIAS": "1"}, 8, len(frames), 320)


def test_chained_form_explicit_clamps(tmp_path, frames, clamped):
    path, oracle = clamped
    _run_case(tmp_path, path, frames, oracle, {"VBT_BAND_VARIANT": "1", "VBT_BAND_PX": "64"}, 8, len(frames), 64)


def test_chained_form_partial_batch(tmp_path, model_path, frames, oracle_run):
    """max_batch 4 running three frames: the grids are those of the frames given."""
    _run_case(tmp_path, model_path, frames, oracle_run, {"VBT_BAND_VARIANT": "1", "VBT_BAND_PX": "320"}, 8, 4, 320)


def test_chained_form_is_refused_on_lite2(tmp_path, monkeypatch, capfd):
    """The chained form is built for 64-channel maps: on Lite2's 112-channel steps variant 1 does not resolve, so a plan file naming it
    is refused with the loader's usual message and the model tuned afresh."""
    from vbt_amd.interpreter import Interpreter
    monkeypatch.delenv("VBT_PLAN_FILE", raising=False)
    monkeypatch.delenv("VBT_BAND_VARIANT", raising=False)
    space = Interpreter(LITE2, max_batch=1, flags=8).plan_space()       # (no autotuning: the groups and alternatives are those of flags 0)
    bands = [e for e in space if e["family"] == "fused_sepconv_band"]
    assert bands and all(1 not in e["variants"] and 0 in e["variants"] for e in bands)
    plan = current_plan(space)
    g = next(e["group"] for e in space if e["chosen"] and e["family"] == "fused_sepconv_band")
    alt, steps = plan[g]
    plan[g] = (alt, tuple((fam, 1 if fam == "fused_sepconv_band" else v) for fam, v in steps))
    prefix = str(tmp_path / "plan")
    text = plan_text(plan)
    with open(f"{prefix}.b1.f0", "w") as f:
        f.write(text)
    monkeypatch.setenv("VBT_PLAN_FILE", prefix)
    capfd.readouterr()
    it = Interpreter(LITE2, max_batch=1, flags=0)
    err = capfd.readouterr().err
    assert "variant 1 is not one the planner offers for this step - plan refused, re-tuning" in err, err
    assert open(f"{prefix}.b1.f0").read() != text                        # tuned afresh and re-written
    assert all(e["variant"] != 1 for e in it.plan_space() if e["family"] == "fused_sepconv_band")


def test_override_does_not_widen_the_plan_space(tmp_path, model_path):
    """The requested variant is judged before VBT_BAND_VARIANT is applied: with the override set to 0 (which every step can run) Lite2's
    steps still do not offer the chained form, and Lite0's offer both."""
    code = ("import pickle, sys\n"
            "from vbt_amd.interpreter import Interpreter\n"
            "out = [[e['variants'] for e in Interpreter(p, max_batch=1, flags=8).plan_space() if e['family'] == 'fused_sepconv_band'] for p in sys.argv[2:]]\n"
            "pickle.dump(out, open(sys.argv[1], 'wb'))\n")
    dst = str(tmp_path / "space.pkl")
    subprocess.run([sys.executable, "-c", code, dst, LITE2, model_path], check=True, cwd=ROOT, env={**os.environ, "VBT_BAND_VARIANT": "0"}, timeout=300)
    lite2, lite0 = pickle.load(open(dst, "rb"))
    assert lite2 and all(sorted(v) == [-1, 0] for v in lite2), lite2
    assert lite0 and all(sorted(v) == [-1, 0, 1] for v in lite0), lite0
