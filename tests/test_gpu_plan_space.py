"""Every kernel variant a plan file may select, and the pinned plans at their own batch sizes, against the oracle tensor by tensor.

The planner holds that all alternatives and kernel variants compute bit-identical tensors (detector_plan.hip, above candidate_variants), and
the autotuner, tools/tune_under_load.py and the pinned plan files may each pick any of them.  The sweep writes the covering plans of
tests/plan_cover.py as plan files, so every (group, alternative, step, variant) the plan loader accepts runs at least once, and compares
every materialised tensor and every detection with the oracle's.  At flags 0 every kernel family of the library appears in the plan
space of Lite0 and of Lite2 (the sweep asserts it), so none is left out.
"""
import ctypes
import os
import shutil
import time

import numpy as np
import pytest

from conftest import ROOT
from plan_cover import all_tuples, covering_plans, current_plan, parse_plan_text, plan_bound, plan_text, plan_tuples

pytestmark = pytest.mark.gpu

LITE0 = os.path.join(ROOT, "models", "efficientdet_lite0_synth.vbtm")
LITE2 = os.path.join(ROOT, "models", "efficientdet_lite2_synth.vbtm")


def _noise_and_checkerboard(S, seed):
    """Uniform noise and a 1-pixel checkerboard: inputs that drive activations into the saturating ends of their int8 ranges."""
    rng = np.random.Generator(np.random.PCG64(seed))
    chk = ((np.add.outer(np.arange(S), np.arange(S)) & 1) * 255).astype(np.uint8)
    return np.stack([rng.integers(0, 256, (S, S, 3), dtype=np.uint8), np.repeat(chk[:, :, None], 3, axis=2)])


def _lite0_frames():
    """7 frames for a model of max_batch 8 (a partial batch, replayed from the captured graph): 5 synth frames of 3 clips, noise and
    a checkerboard."""
    from vbt_amd import synth
    return np.concatenate([synth.clip_frames(0, 0, 2), synth.clip_frames(1, 11, 2), synth.clip_frames(2, 22, 1), _noise_and_checkerboard(320, 23)])


def _lite2_frames():
    from vbt_amd import synth
    return np.stack([synth.render(synth.background(70 + c, 448), 6 * c) for c in range(2)])


SWEEPS = {"lite0": (LITE0, 8, _lite0_frames), "lite2": (LITE2, 2, _lite2_frames)}


def _oracle_tensors(oracle_lib, path, frames):
    """Per frame: the oracle's detections and every graph tensor (index = tensor id; the input and the raw outputs are None)."""
    det = oracle_lib.OracleDetector(path)
    outs, tensors = [], []
    for f in frames:
        outs.append(det.run(f))
        tensors.append([None] + [det.tensor(t) for t in range(1, det.num_tensors - 1)] + [None])
    return outs, tensors


def _compare_tensors(it, B, want, slots, blame):
    """(tensor id, slot, max |diff|, blamed steps) for every materialised tensor of slots `slots` that differs from want[slot][tid];
    reads one tensor (all B frames) at a time."""
    bad = []
    for tid in range(1, it.num_tensors() - 1):
        if not it.materialized(tid):
            continue
        got = it.read_tensor(tid, B)
        for s in slots:
            if not np.array_equal(got[s], want[s][tid]):
                bad.append((tid, s, int(np.abs(got[s].astype(int) - want[s][tid].astype(int)).max()), blame(tid)))
        del got
    return bad


def _detection_mismatches(got, want, slots):
    boxes, scores, classes, counts = got
    ob, os_, oc, on = want
    return [s for s in slots if not (counts[s] == on[s] and np.array_equal(scores[s], os_[s]) and np.array_equal(boxes[s], ob[s])
                                     and np.array_equal(classes[s], oc[s]))]


def _producers(path):
    from vbt_amd.container import Container
    return {int(r["output"]): i for i, r in enumerate(Container(path).ops)}


def _library_families(it):
    from vbt_amd import _lib
    stats, n = (_lib.KernelStat * 64)(), ctypes.c_int()
    _lib.check(_lib.lib().vbt_model_kernel_stats(it.handle, 1, stats, 64, ctypes.byref(n)))
    return sorted(stats[i].name.decode() for i in range(n.value))


def _space_key(space):
    return [(e["group"], e["alt"], e["step"], e["family"], e["variants"]) for e in space]


@pytest.mark.parametrize("which", ["lite0", "lite2"])
def test_every_variant_of_the_plan_space_bit_exact(which, oracle_lib, tmp_path, monkeypatch):
    """Covering plans at flags 0 (every alternative exists there), each written as a plan file the library must load unchanged, and
    then must report as its plan; every materialised tensor and every detection of every frame equals the oracle's.  A mismatch is
    blamed on the step(s) of the plan that evaluate the op writing the tensor, and all of them are collected before the test fails."""
    from vbt_amd import _lib
    from vbt_amd.interpreter import Interpreter
    path, MB, make = SWEEPS[which]
    frames = make()
    B = len(frames)
    outs, tensors = _oracle_tensors(oracle_lib, path, frames)
    want_det = tuple(np.stack([o[i] for o in outs]) for i in range(4))
    producer = _producers(path)
    t0 = time.time()
    monkeypatch.delenv("VBT_PLAN_FILE", raising=False)
    it0 = Interpreter(path, max_batch=MB, flags=0)
    space = it0.plan_space()
    n, one = ctypes.c_int(), _lib.PlanStepSpace()
    assert _lib.lib().vbt_model_plan_space(it0.handle, ctypes.byref(one), 1, ctypes.byref(n)) == -4 and n.value == len(space)   # never truncated
    assert sorted({e["family"] for e in space}) == _library_families(it0)
    del it0
    plans = covering_plans(space)
    assert 0 < len(plans) <= plan_bound(space)
    prefix = str(tmp_path / "plan")
    monkeypatch.setenv("VBT_PLAN_FILE", prefix)
    fn = f"{prefix}.b{MB}.f0"
    ran, bad = set(), []
    for k, plan in enumerate(plans):
        text = plan_text(plan)
        with open(fn, "w") as f:
            f.write(text)
        it = Interpreter(path, max_batch=MB, flags=0)
        assert open(fn).read() == text, f"plan {k} was refused (re-tuned and re-written)"
        got_space = it.plan_space()
        assert _space_key(got_space) == _space_key(space)
        assert current_plan(got_space) == plan
        chosen = [e for e in got_space if e["chosen"]]

        def blame(tid):
            op = producer.get(tid, -1)
            return [(e["group"], e["alt"], e["step"], e["family"], e["variant"]) for e in chosen if e["first_op"] <= op <= e["last_op"]]

        det = it.detect(frames)
        for tid, s, d, steps in _compare_tensors(it, B, tensors, range(B), blame):
            bad += [(*st, tid, s, d) for st in steps] or [(None, None, None, None, None, tid, s, d)]
        bad += [(k, "detections", s) for s in _detection_mismatches(det, want_det, range(B))]
        ran |= plan_tuples(plan)
        del it
    print(f"\n[plan space] {which}: {len(plans)} covering plans (bound {plan_bound(space)}), {len(ran)} (group, alt, step, variant) tuples "
          f"covered, {time.time() - t0:.1f} s")
    for e in space:
        print(f"  g{e['group']} a{e['alt']} s{e['step']} {e['family']}: {e['variants']}")
    assert not bad, f"{len(bad)} mismatches (group, alt, step, family, variant, tensor id, frame, max|diff|): {sorted(set(bad), key=str)[:60]}"
    assert ran == all_tuples(space)


PINNED = [("plan_lite0", LITE0, 1), ("plan_lite0", LITE0, 8), ("plan_lite0", LITE0, 64), ("plan_lite0", LITE0, 256), ("plan_lite2", LITE2, 64)]


@pytest.mark.parametrize("name,path,B", PINNED, ids=[f"{n}.b{b}" for n, _, b in PINNED])
def test_pinned_plan_bit_exact_at_its_batch(name, path, B, oracle_lib, tmp_path, monkeypatch):
    """The plans bench.py and the tools pin, loaded at their own batch size (grids, split factors and default chunks per workgroup
    differ from the sweep's): the file loads unchanged and is what the model reports; a full batch of distinct frames detects what
    the oracle does in every slot, and every materialised tensor equals the oracle's in slots 0, 1, B/2-1, B/2, B-2 and B-1.  Under
    the Lite0 b64 plan also the batch tails 1, 9 (just above the largest captured graph, 8) and 63."""
    from vbt_amd import synth
    from vbt_amd.interpreter import Interpreter
    pinned = os.path.join(ROOT, "profiles", f"{name}.b{B}.f0")
    raw = open(pinned, "rb").read()
    prefix = str(tmp_path / "plan")
    shutil.copy(pinned, f"{prefix}.b{B}.f0")
    monkeypatch.setenv("VBT_PLAN_FILE", prefix)
    t0 = time.time()
    it = Interpreter(path, max_batch=B, flags=0)
    assert open(f"{prefix}.b{B}.f0", "rb").read() == raw, "the pinned plan was refused (re-tuned and re-written)"
    assert current_plan(it.plan_space()) == parse_plan_text(raw.decode())
    S = int(it.get_input_details()[0]["shape"][1])
    frames = np.stack([synth.render(synth.background(500 + i, S), 3 * i) for i in range(B)])
    if B >= 4:
        frames[B // 2:B // 2 + 2] = _noise_and_checkerboard(S, B)
    det = it.detect(frames)
    want_det = oracle_lib.run_batch(path, frames, threads=16)
    assert not _detection_mismatches(det, want_det, range(B)), f"slots whose detections differ: {_detection_mismatches(det, want_det, range(B))}"
    slots = sorted({s for s in (0, 1, B // 2 - 1, B // 2, B - 2, B - 1) if 0 <= s < B})
    odet = oracle_lib.OracleDetector(path)
    want = {}
    for s in slots:
        odet.run(frames[s])
        want[s] = [None] + [odet.tensor(t) for t in range(1, odet.num_tensors - 1)] + [None]
    bad = _compare_tensors(it, B, want, slots, lambda tid: None)
    assert not bad, f"{len(bad)} tensors differ (tensor id, slot, max|diff|): {[b[:3] for b in bad[:40]]}"
    if (name, B) == ("plan_lite0", 64):
        for tail in (1, 9, 63):
            got = it.detect(frames[:tail])
            assert not _detection_mismatches(got, want_det, range(tail)), (tail, _detection_mismatches(got, want_det, range(tail)))
    print(f"\n[pinned plan] {name}.b{B}: {len(slots)} slots, {time.time() - t0:.1f} s")
