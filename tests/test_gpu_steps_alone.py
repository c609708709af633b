"""Every plan step but decode + NMS run ALONE on crafted int8 tensors, against the exact numpy evaluator of tests/graph_ref.py.

The other detector tests feed frames into the top of the network, so a kernel only ever reads what the layers above it produce, and a
whole forward overwrites every tensor, so nothing shows what a launch must not write.  Here the patterns of tests/step_cases.py (U:
uniform bytes, S: rails, X: extremes aligned with the consumer's weights / the whole (a, b) grid of an ADD) are written into every
materialised tensor (Interpreter.write_tensor), one plan step runs (Interpreter.run_steps), and the tensors are read back:

  * every tensor the step changed equals graph_ref.reference(tensor, state after the step) bit for bit in every image - the producer of
    the tensor evaluated on the materialised tensors as they stand, recursing through tensors that live only inside a fused kernel;
  * over the plan the sets of changed tensors are pairwise disjoint and their union is every materialised tensor but the graph input:
    a tensor no step wrote, or two steps wrote, fails;
  * containment: the step re-run on images (0, 2) and (1, 1) leaves the other image slots as they were written and computes the same
    bytes inside; a step that runs from image 0 only answers VBT_ERR_ARG for image 1 and changes nothing; in the fused plans EVERY
    materialised tensor is read back after every run (a store past the step's own images or into another tensor's slot shows), in the
    one-kernel-per-op plan the step's own outputs and the tensors next to them in tensor id.

What the patterns reach - accumulators at the attainable extremes, saturating partial sums, all 65 536 ADD pairs, both rails - is
asserted on the reference alone in tests/test_graph_ref_host.py.  A changed tensor is restored before the next step, so every step
reads patterns only.  Mismatches of all steps are collected before the test fails, as in test_gpu_plan_space.py.
"""
import os
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_ref as gr  # noqa: E402
import step_cases as sc  # noqa: E402
from plan_cover import covering_plans, current_plan, plan_text, plan_tuples  # noqa: E402

pytestmark = pytest.mark.gpu

LITE0 = os.path.join(ROOT, "models", "efficientdet_lite0_synth.vbtm")
LITE2 = os.path.join(ROOT, "models", "efficientdet_lite2_synth.vbtm")
PARTS = ("backbone", "fpn", "head")
ENV_KEYS = ("VBT_NO_KBIAS", "VBT_PLAN_FILE", "VBT_FUSION_FLAGS", "VBT_NO_PW_MERGE", "VBT_PROJ_TAIL", "VBT_FUSED_PARAMS", "VBT_PW_VARIANT",
            "VBT_BAND_VARIANT", "VBT_BAND_PX", "VBT_XD_VARIANT", "VBT_SUBSTREAMS")

# name -> (model, max_batch, flags, environment, patterns)
CONFIGS = {
    "lite0-f1": ("lite0", 3, 1, {}, "USX"),                          # every op alone: every op gets crafted inputs directly
    "lite0-f8": ("lite0", 3, 8, {}, "USX"),
    "lite0-f8-noexpdw-noband": ("lite0", 3, 8 | 4096 | 8192, {}, "USX"),
    "lite0-f8-nombconv": ("lite0", 3, 8 | 2, {}, "USX"),
    "lite0-f8-nonode": ("lite0", 3, 8 | 16, {}, "USX"),
    "lite0-f8-nokbias": ("lite0", 3, 8, {"VBT_NO_KBIAS": "1"}, "XS"),
    "clamped-f8": ("clamped", 3, 8, {}, "US"),
    "lite2-f8": ("lite2", 2, 8, {}, "UX"),                           # channel counts that are no multiples of 64
    # step_cases.write_kb_edge: accumulators at +-(2^22 - 2), the edge of the range the RQ_KBIAS proof covers - under X where the conv's
    # input is materialised, under S (all-high block inputs through saturating expand channels) inside the fused MBConv kernels
    "kbedge-f1": ("kb_edge", 3, 1, {}, "XS"),
    "kbedge-f8": ("kb_edge", 3, 8, {}, "XS"),
    "kbedge-f8-noexpdw-noband": ("kb_edge", 3, 8 | 4096 | 8192, {}, "XS"),
    "kbedge-f8-nombconv": ("kb_edge", 3, 8 | 2, {}, "XS"),
}
CASES = [(n, p) for n in CONFIGS for p in PARTS if not (n.startswith("kbedge") and p != "backbone")]   # (the edge convs are MBConv convs)


@pytest.fixture(scope="module")
def model_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("steps_alone")
    return {"lite0": LITE0, "lite2": LITE2, "clamped": sc.write_clamped(LITE0, str(d / "clamped.vbtm")),
            "kb_edge": sc.write_kb_edge(LITE0, str(d / "kb_edge.vbtm"))[0]}


_graphs = {}


def _graph(path, B):
    """(GraphRef, Cases, stage of every op) of a model file, shared by the tests of the module"""
    if (path, B) not in _graphs:
        from vbt_amd import spec
        g = gr.GraphRef(path)
        names = spec.build_graph(int(g.c.header["arch"]))
        assert len(names.ops) == g.n_ops
        _graphs[(path, B)] = (g, sc.Cases(g, B), [op.stage for op in names.ops])
    return _graphs[(path, B)]


def _frontier(g, tid, held, out):
    """the materialised tensors reference(tid, ...) reads"""
    for t in g.inputs(g.producer[tid]):
        if t == g.input_tensor or t in held:
            out.add(t)
        else:
            _frontier(g, t, held, out)
    return out


def _first_diff(got, want):
    d = np.argwhere(got != want)
    return tuple(int(v) for v in d[0]), len(d), int(np.abs(got.astype(int) - want.astype(int)).max())


class Runner:
    """One model instance under one pattern at a time: the device tensors and their host copies"""

    def __init__(self, it, g, cases, stages, wide, ref_cache=None):
        self.it, self.g, self.cases, self.stages, self.wide = it, g, cases, stages, wide
        self.B = it.max_batch
        nt = it.num_tensors()
        self.held = [t for t in range(1, nt - 1) if it.materialized(t)]            # (0: the graph input; nt - 1: the detections)
        self.steps = it.plan_steps()
        assert len(self.steps) == it.num_launches() and self.steps[-1]["family"] == "decode_nms"
        placed = [(s["group"], s["step"]) for s in self.steps if s["group"] >= 0]
        assert len(set(placed)) == len(placed), "two steps of the execution list claim one place in the plan space"
        self.ref_cache = {} if ref_cache is None else ref_cache
        self.bad, self.written, self.runs = [], {}, 0

    def part(self, i):
        return self.stages[self.steps[i]["last_op"]]

    def load(self, pattern):
        self.pattern = pattern
        self.state = {t: self.cases.tensor(t, pattern) for t in self.held}
        for t, a in self.state.items():
            self.it.write_tensor(t, a)
        self.frames = self.cases.tensor(self.g.input_tensor, pattern)

    def probe(self, i):
        if self.wide:
            return self.held
        s = self.steps[i]
        outs = {self.g.output(o) for o in range(s["first_op"], s["last_op"] + 1)}
        near = {t + d for t in outs for d in (-1, 0, 1)}
        return [t for t in self.held if t in near]

    def _run(self, i, img0, n):
        """-> every probed tensor as read back, and the ones among them that differ from what was written"""
        s = self.steps[i]
        self.it.run_steps(i, i + 1, img0, n, frames=self.frames[img0:img0 + n] if s["reads_frames"] else None)
        self.runs += 1
        return self._read(i)

    def _read(self, i):
        got = {t: self.it.read_tensor(t, self.B) for t in self.probe(i)}
        return got, {t: a for t, a in got.items() if not np.array_equal(a, self.state[t])}

    def _restore(self, changed):
        for t in changed:
            self.it.write_tensor(t, self.state[t])

    def _reference(self, t, changed):
        post = dict(self.state)
        post.update(changed)
        front = _frontier(self.g, t, set(self.held), set())
        key = (t, self.pattern, tuple(sorted(front))) if not front & set(changed) else None
        if key is None or key not in self.ref_cache:
            ref = self.g.reference(t, post, self.frames)
            if key is None:
                return ref
            self.ref_cache[key] = ref
        return self.ref_cache[key]

    def step(self, i):
        """The step's outputs are the tensors it changed under this pattern or an earlier one (under S a result can equal the rail that
        was written; no model starts with S): all of them must equal the reference, changed or not."""
        s = self.steps[i]
        tag = (i, s["family"], s["variant"], self.pattern)
        got, full = self._run(i, 0, self.B)
        outs = self.written.setdefault(i, set())
        outs.update(full)
        if not outs:
            self.bad.append((*tag, "changed no tensor"))
        for t in sorted(outs):
            want = self._reference(t, full)
            for b in range(self.B):
                if not np.array_equal(got[t][b], want[b]):
                    self.bad.append((*tag, "tensor", t, "image", b, "first (y, x, c), count, max|diff|", *_first_diff(got[t][b], want[b])))
        self._restore(full)
        for img0, n in ((0, 2), (1, 1)):
            if img0 + n > self.B or n == self.B:
                continue
            rng = f"images {img0}..{img0 + n - 1}"
            if img0 and s["image0_only"]:
                from vbt_amd._lib import VbtArgError
                try:
                    _, part = self._run(i, img0, n)
                    self.bad.append((*tag, rng, "an image-0-only step did not answer VBT_ERR_ARG"))
                except VbtArgError:
                    _, part = self._read(i)
                    if part:
                        self.bad.append((*tag, rng, f"refused, yet tensors {sorted(part)} changed"))
                self._restore(part)
                continue
            pgot, part = self._run(i, img0, n)
            keep = np.ones(self.B, bool)
            keep[img0:img0 + n] = False
            if set(part) - outs:
                self.bad.append((*tag, rng, f"tensors {sorted(set(part) - outs)} changed, the whole batch writes {sorted(outs)}"))
            for t, a in part.items():
                for b in np.flatnonzero(keep):
                    if not np.array_equal(a[b], self.state[t][b]):
                        self.bad.append((*tag, rng, "tensor", t, "WROTE image", int(b), *_first_diff(a[b], self.state[t][b])))
            for t in sorted(outs):
                if not np.array_equal(pgot[t][~keep], got[t][~keep]):
                    self.bad.append((*tag, rng, "tensor", t, "differs from the whole-batch run"))
            self._restore(part)

    def check_cover(self, steps_run):
        """every materialised tensor written by exactly one of the steps (all non-postprocess steps of the plan were run)"""
        seen = {}
        for i in steps_run:
            for t in self.written.get(i, ()):
                seen.setdefault(t, []).append(i)
        twice = {t: v for t, v in seen.items() if len(v) > 1}
        return twice, sorted(set(self.held) - set(seen))


def _create(path, B, flags, env, monkeypatch):
    from vbt_amd.interpreter import Interpreter
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return Interpreter(path, max_batch=B, flags=flags)


@pytest.mark.parametrize("name,part", CASES, ids=[f"{n}-{p}" for n, p in CASES])
def test_steps_alone(name, part, model_files, monkeypatch):
    model, B, flags, env, patterns = CONFIGS[name]
    path = model_files[model]
    t0 = time.time()
    g, cases, stages = _graph(path, B)
    it = _create(path, B, flags, env, monkeypatch)
    run = Runner(it, g, cases, stages, wide=flags != 1)
    todo = [i for i in range(len(run.steps) - 1) if run.part(i) == part]
    assert todo, "no step of the plan ends in this part of the graph"
    for p in patterns:
        run.load(p)
        for i in todo:
            run.step(i)
    # the cover of the whole plan, one part per test id: the tensors this part of the graph produces are written by its steps
    twice, never = run.check_cover(todo)
    mine = {g.output(o) for o in range(g.n_ops) if stages[o] == part} & set(run.held)
    never = [t for t in never if t in mine]
    tensors = sorted({t for i in todo for t in run.written[i]})
    print(f"\n[steps alone] {name} / {part}: {len(todo)} of {len(run.steps)} steps, {len(run.held)} materialised tensors, {len(tensors)} written, "
          f"{run.runs} runs ({len(todo) * len(patterns)} step x pattern), {time.time() - t0:.1f} s")
    assert not run.bad, f"{len(run.bad)} findings (step, family, variant, pattern, ...): {run.bad[:40]}"
    assert not twice, f"tensors written by two steps: {twice}"
    assert not never, f"materialised tensors of this part that no step wrote: {never}"


COVER_CHUNKS = 10


@pytest.mark.parametrize("chunk", range(COVER_CHUNKS))
def test_covering_plans_steps_alone(chunk, tmp_path, monkeypatch):
    """Lite0 at flags 0 over the covering plans of the plan-space sweep, written as plan files exactly as that sweep writes them: in each
    plan only the steps whose (group, alternative, step, variant) that plan is the first to cover run, under U and X; references are
    shared between plans by (tensor, the materialised tensors it is computed from, pattern).  The merged side-conv launch stands for no
    tuple of its own: it runs under the first plan and under every plan in which it swallowed a step that is new (with the head layers
    unfused it is the last head convs that merge).  Plan k belongs to test id k mod COVER_CHUNKS."""
    from vbt_amd.interpreter import Interpreter
    B = 3
    g, cases, stages = _graph(LITE0, B)
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    t0 = time.time()
    prefix = str(tmp_path / "plan")
    fn = f"{prefix}.b{B}.f0"
    # the space is that of the heuristic plan's model: autotuning selects from it and never changes it
    space = Interpreter(LITE0, max_batch=B, flags=8).plan_space()
    plans = covering_plans(space)
    monkeypatch.setenv("VBT_PLAN_FILE", prefix)
    covered, cache, bad, n_steps, n_runs, n_plans = set(), {}, [], 0, 0, 0
    for k, plan in enumerate(plans):
        new = plan_tuples(plan) - covered
        covered |= plan_tuples(plan)
        if k % COVER_CHUNKS != chunk:
            continue
        text = plan_text(plan)
        with open(fn, "w") as f:
            f.write(text)
        it = Interpreter(LITE0, max_batch=B, flags=0)
        assert open(fn).read() == text, f"plan {k} was refused (re-tuned and re-written)"
        assert current_plan(it.plan_space()) == plan
        run = Runner(it, g, cases, stages, wide=True, ref_cache=cache)
        key = lambda s: (s["group"], plan[s["group"]][0], s["step"], s["variant"])
        todo = [i for i, s in enumerate(run.steps[:-1]) if s["group"] >= 0 and key(s) in new]
        merged = [i for i, s in enumerate(run.steps[:-1]) if s["group"] < 0]
        lost = new - {key(run.steps[i]) for i in todo} - {t for t in new if t[0] == run.steps[-1]["group"]}
        # ... and a step can only have gone into the merged launch: a one-op pointwise step (or one of the two max pools behind the P6
        # conv, which that launch takes along) whose op the merged launch spans
        where = {(e["group"], e["alt"], e["step"]): e for e in space}
        for t in sorted(lost):
            e = where[t[:3]]
            assert len(merged) == 1 and e["family"] in ("pw_conv_mfma_i8", "maxpool3x3s2") and e["first_op"] == e["last_op"] and \
                run.steps[merged[0]]["first_op"] <= e["first_op"] <= run.steps[merged[0]]["last_op"] and \
                not any(s["group"] == t[0] and s["step"] == t[2] for s in run.steps), \
                f"plan {k}: tuple {t} is covered first here, yet no step of the execution list stands for it"
        if k == 0 or lost:
            todo = sorted(todo + merged)
        for p in "UX":
            if todo:
                run.load(p)
            for i in todo:
                run.step(i)
        twice, never = run.check_cover(todo)
        bad += [(k, *b) for b in run.bad] + [(k, "written twice", twice)] * bool(twice)
        if k == 0:      # every step of this plan ran: every materialised tensor is written by exactly one of them
            assert len(todo) == len(run.steps) - 1
            bad += [(k, "materialised tensors no step wrote", never)] * bool(never)
        n_steps += len(todo)
        n_runs += run.runs
        n_plans += 1
        del run, it
    print(f"\n[steps alone] covering plans, chunk {chunk}: {n_plans} of {len(plans)} plans, {n_steps} steps run, {n_runs} runs, {len(cache)} references, "
          f"{time.time() - t0:.1f} s")
    assert not bad, f"{len(bad)} findings (plan, step, family, variant, pattern, ...): {bad[:40]}"
    assert n_plans == 0 or n_steps > 0


def test_plan_steps_describe_the_execution_list(monkeypatch):
    from vbt_amd import _lib
    it = _create(LITE0, 3, 8, {}, monkeypatch)
    steps = it.plan_steps()
    assert len(steps) == it.num_launches()
    assert max(i for i, s in enumerate(steps) if s["reads_frames"]) + 1 == _lib.lib().vbt_model_entry_steps(it.handle)
    merged = [s for s in steps if s["group"] < 0]
    assert len(merged) == 1 and merged[0]["family"] == "pw_conv_mfma_i8" and merged[0]["n_members"] >= 2 and merged[0]["image0_only"]
    chosen = [e for e in it.plan_space() if e["chosen"]]
    for s in steps:
        if s["group"] >= 0:
            e = next(e for e in chosen if (e["group"], e["step"]) == (s["group"], s["step"]))
            assert (e["family"], e["variant"], e["first_op"], e["last_op"]) == (s["family"], s["variant"], s["first_op"], s["last_op"])
        assert s["image0_only"] == (s["family"] == "fused_sepconv_band" or (s["family"] == "pw_conv_mfma_i8" and s["n_members"] > 0))
    import ctypes
    n, one = ctypes.c_int(), _lib.PlanStepInfo()
    assert _lib.lib().vbt_model_plan_steps(it.handle, ctypes.byref(one), 1, ctypes.byref(n)) == -4 and n.value == len(steps)     # never truncated
    assert _lib.lib().vbt_model_plan_steps(None, None, 0, ctypes.byref(n)) == -1
    flat = _create(LITE0, 1, 1, {}, monkeypatch).plan_steps()
    assert all(s["first_op"] == s["last_op"] == i and s["n_members"] == 0 and s["group"] >= 0 for i, s in enumerate(flat))
