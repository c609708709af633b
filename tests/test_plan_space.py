"""The plan space, host side (no GPU): vbt_plan_step_space as the C compiler lays it out is the ctypes structure the wrapper reads, and
the covering plans of tests/plan_cover.py (what tests/test_gpu_plan_space.py runs) cover every (group, alternative, step, variant) of a
space, select nothing outside it, stay within their bound, and are written the way the library writes a plan file."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from plan_cover import (all_tuples, covering_plans, current_plan, parse_plan_text, plan_bound, plan_in_space, plan_text, plan_tuples,
                        space_shape)


def test_plan_step_space_layout_matches_ctypes(tmp_path):
    from vbt_amd._lib import PlanStepSpace
    src = tmp_path / "layout.c"
    fields = [f for f, _ in PlanStepSpace._fields_]
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"vbt_hip_diag.h\"\nint main(void) {\n"
                   "  vbt_plan_step_space s;\n"
                   "  printf(\"size %zu\\n\", sizeof(vbt_plan_step_space));\n"
                   "  printf(\"n_family %zu\\n\", sizeof(s.family));\n  printf(\"n_variants_cap %zu\\n\", sizeof(s.variants) / sizeof(s.variants[0]));\n" +
                   "".join(f"  printf(\"{f} %zu\\n\", offsetof(vbt_plan_step_space, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(PlanStepSpace)
    assert int(out["n_family"]) == 32 and int(out["n_variants_cap"]) == len(PlanStepSpace().variants) == 48
    for f in fields:
        assert int(out[f]) == getattr(PlanStepSpace, f).offset, f


FAMILIES = ("fused_mbconv", "fused_expand_dw", "pw_conv_mfma_i8", "dw_conv_f32acc", "fused_sepconv_band", "decode_nms")
POOL = [-1] + list(range(32)) + list(range(100, 108)) + list(range(200, 208))


def synthetic_space(seed, groups=40):
    """A space shaped like the library's: groups of 1-5 alternatives of 1-3 steps, 1-48 variants per step (one group with a single
    step of a single variant, one alternative with a step of 48), the first alternative chosen where the seed says so."""
    rng = np.random.default_rng(seed)
    space = []
    for g in range(groups):
        n_alts = 1 if g == 0 else int(rng.integers(1, 6))
        chosen = int(rng.integers(0, n_alts))
        for a in range(n_alts):
            for s in range(1 if g == 0 else int(rng.integers(1, 4))):
                n = 1 if g == 0 else 48 if (g, a, s) == (1, 0, 0) else int(rng.integers(1, 34))
                variants = [int(v) for v in rng.choice(POOL, size=n, replace=False)]
                space.append({"group": g, "alt": a, "step": s, "chosen": a == chosen, "variant": variants[int(rng.integers(0, n))],
                              "first_op": 0, "last_op": 0, "family": FAMILIES[int(rng.integers(0, len(FAMILIES)))], "variants": variants})
    return space


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 7, 42])
def test_covering_plans_cover_the_space_inside_the_bound(seed):
    space = synthetic_space(seed)
    plans = covering_plans(space)
    covered = set()
    for p in plans:
        assert plan_in_space(p, space) is None, plan_in_space(p, space)
        covered |= plan_tuples(p)
    assert covered == all_tuples(space)
    assert len(plans) <= plan_bound(space)
    assert len(plans) >= max(len(e["variants"]) for e in space)      # (a plan runs one variant of each step)


def test_covering_plans_of_a_one_variant_space_is_one_plan():
    space = [{"group": g, "alt": 0, "step": 0, "chosen": True, "variant": -1, "first_op": g, "last_op": g, "family": "decode_nms",
              "variants": [-1]} for g in range(3)]
    plans = covering_plans(space)
    assert plans == [current_plan(space)] and plan_bound(space) == 1 and covering_plans([]) == []


def test_plan_in_space_refuses_what_the_space_does_not_offer():
    space = synthetic_space(5, groups=6)
    plan = covering_plans(space)[0]
    shape = space_shape(space)
    g = next(i for i, alts in enumerate(shape) if len(alts) > 1)
    bad_alt = list(plan)
    bad_alt[g] = (len(shape[g]), plan[g][1])
    assert "does not exist" in plan_in_space(bad_alt, space)
    alt, steps = plan[g]
    fam, v = steps[0]
    bad_v = list(plan)
    bad_v[g] = (alt, ((fam, 99999),) + steps[1:])
    assert "not one of" in plan_in_space(bad_v, space)
    bad_f = list(plan)
    bad_f[g] = (alt, ((fam + "_x", v),) + steps[1:])
    assert "not one of" in plan_in_space(bad_f, space)
    assert "steps" in plan_in_space([(alt, steps + steps)] if len(shape) == 1 else plan[:g] + [(alt, steps + steps)] + plan[g + 1:], space)
    assert "groups" in plan_in_space(plan[:-1], space)


def test_current_plan_is_the_chosen_alternatives():
    space = synthetic_space(9, groups=12)
    plan = current_plan(space)
    assert len(plan) == 12 and plan_in_space(plan, space) is None
    for e in space:
        if e["chosen"]:
            assert plan[e["group"]][0] == e["alt"] and plan[e["group"]][1][e["step"]] == (e["family"], e["variant"])


@pytest.mark.parametrize("name", ["plan_lite0.b1.f0", "plan_lite0.b8.f0", "plan_lite0.b64.f0", "plan_lite0.b256.f0", "plan_lite2.b64.f0"])
def test_pinned_plan_text_round_trips(name):
    """The writer spells a plan the way the library's save_plan does: each pinned file comes back byte for byte (b1 and b8 were
    committed without the final newline save_plan writes)."""
    raw = open(os.path.join(ROOT, "profiles", name), "rb").read()
    plan = parse_plan_text(raw.decode())
    assert plan_text(plan).encode() == (raw if name not in ("plan_lite0.b1.f0", "plan_lite0.b8.f0") else raw + b"\n")
    if name == "plan_lite0.b64.f0":
        assert len(plan) == 53 and plan[1] == (2, (("fused_mbconv", 25),)) and plan[12][1] == (("fused_expand_dw", 206), ("pw_conv_mfma_i8", 5))
