"""Test infrastructure: execution plans that, between them, run every kernel variant a plan file may select.

The library reports its plan space (Interpreter.plan_space(), vbt_model_plan_space in include/vbt_hip_diag.h): one entry per step of
every alternative of every plan group, with the variants the plan loader accepts for that step.  A plan picks one alternative per group
and one accepted variant per step of that alternative; here it is a list, one item per group, of (alternative, ((family, variant), ...)),
which is what a format-2 plan file spells out.

covering_plans builds plans greedily until every (group, alternative, step, variant) tuple of the space is in at least one of them: in
each plan every group takes the alternative with the most tuples still uncovered, and every step of it a variant still uncovered.  An
alternative a group takes while it has uncovered tuples covers one more variant of each of its steps that has any left, so a group is
done after at most sum over its alternatives of the largest step variant count plans (plan_bound).
"""


def space_shape(space):
    """[group][alternative][step] -> (family, variants) of a plan space given as plan_space() entries."""
    shape = []
    for e in space:
        g, a, s = e["group"], e["alt"], e["step"]
        if g == len(shape) and a == 0 and s == 0:
            shape.append([])
        if g == len(shape) - 1 and a == len(shape[g]) and s == 0:
            shape[g].append([])
        assert (g, a, s) == (len(shape) - 1, len(shape[-1]) - 1, len(shape[-1][-1])), f"plan space entries out of order at {(g, a, s)}"
        assert e["variants"], f"group {g} alternative {a} step {s}: no variant"
        shape[g][a].append((e["family"], tuple(e["variants"])))
    return shape


def all_tuples(space):
    return {(e["group"], e["alt"], e["step"], v) for e in space for v in e["variants"]}


def plan_tuples(plan):
    return {(g, alt, s, v) for g, (alt, steps) in enumerate(plan) for s, (_, v) in enumerate(steps)}


def current_plan(space):
    """The plan a model runs: its chosen alternatives and their steps' current variants."""
    plan = []
    for e in space:
        if e["chosen"]:
            if e["step"] == 0:
                assert len(plan) == e["group"], f"group {e['group']}: no chosen alternative, or two"
                plan.append((e["alt"], []))
            plan[-1][1].append((e["family"], e["variant"]))
    return [(alt, tuple(steps)) for alt, steps in plan]


def plan_in_space(plan, space):
    """None if the plan only selects what the space offers, else the first thing it does not."""
    shape = space_shape(space)
    if len(plan) != len(shape):
        return f"{len(plan)} groups in the plan, {len(shape)} in the space"
    for g, (alt, steps) in enumerate(plan):
        if not 0 <= alt < len(shape[g]):
            return f"group {g}: alternative {alt} does not exist"
        if len(steps) != len(shape[g][alt]):
            return f"group {g}: {len(steps)} steps, the alternative has {len(shape[g][alt])}"
        for s, ((fam, v), (want_fam, variants)) in enumerate(zip(steps, shape[g][alt])):
            if fam != want_fam or v not in variants:
                return f"group {g} step {s}: {fam}:{v} is not one of {want_fam}:{list(variants)}"
    return None


def plan_bound(space):
    """Most plans covering_plans may need: max over groups of the sum over alternatives of the largest step variant count."""
    return max((sum(max(len(v) for _, v in steps) for steps in alts) for alts in space_shape(space)), default=0)


def covering_plans(space):
    shape = space_shape(space)
    uncovered = all_tuples(space)
    plans = []
    while uncovered:
        plan = []
        for g, alts in enumerate(shape):
            left = [sum((g, a, s, v) in uncovered for s, (_, vs) in enumerate(steps) for v in vs) for a, steps in enumerate(alts)]
            alt = left.index(max(left))
            steps = []
            for s, (fam, vs) in enumerate(alts[alt]):
                steps.append((fam, next((v for v in vs if (g, alt, s, v) in uncovered), vs[0])))
            plan.append((alt, tuple(steps)))
        uncovered -= plan_tuples(plan)
        plans.append(plan)
    return plans


def plan_text(plan):
    """The plan as the library writes a plan file (format 2)."""
    lines = [f"VBTPLAN2 {len(plan)}"]
    for alt, steps in plan:
        lines.append(f"{alt} {len(steps)}" + "".join(f" {fam}:{v}" for fam, v in steps))
    return "\n".join(lines) + "\n"


def parse_plan_text(text):
    """A format-2 plan file -> plan (the inverse of plan_text)."""
    tok = text.split()
    assert tok[0] == "VBTPLAN2", "not a format-2 plan file"
    plan, i = [], 2
    for _ in range(int(tok[1])):
        alt, n = int(tok[i]), int(tok[i + 1])
        steps = tuple((t.rsplit(":", 1)[0], int(t.rsplit(":", 1)[1])) for t in tok[i + 2:i + 2 + n])
        plan.append((alt, steps))
        i += 2 + n
    assert i == len(tok), "trailing tokens"
    return plan
