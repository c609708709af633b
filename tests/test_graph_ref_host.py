"""tests/graph_ref.py (the numpy evaluator of the container's op types) against oracle/detector.c on every tensor of four models, hand
vectors for its requantisation, and the conditions the crafted patterns of tests/step_cases.py are meant to meet - asserted here on the
reference alone, on the CPU, so that tests/test_gpu_steps_alone.py can rely on them.

What "reach" means below.  For a conv op and its input's X pattern the accumulator of output channel n can be at most
hi_n = b_n + sum max(w (127 - z_x), w (-128 - z_x)) and at least the matching lo_n (step_cases.conv_extremes).  The pattern hosts
min(2N, usable positions) of these 2N extremes and the reference accumulator must attain exactly that many - for every conv that is the
FIRST consumer of its input (the pattern of a tensor serves one consumer; the others are listed in the table with what they reach).  The
library's proof that a conv's accumulators stay inside (-2^22, 2^22) is 255 * sum |w| + |b| < 2^22 - 1 on every channel
(step_cases.kb_bound); a conv's reach is max over channels of |accumulator| / that channel's own bound.  x - z_x spans 255, not +-255, so
a channel whose weights have mixed signs stops near one half; a channel whose weights share one sign comes close to 1.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_ref as gr  # noqa: E402
import step_cases as sc  # noqa: E402

LITE0 = os.path.join(ROOT, "models", "efficientdet_lite0_synth.vbtm")
LITE2 = os.path.join(ROOT, "models", "efficientdet_lite2_synth.vbtm")


def _frames(S):
    from vbt_amd import synth
    rng = np.random.Generator(np.random.PCG64(5))
    return np.stack([synth.render(synth.background(3, S), 4), rng.integers(0, 256, (S, S, 3), dtype=np.uint8),
                     np.zeros((S, S, 3), np.uint8), np.full((S, S, 3), 255, np.uint8)])


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("graph_ref")
    tie = str(d / "tie.vbtm")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_model.py"), "--arch", "0", "--out", tie, "--calib", "4", "--tie_adds"],
                          stdout=subprocess.DEVNULL)
    return {"lite0": LITE0, "lite2": LITE2, "clamped": sc.write_clamped(LITE0, str(d / "clamped.vbtm")), "tie_adds": tie,
            "kb_edge": sc.write_kb_edge(LITE0, str(d / "kb_edge.vbtm"))[0]}


@pytest.mark.parametrize("name", ["lite0", "lite2", "clamped", "tie_adds", "kb_edge"])
def test_evaluator_equals_the_oracle_on_every_tensor(name, models, oracle_lib):
    path = models[name]
    g = gr.GraphRef(path)
    det = oracle_lib.OracleDetector(path)
    frames = _frames(det.size)
    if name == "lite2":
        frames = frames[:1]
    val = g.run_graph(frames)
    assert sorted(val) == list(range(1, det.num_tensors - 1))
    bad = []
    for b, f in enumerate(frames):
        det.run(f)
        for t, v in val.items():
            want = det.tensor(t)
            if not np.array_equal(v[b], want):
                d = np.argwhere(v[b] != want)
                bad.append((b, t, g.type(g.producer[t]), tuple(d[0]), len(d), int(np.abs(v[b].astype(int) - want.astype(int)).max())))
    assert not bad, f"{len(bad)} tensors differ (frame, tensor, op type, first (y, x, c), count, max|diff|): {bad[:20]}"


def test_requantisation_hand_vectors():
    q = gr.requantize
    # exact .5 ties under a power-of-two multiplier: to the even neighbour, in both directions and for both signs
    assert q(np.array([1, 3, 5, -1, -3, -5]), np.float32(0.5), 0, -128, 127).tolist() == [0, 2, 2, 0, -2, -2]
    assert q(np.array([2, 6, 10, -6]), np.float32(0.25), 3, -128, 127).tolist() == [3, 5, 5, 1]          # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -1.5 -> -2
    # |acc| > 2^24: the conversion to float32 itself rounds to even.  2^24 + 1 -> 2^24, 2^24 + 3 -> 2^24 + 4; times 2^-20: 16, 16.000004 -> 16
    assert np.array([2 ** 24 + 1, 2 ** 24 + 3], np.int64).astype(np.float32).tolist() == [2.0 ** 24, 2.0 ** 24 + 4]
    # ... seen through the clamp.  5 * 2^22 + 1 ties between 5 * 2^22 (even mantissa) and + 2: to even gives 2.5 under 2^-23 -> 2; a
    # conversion rounding the tie upwards gives 2.5000002 -> 3.  3 * 2^23 - 1 ties between 3 * 2^23 - 2 (odd mantissa) and 3 * 2^23: to
    # even gives 1.5 under 2^-24 -> 2; a truncating conversion gives 1.4999999 -> 1.
    assert q(np.array([5 * 2 ** 22 + 1, -5 * 2 ** 22 - 1]), np.float32(2.0 ** -23), 0, -128, 127).tolist() == [2, -2]
    assert q(np.array([3 * 2 ** 23 - 1, -3 * 2 ** 23 + 1]), np.float32(2.0 ** -24), 0, -128, 127).tolist() == [2, -2]
    # the product is taken in float32 on the converted accumulator, not in double on the integer: (2^24 + 1) * 5 * 2^-25 is 2.5000001 in
    # double (-> 3) and float32(2^24) * 5 * 2^-25 = 2.5 (-> 2)
    assert q(np.array([2 ** 24 + 1]), np.float32(5.0 * 2.0 ** -25), -128, -128, 127).tolist() == [2 - 128]
    # beyond each rail (after the zero point), and an explicit clamp narrower than int8
    assert q(np.array([1000, -1000, 120, -120]), np.float32(1.0), 10, -128, 127).tolist() == [127, -128, 127, -110]
    assert q(np.array([1000, -1000, 50, -50, 96, -101]), np.float32(1.0), 0, -99, 93).tolist() == [93, -99, 50, -50, 93, -99]
    # per-channel multipliers broadcast over the last axis
    assert q(np.array([[4, 4], [-4, -4]]), np.array([0.5, 0.125], np.float32), 1, -128, 127).tolist() == [[3, 1], [-1, 1]]


def test_add_equals_the_scalar_integer_statement():
    from test_quant_kat import ref_add, ref_add_params
    a, b = [x.reshape(-1).astype(np.int8) for x in np.meshgrid(np.arange(-128, 128), np.arange(-128, 128), indexing="ij")]
    for pargs, zo, lo, hi in (((0.0431, 0.0517, 0.0622, -7, 12), 5, -128, 127), ((0.25, 0.5, 0.5, 1, -1), -128, -128, 40),
                              ((2.0, 0.004, 0.008, 100, -100), 0, -128, 127)):
        prm = ref_add_params(*pargs)
        got = gr.add_q(a, b, prm, zo, lo, hi)
        assert got[::41].tolist() == [ref_add(int(x), int(y), prm, zo, lo, hi) for x, y in zip(a[::41], b[::41])]


# ---------------------------------------------------------------------------------------------------------------------------------
# conditions on the patterns
# ---------------------------------------------------------------------------------------------------------------------------------
def reach_table(g, cases):
    """per conv op: (op, type, N, first consumer?, extremes hosted, extremes attained, kb-provable, reach against the channel's own bound,
    reach against 2^22 - 1)"""
    rows = []
    for oi in sc.conv_ops(g):
        src = g.inputs(oi)[0]
        acc = g.accumulator(oi, cases.tensor(src, "X"))
        N = acc.shape[-1]
        flat = acc.reshape(-1, N)
        hi, lo = sc.conv_extremes(g, oi)
        assert np.all(flat.max(axis=0) <= hi) and np.all(flat.min(axis=0) >= lo), f"op {oi}: the closed form is not an extreme"
        got = int((flat.max(axis=0) == hi).sum() + (flat.min(axis=0) == lo).sum())
        bound = sc.kb_bound(g, oi)
        rows.append((oi, g.type(oi), N, cases.first_consumer(src) == oi, min(2 * N, cases.usable(oi)), got, bool(np.all(bound < 2 ** 22 - 1)),
                     float((np.abs(flat).max(axis=0) / bound).max()), float(np.abs(flat).max() / (2 ** 22 - 1))))
    return rows


def format_reach(rows):
    out = ["op type   N first hosted attained kb reach(own) reach(2^22-1)"]
    for oi, ty, N, first, want, got, kb, r_own, r_abs in rows:
        out.append(f"{oi:3d} {('stem', 'pw', 'dw')[ty - 1]:4s} {N:4d} {int(first)} {want:6d} {got:8d} {int(kb)} {r_own:9.3f} {r_abs:9.3f}")
    return "\n".join(out)


@pytest.mark.parametrize("which,B", [("lite0", 3), ("lite2", 2)])
def test_accumulator_reach_under_x(which, B):
    g = gr.GraphRef({"lite0": LITE0, "lite2": LITE2}[which])
    rows = reach_table(g, sc.Cases(g, B))
    print(f"\n[reach] {which}, batch {B}\n" + format_reach(rows))
    own = [r for r in rows if r[3]]
    assert len(own) >= 0.9 * len(rows)
    short = [(r[0], r[4], r[5]) for r in own if r[5] != r[4]]
    assert not short, f"convs whose X pattern hosts more extremes than the accumulator attains (op, hosted, attained): {short}"
    assert all(r[4] > 0 for r in own)
    kb = [r for r in rows if r[6]]
    print(f"[reach] {which}: {len(kb)} of {len(rows)} convs are kb-provable; best reach {max(r[7] for r in kb):.3f}; "
          f"{sum(r[7] >= 0.9 for r in kb)} at 0.9 or above")
    assert len(kb) >= 0.8 * len(rows)
    if which == "lite0":
        assert sum(r[1] == gr.OP_PW for r in rows) == 101 and sum(r[1] == gr.OP_PW for r in kb) == 91
        # what the shipped weights allow, whatever the input: the edge of the proven range is test_kb_edge_container's business
        assert max(r[8] for r in kb) < 0.5


def test_kb_edge_container_runs_at_the_edge_of_the_proven_range(tmp_path):
    """step_cases.write_kb_edge: every rewritten conv still passes the library's proof (255 * sum |w| + |b| < 2^22 - 1 on every channel,
    restated in step_cases.kb_bound), and its reference accumulator reaches 0.9 * (2^22 - 1) and beyond at BOTH signs - under X with
    the conv's input crafted directly (the one-kernel-per-op plan), and for the depthwise convs also under S with only the block input
    crafted, i.e. inside a fused MBConv kernel, where the expanded tensor never leaves LDS."""
    path, edge = sc.write_kb_edge(LITE0, str(tmp_path / "kb_edge.vbtm"))
    g = gr.GraphRef(path)
    cases = sc.Cases(g, 3)
    want = 0.9 * sc.KB_LIMIT
    assert len(edge["dw"]) == 15 and len(edge["pw"]) == 5
    assert {int(g.ops[d]["k"]) for d in edge["dw"]} == {3, 5} and {int(g.ops[d]["stride"]) for d in edge["dw"]} == {1, 2}
    rows = []
    for oi in edge["dw"] + edge["pw"]:
        assert np.all(sc.kb_bound(g, oi) < sc.KB_LIMIT), oi
        assert sc.kb_bound(g, oi).max() == sc.KB_LIMIT - 1
        src = g.inputs(oi)[0]
        assert cases.first_consumer(src) == oi
        acc = g.accumulator(oi, cases.tensor(src, "X"))
        assert np.abs(acc).max() < sc.KB_LIMIT
        rows.append((oi, "X", int(acc.max()), int(acc.min())))
    for e, d, p in edge["blocks"]:
        if d in edge["dw"]:
            acc = g.accumulator(d, g.eval_op(e, [cases.tensor(g.inputs(e)[0], "S")]))
            rows.append((d, "S, through the expand conv", int(acc.max()), int(acc.min())))
    print("\n[kb edge] op, pattern, max / min accumulator as a fraction of 2^22 - 1")
    for oi, how, hi, lo in rows:
        print(f"  {oi:3d} {how}: {hi / sc.KB_LIMIT:.6f} {lo / sc.KB_LIMIT:.6f}")
    assert all(hi >= want and lo <= -want for _, _, hi, lo in rows), rows


def three_input_sums(g):
    """(partial ADD, final ADD) of every 3-input sum: an ADD one of whose inputs is an ADD's output read by nobody else"""
    out = []
    for oi in range(g.n_ops):
        if g.type(oi) != gr.OP_ADD:
            continue
        for t in g.inputs(oi):
            p = g.producer.get(t)
            if p is not None and g.type(p) == gr.OP_ADD and g.readers[t] == [oi]:
                out.append((p, oi))
    return out


def can_saturate(g, p):
    """the rails the partial sum `p` reaches for SOME input pair, on its unclamped value: the ADD is monotonic in both inputs (positive
    multipliers), so the corners decide"""
    r = g.ops[p]
    bias, am, bm, shift = (int(v) for v in r["add_q"])
    assert am > 0 and bm > 0
    zo = g.zero_point(g.output(p))
    top, bottom = ((bias + 127 * am + 127 * bm) >> shift) + zo, ((bias - 128 * am - 128 * bm) >> shift) + zo
    return top > int(r["act_max"]), bottom < int(r["act_min"])


@pytest.mark.parametrize("which,B", [("lite0", 3), ("lite2", 2)])
def test_partial_sums_saturate_under_x_and_s(which, B):
    """Each source of the sum patterned directly (what the one-kernel-per-op plan runs; the fused nodes read the same bytes through
    their resamples): the UNCLAMPED partial sum lies beyond a rail on at least 1 % of the elements, at each rail the parameters allow."""
    g = gr.GraphRef({"lite0": LITE0, "lite2": LITE2}[which])
    cases = sc.Cases(g, B)
    sums = three_input_sums(g)
    assert len(sums) >= 9
    never, bad = [], []
    for p, _ in sums:
        r = g.ops[p]
        can = can_saturate(g, p)
        if not any(can):
            never.append(p)
            continue
        bias, am, bm, shift = (int(v) for v in r["add_q"])
        zo = g.zero_point(g.output(p))
        for pattern in ("X", "S"):
            a, b = (cases.tensor(t, pattern) for t in g.inputs(p))
            raw = ((bias + a.astype(np.int64) * am + b.astype(np.int64) * bm) >> shift) + zo
            frac = (float((raw > int(r["act_max"])).mean()), float((raw < int(r["act_min"])).mean()))
            for side in (0, 1):
                if can[side] and frac[side] < 0.01:
                    bad.append((p, pattern, ("top", "bottom")[side], frac[side]))
    print(f"\n[partial sums] {which}: {len(sums)} 3-input sums; no input pair saturates the partial sum of ops {never}")
    assert not bad, bad
    assert len(never) < len(sums)


@pytest.mark.parametrize("which,B", [("lite0", 3), ("lite2", 2)])
def test_add_pair_coverage_under_x(which, B):
    """Every ADD whose tensor holds 65 536 elements or more per batch and whose two inputs both serve it sees every (a, b) pair; the
    large ADDs one of whose inputs serves an earlier consumer are counted and listed, and see at least 512 pairs.  EVERY ADD of the
    graph, large or small, sees both inputs on the same rail, (127, 127) and (-128, -128): the two pairs that bring
    bias + a * a_mult + b * b_mult closest to the ends of int32."""
    g = gr.GraphRef({"lite0": LITE0, "lite2": LITE2}[which])
    cases = sc.Cases(g, B)
    full, other = [], []
    corners = {(v + 128) * 256 + v + 128 for v in (-128, 127)}
    for oi in range(g.n_ops):
        if g.type(oi) != gr.OP_ADD:
            continue
        ta, tb = g.inputs(oi)
        a, b = cases.tensor(ta, "X"), cases.tensor(tb, "X")
        pairs = np.unique((a.astype(np.int32).reshape(-1) + 128) * 256 + b.astype(np.int32).reshape(-1) + 128)
        assert corners <= set(pairs.tolist()), (oi, "a corner pair is missing")
        if B * int(np.prod(g.shape(g.output(oi)))) < sc.GRID:
            continue
        n = len(pairs)
        if cases.first_consumer(ta) == oi and cases.first_consumer(tb) == oi:
            full.append((oi, n))
        else:
            other.append((oi, n))
    print(f"\n[pairs] {which}: ADDs with both inputs their own (op, pairs) {full}; large ADDs sharing an input with an earlier consumer {other}")
    assert full and all(n == sc.GRID for _, n in full), full
    assert all(n >= 512 for _, n in other), other


@pytest.mark.parametrize("which,B", [("lite0", 3), ("lite2", 2)])
def test_rails_and_distinct_images(which, B):
    g = gr.GraphRef({"lite0": LITE0, "lite2": LITE2}[which])
    cases = sc.Cases(g, B)
    for tid in range(len(g.tensors) - 1):
        u = cases.tensor(tid, "U")
        lo, hi = (0, 255) if tid == g.input_tensor else (-128, 127)
        assert all((u[b] == lo).any() and (u[b] == hi).any() for b in range(B)), tid
        for p in sc.PATTERNS:
            a = cases.tensor(tid, p)
            assert all(not np.array_equal(a[i], a[j]) for i in range(B) for j in range(i)), (tid, p)
            assert np.array_equal(a, sc.Cases(g, B).tensor(tid, p))        # deterministic


def test_reference_recurses_through_unmaterialised_tensors():
    """reference(tid, state) with a tensor missing from the state equals the evaluation with it present"""
    g = gr.GraphRef(LITE0)
    cases = sc.Cases(g, 2)
    add = next(f for _, f in three_input_sums(g))
    partial = next(t for t in g.inputs(add) if g.type(g.producer[t]) == gr.OP_ADD)
    srcs = set(g.inputs(add)) | set(g.inputs(g.producer[partial]))
    state = {t: cases.tensor(t, "U") for t in srcs if t != partial}
    full = dict(state)
    full[partial] = g.eval_op(g.producer[partial], [state[t] for t in g.inputs(g.producer[partial])])
    assert np.array_equal(g.reference(g.output(add), state), g.reference(g.output(add), full))
    full[partial] = cases.tensor(partial, "S")
    assert not np.array_equal(g.reference(g.output(add), state), g.reference(g.output(add), full))
