"""Conditions on the crowd scenes of tests/crowd_cases.py, checked on the numpy oracles alone (no device): the scenes reach what the
device tests of tests/test_gpu_tracker_crowd.py are there for - the general assignment solver at 25 x 64, rectangular both ways and
with exact ties, a full track list with deaths and slot reuse, mass recovery in the second association - so that those tests cannot
pass by not reaching the code.  Every count is printed before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest

import crowd_cases as cc

THR = 0.1


def _first(rep):
    return [c for c in rep.calls if c.site == "first"]


def _second(rep):
    return [c for c in rep.calls if c.site == "second"]


def _replay(tracker, name):
    return cc.replay_sort(name) if tracker == "sort" else cc.replay_ocsort(name, tracker)


TRACKERS = ("diou", "iou", "sort")


def test_builders_are_deterministic_and_within_the_limits():
    for name, (build, _) in cc.SCENES.items():
        (fa, ta), (fb, tb) = build(), build()
        assert len(fa) == len(fb) <= 80 and np.array_equal(ta, tb), name
        assert all(a.shape == b.shape and a.shape[1] == 6 and len(a) <= cc.MAXD and np.array_equal(a, b) for a, b in zip(fa, fb)), name
        assert all((a[:, 2] > a[:, 0]).all() and (a[:, 3] > a[:, 1]).all() and (a[:, 4] > 0.2).all() for a in fa), name
    assert max(len(f) for f in cc.scene("A")[0]) == max(len(f) for f in cc.scene("B")[0]) == cc.MAXD


@pytest.mark.parametrize("tracker", TRACKERS)
def test_scene_a_full_house(tracker):
    rep = _replay(tracker, "A")
    live, per_step = cc.live_counts(rep), cc.rows_per_step(rep)
    full_calls = sum(c.cost.shape == (cc.MAXD, cc.MAXT) for c in _first(rep))
    full = [s for s in rep.steps if len(s.ids) == cc.MAXT]
    last_emits = sum(s.ids[63] in cc.emitted_ids(s) for s in full)
    last_silent = sum(s.ids[63] not in cc.emitted_ids(s) and len(s.out) > 0 for s in full)
    print(f"A/{tracker}: max live {max(live)}, frames at 64: {live.count(64)}, solver calls 25x64: {full_calls}, most rows in a frame "
          f"{max(per_step)}, rows {len(rep.rows['id'])}, position 63 emits in {last_emits} frames, is silent while others emit in {last_silent}")
    assert max(live) == cc.MAXT and live.count(cc.MAXT) >= 30
    assert full_calls >= 20
    assert max(per_step) == cc.MAXD
    assert last_emits >= 1 and last_silent >= 1
    assert len(rep.rows["id"]) >= 300
    assert rep.steps[-1].ids == list(range(64))                     # list position = object number: no track was ever replaced


@pytest.mark.parametrize("asso", ["diou", "iou"])
def test_scene_b_deaths_and_slot_reuse_at_64(asso):
    rep = cc.replay_ocsort("B", asso)
    live = cc.live_counts(rep)
    mass = [(i, n, pos) for i, n, pos in cc.deaths(rep) if n == cc.MAXT and len(pos) >= 2]
    print(f"B/{asso}: deaths (step, live, positions) {cc.deaths(rep)}, live after each step {live}")
    assert max(live) == cc.MAXT and len(mass) >= 1
    step, _, pos = mass[0]
    assert 0 in pos and 63 in pos and any(0 < p < 63 for p in pos) and len(pos) >= 8
    assert min(live[step:]) < cc.MAXT and live[-1] == cc.MAXT and cc.MAXT in live[step + 1:]       # later births: back to 64
    born_late = set(rep.steps[-1].ids) - set(rep.steps[step].before)
    assert len(born_late) >= 8
    # the export rule at the time of the deaths and at the end: a dead id holds it, so the device has to carry it in best_id / best_cum
    dead = {rep.steps[step].before[p] + 1 for p in pos}
    at_death = {k: v[rep.rows["time"] <= cc.scene("B")[1][step]] for k, v in rep.rows.items()}
    best_then, _ = cc.export_rule(at_death)
    best_end, cum = cc.export_rule(rep.rows)
    print(f"B/{asso}: dead ids {sorted(dead)}, export id at the deaths {best_then}, at the end {best_end}, path {cum[best_end]:.4f}, "
          f"runner-up {sorted(cum.values())[-2]:.4f}")
    assert best_then in dead and best_end in dead


@pytest.mark.parametrize("tracker", TRACKERS)
def test_scene_c_more_detections_than_tracks(tracker):
    rep = _replay(tracker, "C")
    shapes = [c.cost.shape for c in _first(rep)]
    more, fewer = sum(d > t >= 5 for d, t in shapes), sum(5 <= d < t for d, t in shapes)
    print(f"C/{tracker}: first-association solver calls {len(shapes)}, n_det > n_trk >= 5: {more}, 5 <= n_det < n_trk: {fewer}, "
          f"largest {max(shapes)}")
    assert more >= 10 and fewer >= 10


@pytest.mark.parametrize("asso", ["diou", "iou"])
def test_scene_d_recovery_en_masse(asso):
    rep = cc.replay_ocsort("D", asso)
    big = [(c.frame, c.cost.shape, int(sum(-c.cost[r, k] >= THR for r, k in c.pairs))) for c in _second(rep) if min(c.cost.shape) >= 5]
    print(f"D/{asso}: second association (frame, (unmatched detections, unmatched tracks), recovered) {big}")
    assert any(d <= t for _, (d, t), _ in big) and any(d > t for _, (d, t), _ in big)
    assert max(r for _, _, r in big) >= 5


@pytest.mark.parametrize("tracker", TRACKERS)
def test_scene_e_exact_ties(tracker):
    rep = _replay(tracker, "E")
    twins = [c for c in rep.calls if min(c.cost.shape) >= 5 and cc.has_twin_lines(c.cost)]
    n_second = sum(c.site == "second" for c in twins)
    same_det = sum(len(np.unique(f, axis=0)) < len(f) for f in cc.scene("E")[0])
    print(f"E/{tracker}: cost matrices with two identical rows or columns {len(twins)} ({n_second} of the second association), frames "
          f"with a repeated detection {same_det}")
    assert len(twins) >= 5 and same_det >= 5
    if tracker == "diou":
        assert n_second >= 1                                         # never-observed tracks: identical columns on the last observations


def test_recording_leaves_the_oracle_as_it_was():
    from oracle import ocsort_np as oc
    solve, assoc = oc.linear_assignment, oc.associate
    cc.replay_ocsort_on(*cc.scene("D"))
    assert oc.linear_assignment is solve and oc.associate is assoc
    plain = oc.track_boxes(*cc.scene("D"), max_age=30, asso_func="diou", iou_threshold=0.1)
    rec = cc.replay_ocsort("D")
    assert all(np.array_equal(np.asarray(plain[k]), rec.rows[k]) for k in ["id"] + cc.COLS)
