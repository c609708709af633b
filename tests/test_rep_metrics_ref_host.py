"""The rep metrics reference (tests/rep_metrics_ref.py) on the 34 golden clips, on the CPU: its phases are the golden phases, the
corpus exercises the cases the device tests rely on (compaction by the filter, path gaps), and the metrics hold the relations their
definitions imply."""
import numpy as np

import rep_metrics_ref as R


def _all():
    return [(name, cols, gold) + R.corpus_ref(name, cols) for name, cols, gold in R.corpus()]


def test_reference_phases_are_the_golden_phases():
    runs = _all()
    assert len(runs) == 34
    total = 0
    for name, _, gold, ph, m, _ in runs:
        assert np.array_equal(ph, gold), name
        assert m.shape == (len(ph), 8), name
        total += len(ph)
    assert total == 508
    assert sum(r[5].appended - len(r[3]) for r in runs) == 18                 # dropped by the filter after their metrics were stored


def test_corpus_has_path_gaps_in_005_and_007():
    by = {r[0]: r[5] for r in _all()}
    assert by["005"].gaps > 0 and by["007"].gaps > 0
    assert sum(vt.gaps for vt in by.values()) == 35


def test_metric_relations():
    worst = 0.0
    for name, _, _, ph, m, _ in _all():
        for p, r in zip(ph, m):
            assert r[R.PV] >= r[R.MV], name                        # a maximum over steps against the mean
            assert r[R.PV_Y] <= r[R.PV], name
            assert p[0] < r[R.T_PV] <= p[1], name
            assert r[R.N_STEPS] >= 1 and r[R.X_DEV] >= 0, name
            assert r[R.MV] == p[4] / (p[1] - p[0]), name           # the ACV of plot.py:173, by that one division
            worst = max(worst, abs(r[R.ROM_X] + r[R.ROM_Y] - p[4]) / p[4])
    assert worst <= 1.1e-15
