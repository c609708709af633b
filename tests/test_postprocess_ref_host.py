"""The crafted decode + NMS scenarios on the CPU (tests/postprocess_cases.py): every scenario meets its coverage condition - computed
from the numpy reference alone - and the numpy reference (tests/postprocess_ref.py) equals the C oracle's post-process
(oracle/detector.c: vbto_postprocess on the same head bytes) bit for bit on all four outputs, for all six models.  This is what makes
the scenarios trustworthy before tests/test_gpu_postprocess.py shows them to the kernel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postprocess_cases as pc  # noqa: E402


@pytest.fixture(scope="module")
def files(tmp_path_factory, model_path):
    return pc.model_files(tmp_path_factory.mktemp("post"), model_path)


@pytest.mark.parametrize("name", pc.MODELS)
def test_scenarios_meet_their_coverage_conditions(files, name):
    path, kind = files[name]
    m, cases = pc.build(path, kind)
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) and all(any(n.startswith(s) for n in names) for s in pc.KINDS[kind]["names"])
    for c in cases:
        print(pc.describe(c))
        c.check()
        n = c.ref.count
        assert not c.ref.boxes[n:].any() and not c.ref.scores[n:].any() and not c.ref.classes[n:].any()
        assert (np.diff(c.ref.cand_score) <= 0).all()
    # the boundary frames: every boundary anchor is examined in some frame slot
    seen = set()
    for c in cases:
        if c.name.startswith("boundaries"):
            seen |= set(c.ref.order[:c.ref.visited].tolist())
    assert seen == set(pc.Gen(m, kind).boundary_anchors().tolist())
    if kind != "tiny":
        kinds = {k for c in cases for k, _ in c.rounds}
        assert {"bitonic", "slice:bitonic", "slice:empty", "count1", "count2", "count3", "count4"} <= kinds, kinds


def test_level_tensors_round_trip(files):
    for name in ("lite0", "tiny_c3"):
        m, cases = pc.build(*files[name])
        c = cases[-1]
        t = m.to_levels(c.cls, c.box)
        assert [x.shape for x in t] == m.shapes
        cls, box = m.from_levels(t)
        assert np.array_equal(cls, c.cls) and np.array_equal(box, c.box)
        a = int(m.base[1]) + 5                       # anchor 5 of level 1: location 0, anchor-in-location 5
        assert t[1][0, 0, 5 * m.C:(5 + 1) * m.C].tolist() == c.cls[a].tolist() and t[m.nl + 1][0, 0, 20:24].tolist() == c.box[a].tolist()


@pytest.mark.parametrize("name", pc.MODELS)
def test_reference_equals_oracle_postprocess(files, oracle_lib, name):
    path, kind = files[name]
    m, cases = pc.build(path, kind)
    det = oracle_lib.OracleDetector(path)
    for c in cases:
        for tid, t in zip(m.inputs, m.to_levels(c.cls, c.box)):
            det.set_tensor(tid, t)
        boxes, scores, classes, count = det.postprocess()
        r = c.ref
        assert count == r.count, (c.name, count, r.count)
        assert np.array_equal(boxes, r.boxes) and np.array_equal(scores, r.scores) and np.array_equal(classes, r.classes), c.name
