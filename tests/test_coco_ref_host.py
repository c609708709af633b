"""COCO metrics without a GPU (include/vbt_hip.h, "COCO metrics").  pycocotools is not installed where this suite runs, so the numpy
restatement (tests/coco_ref.py) every GPU test compares against is pinned here instead: by a case worked out by hand, by the two
threshold tables against np.linspace, and by the recall denominators of the reference's own training logs
(tests/golden/coco_log_metrics.json), which show that the reference's evaluator saw the same 105 boxes in the same area classes.  The
shared core (vbt_amd/csrc/coco_core.h) runs as a stand-alone host program under -fsanitize=address,undefined
(tests/fuzz/coco_check.cc, run as a program, never loaded into Python) against the restatement on every case of the GPU test; and the
entry points of the C ABI are exported, declared and bound."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import coco_cases as K
import coco_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vbt_coco_create", "vbt_coco_destroy", "vbt_coco_reset", "vbt_coco_add_detections", "vbt_coco_table", "vbt_coco_accumulate")


def test_entry_points_are_exported_declared_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib, evaluate
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "vbt_hip.h")).read()
    assert "COCO metrics" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in _lib.declared_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, code), name
    import ctypes
    assert ctypes.sizeof(_lib.CocoSummary) == 12 * 8 + 6 * 4
    assert callable(evaluate.CocoEvaluator.accumulate) and callable(evaluate.coco_metrics)
    assert evaluate.COCO_KEYS == C.STAT_NAMES + ("AP_/barbell",)


def test_hand_worked_case():
    """Image 128 x 128, boxes A = (16,16,64,64) (48 x 48 = 2304, medium) and B = (80,80,110,110) (30 x 30 = 900, small); detections
    (16,16,64,64) at 0.9 = A exactly, (70,5,95,25) at 0.8 touching nothing (20 x 25 = 500, small) and (87,80,117,110) at 0.7 with
    intersection 23 x 30 = 690 and union 900 + 900 - 690 = 1110 with B: IoU 0.6216, a match at thresholds 0.5, 0.55 and 0.6.
    all, t <= 0.6: tp fp tp, recall 0.5 0.5 1, precision 1 1/2 2/3, envelope 1 2/3 2/3: 51 thresholds at 1 and 50 at 2/3; t > 0.6: 51 at 1,
    50 at 0.  AP50 = (51 + 50 2/3) / 101, AP75 = 51 / 101, AP = (3 (51 + 100/3) + 7 * 51) / 1010 = 61 / 101.
    small (npig 1): A is ignored, the first detection matches it and is ignored; the second is a false positive, the third the true
    positive at t <= 0.6: precision 1/2 at every threshold -> APs = 3 * 0.5 / 10 = 0.15, ARs = 0.3.  medium (npig 1): the small
    detections that stay unmatched are ignored, the first is the true positive: APm = ARm = 1.  large: no box, -1.
    ARmax1 = 0.5 (only the first detection), ARmax10 = ARmax100 = (3 * 1 + 7 * 0.5) / 10 = 0.65."""
    tab, precision, recall, scores, stats = C.evaluate([C.hand_case()])
    assert C.bb_iou(C.det_xywh(C.hand_case()[0][2:3], 128, 128)[0], C.gt_xywh(C.hand_case()[5][1:2])[0]) == 690 / 1110
    assert list(tab["n_gt"]) == [2, 1, 1, 0]
    for k in C.STAT_NAMES:
        print(k, stats[k], C.HAND_STATS[k])
        assert abs(stats[k] - C.HAND_STATS[k]) <= 1e-12, k
    assert np.all(precision[:, :, 3, :] == -1) and np.all(recall[:, 3, :] == -1)
    assert precision[0, 50, 0, 2] == 1 / (1 + np.spacing(1)) and precision[0, 51, 0, 2] == 2 / (1 + 2 + np.spacing(1)) and scores[0, 51, 0, 2] == np.float32(0.7)


def test_tables_equal_numpy():
    assert np.array_equal(C.IOU_THRS, np.linspace(.5, .95, 10))
    assert np.array_equal(C.REC_THRS, np.linspace(0, 1, 101))
    assert C.IOU_THRS[0] == 0.5 and C.IOU_THRS[5] == 0.75                         # AP50 and AP75 are slices 0 and 5


def test_log_pin_the_reference_saw_the_same_boxes_and_area_classes():
    ann = K.annotations()
    images = [(*C.pad([], []), a["height"], a["width"], np.asarray(a["boxes"], int).reshape(-1, 4)) for a in ann]
    assert list(C.table(images)["n_gt"]) == [105, 1, 61, 43]
    logs = json.load(open(os.path.join(K.GOLDEN, "coco_log_metrics.json")))["dicts"]
    assert len(logs) == 10
    n = 0
    for d in logs:
        m = d["metrics"]
        assert m["AP_/barbell"] == m["AP"]
        for key, mult in (("ARs", 10), ("ARm", 610), ("ARl", 430), ("ARmax1", 1050), ("ARmax10", 1050), ("ARmax100", 1050)):
            v = m[key] * mult
            assert abs(v - round(v)) <= 1e-4, (d["log"], d["line"], key, v)
            n += 1
    assert n == 60


def test_crafted_cases_show_their_rule():
    """conditions on the restatement's own answers: each crafted image does exercise what it is named after"""
    cases = K.crafted()
    bit = lambda a, t: np.uint64(1 << (a * 10 + t))
    t = C.table(cases["tie takes the last"])
    assert t["matched"][0] & bit(0, 5) and not t["matched"][0] & bit(0, 6)                                  # IoU 0.75 with both boxes
    assert all(t["matched"][1] & bit(0, k) for k in range(1, 6))                                            # the first box was left free
    t = C.table(cases["small and medium"])
    assert t["matched"][0] & bit(2, 5) and not t["ignored"][0] & bit(2, 5) and not t["matched"][0] & bit(2, 6)
    assert t["matched"][0] & bit(1, 4) and not t["ignored"][0] & bit(1, 4)                                  # small range, t = 0.7: the small box
    assert t["matched"][0] & bit(1, 5) and t["ignored"][0] & bit(1, 5)                                      # t = 0.75: the ignored medium box
    t = C.table(cases["unmatched outside the range"])
    assert t["ignored"][0] & bit(1, 0) and not t["matched"][0] & bit(1, 0) and not t["ignored"][1] & bit(1, 0)
    t = C.table(cases["iou exactly 0.5"])
    assert t["matched"][0] & bit(0, 0) and not t["matched"][0] & bit(0, 1)
    t = C.table(cases["iou exactly 1"])
    assert all(t["matched"][0] & bit(0, k) for k in range(10))
    t = C.table(cases["areas on the range borders"])
    assert list(t["n_gt"]) == [2, 1, 2, 1]
    assert list(C.table(cases["boxes without detections"])["n_gt"]) == [4, 2, 4, 0]      # 32 x 32 (both ranges) and 70 x 50, twice
    t = C.table(cases["stable sorts"])
    assert list(t["rank"][:5]) == [0, 1, 2, 3, 4] and list(t["score"][:5]) == [0.5, 0.5, 0.25, 0.0, 0.0] and np.signbit(t["score"][3])
    t = C.table(cases["25 detections on 3 boxes"])
    _, recall, _ = C.accumulate(t)
    assert len(t["rank"]) == 25 and recall[0, 0, 0] < recall[0, 0, 1] <= recall[0, 0, 2]
    assert list(C.table(cases["64 boxes"])["n_gt"])[0] == 64
    t = C.table(cases["xmax below xmin"])
    assert t["matched"][0] == 0 and t["matched"][1] & bit(0, 9)
    tab, _, _, _, stats = C.evaluate(K.annotated())
    print("annotated set:", {k: round(v, 4) for k, v in stats.items()}, len(tab["score"]), "rows")
    assert min(stats[k] for k in ("APs", "APm", "APl")) >= 0 and 0.1 < stats["AP"] < 0.9


# ---- the shared core under sanitizers ----

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coco") / "coco_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "fuzz", "coco_check.cc"), "-o", exe])
    return exe


def _run(harness, path):
    return subprocess.run([harness, path], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)


def test_host_program_equals_the_restatement(harness, tmp_path):
    sets = dict(K.crafted(), annotated=K.annotated(), seeded=K.seeded())
    for name, images in sets.items():
        path = str(tmp_path / "case.bin")
        K.write_case(path, images)
        p = _run(harness, path)
        assert p.returncode == 0 and p.stdout.strip() == "ok" and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, \
            (name, p.stdout[-1000:], p.stderr[-3000:])


def test_host_program_sees_a_wrong_bit(harness, tmp_path):
    images = [C.hand_case()]
    tab, precision, recall, scores, stats = C.evaluate(images)
    path = str(tmp_path / "case.bin")
    K.write_case(path, images, (tab, precision, recall, scores, dict(stats, AP=stats["AP"] + 1e-9)))
    p = _run(harness, path)
    assert p.returncode == 1 and "stat 0" in p.stdout, (p.stdout, p.stderr[-2000:])
    data = bytearray(open(str(tmp_path / "case.bin"), "rb").read())
    off = 4 + 16 + 25 * 16 + 25 * 4 + 2 * 16 + 4 + 3 * 4 + 3 * 4                    # the first matched mask of the only image
    data[off] ^= 1
    open(path, "wb").write(bytes(data))
    p = _run(harness, path)
    assert p.returncode == 1 and "image 0 rank 0: matched" in p.stdout, (p.stdout, p.stderr[-2000:])
