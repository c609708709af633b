"""Detector evaluation, CPU side: the vbt_eval_* ABI is exported and bound, the annotation reader, and the reference-held pins of the
CPU restatement (tests/eval_ref.py) that the GPU tests use as their yardstick: its curves on the reference's own detections table
(tests/golden/eval_detections_ref.npz = dfs/eval_detections.pkl.gz) equal scikit-learn's (tests/golden/eval_curves_ref.npz)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import eval_ref
from conftest import GOLDEN, ROOT

EVAL_SYMBOLS = ("vbt_eval_create", "vbt_eval_destroy", "vbt_eval_reset", "vbt_eval_add_detections", "vbt_eval_table", "vbt_eval_curves",
                "vbt_eval_curves_from_table")


def _ref_table():
    d = np.load(os.path.join(GOLDEN, "eval_detections_ref.npz"))
    return d["score"], d["iou"], d["model"], [str(m) for m in d["model_names"]]


def test_eval_symbols_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib
    L = _lib.lib()
    for n in EVAL_SYMBOLS:
        assert hasattr(L, n), f"libvbt_hip.so does not export {n}"
        assert n in _lib.declared_symbols(), f"{n} is not bound in vbt_amd/_lib.py"


def test_eval_create_without_gpu_is_a_hip_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vbt_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.vbt_eval_create(0, 64, 1600, ctypes.byref(h)) == -3          # VBT_ERR_HIP, like every other *_create
    assert not h.value
    s = _lib.EvalSummary()
    sc, io = np.zeros(4, np.float32), np.zeros(4)
    assert L.vbt_eval_curves_from_table(sc.ctypes.data, io.ctypes.data, 4, 0.5, 0, ctypes.byref(s), None, None, None, 0, None, None, None, 0) == -3
    from vbt_amd import evaluate
    with pytest.raises(_lib.VbtError):
        evaluate.curves_from_table(sc, io)


VOC = """<annotation><folder></folder><filename>{name}</filename><size><width>{w}</width><height>{h}</height><depth>3</depth></size>
{objects}</annotation>"""
OBJ = "<object><name>{label}</name><bndbox><xmin>{b[1]}</xmin><xmax>{b[3]}</xmax><ymin>{b[0]}</ymin><ymax>{b[2]}</ymax></bndbox></object>"


def write_voc(path, name, h, w, objects):
    with open(path, "w") as f:
        f.write(VOC.format(name=name, h=h, w=w, objects="".join(OBJ.format(label=lab, b=b) for lab, b in objects)))


def test_read_annotations(tmp_path):
    from vbt_amd.evaluate import read_annotations
    want = {"b.jpg": [[10, 20, 110, 220], [5, 6, 7, 8]], "a.jpg": [[1, 2, 3, 4]], "c.jpg": []}
    write_voc(tmp_path / "x2.xml", "b.jpg", 416, 416, [("barbell", want["b.jpg"][0]), ("person", [0, 0, 9, 9]), ("barbell", want["b.jpg"][1])])
    write_voc(tmp_path / "x1.xml", "a.jpg", 1080, 1920, [("barbell", want["a.jpg"][0])])
    write_voc(tmp_path / "x3.xml", "c.jpg", 100, 50, [("plate", [1, 1, 2, 2])])
    (tmp_path / "notes.txt").write_text("not an annotation")
    got = read_annotations(str(tmp_path))
    assert list(got) == ["a.jpg", "b.jpg", "c.jpg"]                        # sorted XML file order
    for k, v in want.items():
        assert got[k].shape == (len(v), 4) and np.issubdtype(got[k].dtype, np.integer)
        assert np.array_equal(got[k], np.asarray(v, int).reshape(-1, 4))
    assert got.sizes == {"a.jpg": (1080, 1920), "b.jpg": (416, 416), "c.jpg": (100, 50)}
    other = read_annotations(str(tmp_path), label="person")
    assert np.array_equal(other["b.jpg"], [[0, 0, 9, 9]]) and len(other["a.jpg"]) == 0


def test_restatement_curves_equal_scikit_learn_on_the_reference_table():
    score, iou, model, names = _ref_table()
    gold = np.load(os.path.join(GOLDEN, "eval_curves_ref.npz"))
    assert len(score) == 9150 and len(names) == 6
    assert np.array_equal(score * 256, np.round(score * 256))             # dequantised int8 scores: every value k/256
    for ti, thr in enumerate(gold["iou_thresholds"]):
        for mi in range(6):
            c = eval_ref.curves(score[model == mi], iou[model == mi], float(thr))
            k = f"m{mi}_t{ti}_"
            for name in ("precision", "recall", "pr_thresholds", "fpr", "tpr", "roc_thresholds"):
                assert np.array_equal(getattr(c, name), gold[k + name]), (names[mi], thr, name)
            assert np.isinf(c.roc_thresholds[0])
            # terms in [0, 1], sum <= 1: two summation orders of n terms differ by at most 2 n 2^-53
            assert abs(c.ap - float(gold[k + "ap"])) <= len(c.precision) * 2.0 ** -52
            assert abs(c.auc - float(gold[k + "auc"])) <= len(c.fpr) * 2.0 ** -52
            assert c.flags == 0


def test_reference_table_row_order_is_gt_rows_first():
    """What match_bboxes emits (eval.py:96-153): per (file, model) group of 25 rows, rows with IoU > 0 only among the first n_gt
    (the padded matrix's ground-truth rows), then the dummy rows with IoU 0 and non-increasing scores."""
    score, iou, model, names = _ref_table()
    ann = json.load(open(os.path.join(GOLDEN, "eval_annotations.json")))["images"]
    assert len(ann) == 61 and sum(len(a["boxes"]) for a in ann) == 105
    assert sorted({(a["height"], a["width"]) for a in ann}) == [(416, 416), (1920, 1080)]
    assert sum((a["height"], a["width"]) == (416, 416) for a in ann) == 59
    hist_gt = np.bincount([len(a["boxes"]) for a in ann], minlength=5)
    assert list(hist_gt) == [0, 20, 39, 1, 1]
    groups = score.reshape(61, 6, 25), iou.reshape(61, 6, 25), model.reshape(61, 6, 25)
    assert np.array_equal(groups[2], np.broadcast_to(np.arange(6)[None, :, None], (61, 6, 25)))     # file outer, model inner
    lead = np.zeros((61, 6), int)
    for f in range(61):
        for m in range(6):
            s, u = groups[0][f, m], groups[1][f, m]
            nz = np.nonzero(u > 0)[0]
            lead[f, m] = nz.max() + 1 if len(nz) else 0
    n_lead = lead.max(axis=1)                                              # leading rows of the file = its number of boxes
    assert list(np.bincount(n_lead, minlength=5)) == [0, 20, 39, 1, 1]
    for f in range(61):
        for m in range(6):
            s, u = groups[0][f, m], groups[1][f, m]
            assert np.all(u[n_lead[f]:] == 0)
            assert np.all(np.diff(s[n_lead[f]:]) <= 0)


def test_restatement_degenerate_tables():
    s = np.array([0.5, 0.25, 0.25, 0.75], np.float32)
    c = eval_ref.curves(s, np.zeros(4), 0.5)
    assert c.flags == eval_ref.NO_POSITIVES and np.isnan(c.ap) and np.isnan(c.auc) and np.all(np.isnan(c.tpr)) and not np.any(np.isnan(c.fpr))
    c = eval_ref.curves(s, np.ones(4), 0.5)
    assert c.flags == eval_ref.NO_NEGATIVES and c.ap == 1.0 and np.isnan(c.auc) and np.all(np.isnan(c.fpr))


def test_restatement_match_follows_scipy_row_order():
    gt = np.array([[0, 0, 10, 10], [20, 20, 30, 30]])
    det = np.array([[21, 21, 30, 30], [50, 50, 60, 60], [0, 0, 10, 9], [50, 50, 60, 60]])
    gi, di, iou = eval_ref.match(gt, det)
    assert list(gi[:2]) == [0, 1] and list(di[:2]) == [2, 0] and iou[0] == 0.9 and iou[1] == 0.81
    assert sorted(di[2:]) == [1, 3] and np.all(iou[2:] == 0) and list(gi[2:]) == [2, 3]
    gi, di, iou = eval_ref.match(gt, np.zeros((0, 4), int))
    assert len(gi) == 0
    gi, di, iou = eval_ref.match(np.zeros((0, 4), int), det)
    assert list(di) == [0, 1, 2, 3] and np.all(iou == 0)


def test_evaluate_imports_neither_torch_nor_oracle():
    code = "import sys; import vbt_amd.evaluate; bad = [m for m in sys.modules if m == 'torch' or m.split('.')[0] in ('oracle', 'scipy', 'sklearn')]; print(bad); sys.exit(1 if bad else 0)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    src = open(os.path.join(ROOT, "vbt_amd", "evaluate.py")).read()
    assert "import torch" not in src and "oracle" not in src
