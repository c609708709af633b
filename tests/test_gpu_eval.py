"""Detector evaluation on the GPU: the curve kernel against scikit-learn's goldens on the reference's own table and against the CPU
restatement (tests/eval_ref.py) on seeded tables; the match kernel against the restatement (scipy's linear_sum_assignment); and
create_detections_df / the CLI end to end."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import eval_ref
from conftest import GOLDEN, ROOT
from test_eval_host import write_voc

pytestmark = pytest.mark.gpu

CURVE_ARRAYS = ("precision", "recall", "pr_thresholds", "fpr", "tpr", "roc_thresholds")


def _check_curves(got, want, what, want_ap=None, want_auc=None):
    for name in CURVE_ARRAYS:
        g, w = getattr(got, name), want[name] if isinstance(want, dict) else getattr(want, name)
        assert g.shape == w.shape and np.array_equal(g, w, equal_nan=True), (what, name)
    ap = want_ap if want_ap is not None else want.ap
    auc = want_auc if want_auc is not None else want.auc
    d_ap = abs(got.ap - ap) if not np.isnan(ap) else (0.0 if np.isnan(got.ap) else np.inf)
    d_auc = abs(got.auc - auc) if not np.isnan(auc) else (0.0 if np.isnan(got.auc) else np.inf)
    print(f"{what}: n_pr {len(got.precision)} n_roc {len(got.fpr)} |dAP| {d_ap:.3e} |dAUC| {d_auc:.3e}")
    # terms lie in [0, 1] and the sum is <= 1: two summation orders of n terms differ by at most 2 n 2^-53
    assert d_ap <= len(got.precision) * 2.0 ** -52, (what, "ap", got.ap, ap)
    assert d_auc <= len(got.fpr) * 2.0 ** -52, (what, "auc", got.auc, auc)


def test_curves_equal_scikit_learn_on_the_reference_table():
    from vbt_amd import evaluate
    d = np.load(os.path.join(GOLDEN, "eval_detections_ref.npz"))
    gold = np.load(os.path.join(GOLDEN, "eval_curves_ref.npz"))
    for ti, thr in enumerate(gold["iou_thresholds"]):
        for mi, name in enumerate(d["model_names"]):
            sel = d["model"] == mi
            got = evaluate.curves_from_table(d["score"][sel], d["iou"][sel], float(thr))
            k = f"m{mi}_t{ti}_"
            assert np.isinf(got.roc_thresholds[0]) and got.flags == 0 and got.n_rows == int(sel.sum())
            _check_curves(got, {a: gold[k + a] for a in CURVE_ARRAYS}, f"{name} IoU {thr}", float(gold[k + "ap"]), float(gold[k + "auc"]))


def _seeded_tables():
    rng = np.random.Generator(np.random.PCG64(2024))
    yield "float scores", rng.random(5000, dtype=np.float32) * 2 - 0.5, rng.random(5000), 0.5          # non-k/256, some negative
    yield "heavy ties", rng.integers(0, 7, 4000).astype(np.float32) / 3, rng.random(4000), 0.3
    yield "two scores", np.repeat(np.float32([0.25, 0.75]), 50), rng.random(100), 0.5
    yield "all positive", rng.random(300, dtype=np.float32), 0.6 + 0.4 * rng.random(300), 0.5
    yield "all negative", rng.random(300, dtype=np.float32), 0.4 * rng.random(300), 0.5
    yield "one row, positive", np.float32([0.5]), np.array([0.9]), 0.5
    yield "one row, negative", np.float32([0.5]), np.array([0.1]), 0.5
    yield "k/256 scores", rng.integers(0, 256, 30000).astype(np.float32) / 256, rng.random(30000) ** 2, 0.5
    n = 1 << 20
    s = rng.random(n, dtype=np.float32)
    yield "2^20 rows", s, np.clip(s.astype(np.float64) + 0.3 * rng.standard_normal(n), 0, 1), 0.5
    yield "2^20 rows, 256 scores", np.floor(s * 256).astype(np.float32) / 256, np.clip(s.astype(np.float64) + 0.3 * rng.standard_normal(n), 0, 1), 0.75


def test_curves_equal_the_restatement_on_seeded_tables():
    from vbt_amd import evaluate
    for what, scores, ious, thr in _seeded_tables():
        want = eval_ref.curves(scores, ious, thr)
        got = evaluate.curves_from_table(scores, ious, thr)
        assert (got.n_rows, got.n_pos, got.n_neg, got.flags) == (want.n_rows, want.n_pos, want.n_neg, want.flags), what
        _check_curves(got, want, what)
    assert eval_ref.curves(*list(_seeded_tables())[3][1:]).flags == eval_ref.NO_NEGATIVES
    assert eval_ref.curves(*list(_seeded_tables())[4][1:]).flags == eval_ref.NO_POSITIVES


def test_curves_capacity_and_nan():
    from vbt_amd import _lib
    L = _lib.lib()
    sc, io = np.float32([0.1, 0.2, 0.3, 0.4]), np.array([0.9, 0.1, 0.9, 0.1])
    s = _lib.EvalSummary()
    p = np.zeros(8)
    rc = L.vbt_eval_curves_from_table(sc.ctypes.data, io.ctypes.data, 4, 0.5, 0, ctypes.byref(s), p.ctypes.data, None, None, 2, None, None, None, 8)
    assert rc == -4 and s.n_pr == 5 and s.n_rows == 4                      # VBT_ERR_CAPACITY, the summary stays readable
    sc[1] = np.nan
    assert L.vbt_eval_curves_from_table(sc.ctypes.data, io.ctypes.data, 4, 0.5, 0, ctypes.byref(s), None, None, None, 8, None, None, None, 8) == -1


# ---------------------------------------------------------------------------------------------- matching
def _device_match(images, max_batch=64):
    """images: list of (boxes f32 [25,4], scores f32 [25], count, height, width, gt int [n,4]) -> Evaluator.table() via batches"""
    from vbt_amd.evaluate import Evaluator
    from vbt_amd.mem import DeviceBuffer
    ev = Evaluator(len(images) * 25, max_batch)
    keep = []
    for i0 in range(0, len(images), max_batch):
        part = images[i0:i0 + max_batch]
        bufs = [DeviceBuffer.from_host(np.stack([np.asarray(im[k], dt).reshape(shp) for im in part]))
                for k, dt, shp in ((0, np.float32, (25, 4)), (1, np.float32, (25,)), (2, np.int32, ()))]
        keep.append(bufs)
        ev.add(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, [(im[3], im[4]) for im in part], [im[5] for im in part])
    return ev, ev.table()


def _restated_table(images):
    cols = {k: [] for k in ("score", "iou", "image", "det_idx", "gt_idx")}
    for i, (boxes, scores, count, h, w, gt) in enumerate(images):
        s, u, di, gi = eval_ref.match_image(boxes, scores, count, h, w, gt)
        cols["score"].append(s); cols["iou"].append(u); cols["det_idx"].append(di); cols["gt_idx"].append(gi)
        cols["image"].append(np.full(len(s), i, np.int32))
    return {k: np.concatenate(v) for k, v in cols.items()}


def _check_table(got, want):
    for k in ("image", "det_idx", "gt_idx", "score", "iou"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def _pad(boxes, scores):
    b, s = np.zeros((25, 4), np.float32), np.zeros(25, np.float32)
    b[:len(boxes)] = boxes
    s[:len(scores)] = scores
    return b, s, len(boxes)


def _annotations():
    return json.load(open(os.path.join(GOLDEN, "eval_annotations.json")))["images"]


def test_match_reference_annotations_with_the_synthetic_models_detections(model_path):
    """(i) the 61 annotated images of the reference with their real sizes; detections = what the synthetic Lite0 model returns on
    seeded frames (every counted detection: threshold 0)."""
    from vbt_amd import synth
    from vbt_amd.interpreter import Interpreter
    ann = _annotations()
    frames = np.stack([synth.render(synth.background(100 + i), 3 * i) for i in range(len(ann))])
    boxes, scores, _, counts = Interpreter(model_path, max_batch=len(ann)).detect(frames)
    assert counts.max() > 0
    images = [(boxes[i], scores[i], int(counts[i]), a["height"], a["width"], np.asarray(a["boxes"], int).reshape(-1, 4)) for i, a in enumerate(ann)]
    _, got = _device_match(images)
    want = _restated_table(images)
    assert len(want["score"]) == int(counts.sum())                          # n_gt <= n_pred everywhere: every detection is emitted
    _check_table(got, want)


def _crafted_images():
    """(ii) detections built around the reference's ground truth so that the assignment matters."""
    rng = np.random.Generator(np.random.PCG64(7))
    images = []
    for a in _annotations():
        h, w = a["height"], a["width"]
        gt = np.asarray(a["boxes"], np.float64).reshape(-1, 4)
        norm = gt / np.array([h, w, h, w])
        dets = []
        if len(gt) >= 2:
            # the (jittered) union of the first two boxes, which both prefer, + each box shrunk to a fifth of its area: per-box
            # argmax gives both boxes the union, the assignment has to give one of them its shrunk copy
            u = np.r_[np.minimum(norm[0, :2], norm[1, :2]), np.maximum(norm[0, 2:], norm[1, 2:])]
            dets.append(u + rng.normal(0, 0.002, 4))
            for g in norm:
                c, half = (g[:2] + g[2:]) / 2, (g[2:] - g[:2]) / 2
                dets.append(np.r_[c - half * np.sqrt(0.2), c + half * np.sqrt(0.2)])
        else:
            for g in norm:
                dets += [g + rng.normal(0, 0.02, 4), g + rng.normal(0, 0.05, 4)]
        dets.append(dets[0].copy())                                         # an exact duplicate: two detections tie on every box
        dets.append(np.array([0.5, 0.5, 0.5, 0.9]))                         # zero area
        dets.append(np.array([-0.2, -0.1, 0.4, 1.3]))                       # corners outside [0, 1], negative ones truncate up
        dets = np.asarray(dets[:25], np.float32)
        images.append((*_pad(dets, rng.random(len(dets), dtype=np.float32)), h, w, gt.astype(int)))
    big = np.array([[10 * (i // 8), 12 * (i % 8), 10 * (i // 8) + 9, 12 * (i % 8) + 11] for i in range(64)])      # 64 disjoint boxes
    # the solver at the full wave: more boxes than the 25 predictions, so the square problem is n_gt wide and its last n_gt - 25
    # columns are padding, all equal
    spread = np.asarray([big[(5 * i) % 64] + [0, 0, -(i % 3), -(i % 4)] for i in range(25)]) / 100.0       # 25 of the 64 boxes, some cut short
    spread[7], spread[19] = spread[3], (spread[11] + spread[12]) / 2
    images.append((*_pad(np.asarray(spread, np.float32), rng.random(25, dtype=np.float32)), 100, 100, big))         # 64 x 64, 39 padding columns
    twice = [big[3 * (i // 2)] for i in range(24)] + [np.r_[big[1][:2], big[2][2:]]]                      # 12 boxes twice, one span of two
    images.append((*_pad(np.asarray(twice, np.float32) / 100.0, rng.random(25, dtype=np.float32)), 100, 100, big[:40]))  # 40 x 40, exact ties
    shifted = np.asarray([big[i] + [1, 1, 0, 0] for i in rng.permutation(25)], np.float32) / 100.0
    images.append((*_pad(shifted, rng.random(25, dtype=np.float32)), 100, 100, big[:26][::-1].copy()))            # 26 x 26: one above the cap
    some = np.asarray([big[i] / np.array([100, 100, 100, 100]) for i in (5, 17, 17, 40, 63)], np.float32)
    zero = np.zeros((0, 4), int)
    images.append((*_pad(some, rng.random(5, dtype=np.float32)), 100, 100, big))                                    # n_gt = 64 > n_pred
    images.append((*_pad(some, rng.random(5, dtype=np.float32)), 100, 100, zero))                                   # n_gt = 0
    images.append((*_pad(some[:0], []), 100, 100, big[:3]))                                                         # counts = 0
    images.append((*_pad(some[:0], []), 100, 100, zero))                                                            # nothing at all
    images.append((*_pad(some[:2], rng.random(2, dtype=np.float32)), 100, 100, big[:5]))                            # n_gt > n_pred
    images.append((*_pad(np.zeros((3, 4), np.float32), [0.5, 0.5, 0.5]), 50, 50, np.zeros((2, 4), int)))            # union 0 everywhere
    full = np.asarray([big[i] / 100.0 for i in range(25)], np.float32)
    images.append((*_pad(full, rng.random(25, dtype=np.float32)), 100, 100, big[:25][::-1].copy()))                # 25 x 25, a permutation
    return images


def test_match_crafted_detections_exercise_the_solver():
    from scipy.optimize import linear_sum_assignment
    images = _crafted_images()
    # conditions on the INPUTS, checked before the device is consulted
    multi = differs = ties = 0
    for boxes, scores, count, h, w, gt in images:
        if len(gt) < 2 or count < 2 or len(gt) > count:
            continue
        m = eval_ref.iou_matrix(gt, eval_ref.scale_boxes(boxes[:count], h, w))
        multi += 1
        rows, cols = linear_sum_assignment(1 - m)
        differs += not np.array_equal(cols, m.argmax(axis=1))
        ties += any(np.any((m[i][:, None] == m[i][None, :]) & (m[i][:, None] > 0) & ~np.eye(count, dtype=bool)) for i in range(len(gt)))
    assert multi >= 41 and differs * 4 >= multi, (multi, differs)
    assert ties >= 1
    # ... and of the images with more boxes than predictions, on the padded square problem the device solves: its size, whether the
    # assignment differs from every prediction taking its best box, positive exact ties inside a box's row
    tall, tall_differs, tall_ties = [], 0, 0
    for boxes, scores, count, h, w, gt in images:
        if count < 2 or len(gt) <= count:
            continue
        m = eval_ref.iou_matrix(gt, eval_ref.scale_boxes(boxes[:count], h, w))
        sq = np.zeros((len(gt), len(gt)))
        sq[:, :count] = m
        rows, cols = linear_sum_assignment(1 - sq)
        tall.append((len(gt), count))
        tall_differs += not np.array_equal(np.argsort(cols)[:count], m.argmax(axis=0))
        tall_ties += any(np.any((m[i][:, None] == m[i][None, :]) & (m[i][:, None] > 0) & ~np.eye(count, dtype=bool)) for i in range(len(gt)))
    assert {(64, 25), (40, 25), (26, 25)} <= set(tall) and len(tall) >= 5, tall
    assert tall_differs >= 2 and tall_ties >= 2, (tall_differs, tall_ties)
    ev, got = _device_match(images, max_batch=32)
    want = _restated_table(images)
    _check_table(got, want)
    per_image = np.bincount(got["image"], minlength=len(images))
    n = len(images)
    assert list(per_image[n - 7:]) == [5, 5, 0, 0, 2, 3, 25]
    assert list(per_image[n - 10:n - 7]) == [25, 25, 25]                    # more boxes than predictions: every prediction gets a row
    assert np.all(got["gt_idx"][got["image"] == n - 6] >= 0) and np.all(got["iou"][got["image"] == n - 6] == 0)     # n_gt = 0: all dummy rows
    # the curves over the handle's device table equal the table-in form
    from vbt_amd import evaluate
    a, b = ev.curves(0.5), evaluate.curves_from_table(got["score"], got["iou"], 0.5)
    for name in CURVE_ARRAYS:
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name
    assert a.ap == b.ap and a.auc == b.auc and a.n_rows == len(got["score"])
    ev.reset()
    assert len(ev.table()["score"]) == 0


def test_match_capacity_is_an_error_not_a_clip():
    from vbt_amd import _lib
    from vbt_amd.evaluate import Evaluator
    from vbt_amd.mem import DeviceBuffer
    b, s, c = _pad(np.float32([[0.1, 0.1, 0.2, 0.2]]), [0.5])
    bufs = [DeviceBuffer.from_host(x) for x in (np.stack([b, b]), np.stack([s, s]), np.int32([1, 1]))]
    ev = Evaluator(50, 2)
    gt65 = np.array([[i, i, i + 5, i + 5] for i in range(65)])
    with pytest.raises(_lib.VbtError, match="image 1 .* 65 ground-truth boxes"):
        ev.add(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, [(100, 100)] * 2, [gt65[:64], gt65])
    assert _lib.lib().vbt_last_error().decode().startswith("vbt_eval_add_detections")
    assert len(ev.table()["score"]) == 0                                    # nothing was enqueued
    ev.add(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, [(100, 100)] * 2, [gt65[:64], gt65[:1]])
    assert len(ev.table()["score"]) == 2
    small = Evaluator(1, 2)                                                 # a table too small: reported, never a silent clip
    small.add(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, [(100, 100)] * 2, [gt65[:1], gt65[:1]])
    with pytest.raises(_lib.VbtError, match="2 were produced"):
        small.table()


def test_match_bboxes_call_shape():
    from vbt_amd.evaluate import match_bboxes
    gt = np.array([[0, 0, 10, 10], [20, 20, 30, 30]])
    det = np.array([[21, 21, 30, 30], [50, 50, 60, 60], [0, 0, 10, 9], [50, 50, 60, 60], [-5, -5, 4, 4]])
    gi, di, iou = match_bboxes(gt, det)
    wg, wd, wi = eval_ref.match(gt, det)
    assert np.array_equal(gi, wg) and np.array_equal(di, wd) and np.array_equal(iou, wi)
    gi, di, iou = match_bboxes(gt, np.zeros((0, 4), int))
    assert len(gi) == len(di) == len(iou) == 0


# ---------------------------------------------------------------------------------------------- end to end
def _write_dataset(d, sizes_counts):
    from vbt_amd import synth
    rng = np.random.Generator(np.random.PCG64(11))
    k = 0
    for (h, w), n in sizes_counts:
        for _ in range(n):
            img = synth.render(synth.background(500 + k, max(h, w)), 2 * k)[:h, :w]
            name = f"img_{k:03d}.jpg"
            np.save(os.path.join(d, f"img_{k:03d}.npy"), np.ascontiguousarray(img))
            objs = []
            for _ in range(int(rng.integers(0, 4))):
                y0, x0 = int(rng.integers(0, h - 20)), int(rng.integers(0, w - 20))
                objs.append(("barbell", [y0, x0, int(rng.integers(y0 + 5, h)), int(rng.integers(x0 + 5, w))]))
            objs.append(("person", [0, 0, 5, 5]))
            write_voc(os.path.join(d, f"img_{k:03d}.xml"), name, h, w, objs)
            k += 1
    return k


def _expected_df(models, d, annotations):
    """Interpreter-level detections (host resize + vbt_detect) + the CPU restatement, in eval.py's loop order."""
    import pandas as pd
    from vbt_amd import _lib
    from vbt_amd.evaluate import model_name
    from vbt_amd.interpreter import Interpreter
    det = {}
    for m in models:
        it = Interpreter(m, max_batch=1)
        S = int(it.get_input_details()[0]["shape"][1])
        per = {}
        for name in annotations:
            img = np.load(os.path.join(d, os.path.splitext(name)[0] + ".npy"))
            small = np.empty((1, S, S, 3), np.uint8)
            _lib.check(_lib.lib().vbt_resize_frames(img.ctypes.data, 1, img.shape[0], img.shape[1], 0, small.ctypes.data, S, S, 0, 0, 0, None))
            b, s, _, c = it.detect(small)
            per[name] = (b[0], s[0], int(c[0]), img.shape[0], img.shape[1])
        det[model_name(m)] = per
    scores, names, ious = [], [], []
    for name, gt in annotations.items():
        for mname, per in det.items():
            s, u, _, _ = eval_ref.match_image(*per[name], gt)
            scores.append(s); ious.append(u); names += [mname] * len(s)
    return pd.DataFrame({"Score": np.concatenate(scores), "Model": names, "IoU": np.concatenate(ious)})


def test_create_detections_df_and_cli_end_to_end(tmp_path, model_path):
    import pandas as pd
    import shutil
    from vbt_amd import evaluate
    d = str(tmp_path / "data")
    os.makedirs(d)
    n = _write_dataset(d, [((200, 240), 70), ((240, 200), 5)])              # 70 > 64: a batch boundary inside the first size group
    models = [str(tmp_path / "lite0_a.vbtm"), str(tmp_path / "lite0_b.vbtm")]
    for m in models:
        shutil.copy(model_path, m)
    ann = evaluate.read_annotations(d)
    assert len(ann) == n == 75
    want = _expected_df(models, d, ann)
    out = str(tmp_path / "dfs" / "eval.pkl.gz")
    got = evaluate.create_detections_df(models, d, ann, out)
    assert list(got.columns) == ["Score", "Model", "IoU"] and got["Score"].dtype == np.float32 and got["IoU"].dtype == np.float64
    assert len(got) == len(want) > 0
    assert np.array_equal(got["Score"].to_numpy(), want["Score"].to_numpy()) and np.array_equal(got["IoU"].to_numpy(), want["IoU"].to_numpy())
    assert list(got["Model"]) == list(want["Model"]) and set(got["Model"]) == {"lite0_a", "lite0_b"}
    assert pd.read_pickle(out).equals(got)
    # the CLI: creates, then reads instead of recomputing unless --replace_df
    cli_df = str(tmp_path / "cli" / "eval.pkl.gz")
    base = [sys.executable, "-m", "vbt_amd.cli", "eval", *models, "--img_dir", d, "--annotations_dir", d, "--detections_df", cli_df,
            "--iou_threshold", "0.5", "--score_thresholds", "[0.2, 0.5]", "--curve_dir", str(tmp_path / "curves")]
    r = subprocess.run(base, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"Creating dataframe '{cli_df}'." in r.stdout and pd.read_pickle(cli_df).equals(got)
    c = evaluate.curves(got, 0.5)
    for m in ("lite0_a", "lite0_b"):
        assert f"{m}, AP_50={c[m].ap:.4f}, AUC={c[m].auc:.4f}" in r.stdout
        assert os.path.exists(tmp_path / "curves" / f"roc_{m}_iou_0.5.csv") and os.path.exists(tmp_path / "curves" / f"precision_recall_{m}_iou_0.5.csv")
    assert r.stdout.count("ROC threshold") == 4
    marked = pd.read_pickle(cli_df)
    marked.loc[0, "IoU"] = 0.123456                                         # a second run must READ this file, not recompute it
    marked.to_pickle(cli_df)
    r = subprocess.run(base, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"Loading dataframe '{cli_df}'." in r.stdout
    assert pd.read_pickle(cli_df).loc[0, "IoU"] == 0.123456
    r = subprocess.run(base + ["--replace_df"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Creating dataframe" in r.stdout and pd.read_pickle(cli_df).equals(got)
