"""COCO metrics on the GPU (include/vbt_hip.h, "COCO metrics"; vbt_amd/csrc/evaluate_coco.hip) against the numpy restatement
(tests/coco_ref.py, pinned by tests/test_coco_ref_host.py - not by pycocotools, which is not installed here): crafted device arrays,
one rule of COCOeval.evaluateImg each, the reference's 61 annotated images with two detection sets, seeded images added in batches of
1, 7 and 64 on two streams, the capacities, and `cli eval --coco --coco_dump` end to end.
Comparison: rows (score, image, rank, masks), n_gt and the precision / recall / scores arrays with array_equal - every entry is a
quotient of integers, or one double addition and one division; the 12 stats within 1e-12 - they differ from np.mean by the summation
order only: at most 1010 addends in [0, 1], a sequential-sum error of at most 1010 * 2^-53 ~ 1.1e-13 relative to a mean <= 1."""
import ast
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import coco_cases as K
import coco_ref as C
from conftest import ROOT
from test_eval_host import write_voc

pytestmark = pytest.mark.gpu

ROW_COLUMNS = ("score", "image", "rank", "matched", "ignored")


def _buffers(part):
    from vbt_amd.mem import DeviceBuffer
    return [DeviceBuffer.from_host(np.stack([np.asarray(im[k], dt).reshape(shp) for im in part]))
            for k, dt, shp in ((0, np.float32, (25, 4)), (1, np.float32, (25,)), (2, np.int32, ()))]


def _device(images, max_batch=64, streams=None, rows_cap=None):
    """images through a CocoEvaluator in batches of max_batch (on `streams` alternately): (evaluator, table, CocoResult)"""
    from vbt_amd.evaluate import CocoEvaluator
    ev = CocoEvaluator(rows_cap or max(1, len(images) * 25), max_batch)
    keep = []
    for j, i0 in enumerate(range(0, len(images), max_batch)):
        part = images[i0:i0 + max_batch]
        bufs = _buffers(part)
        keep.append(bufs)
        ev.add(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, [(im[3], im[4]) for im in part], [im[5] for im in part],
               streams[j % len(streams)] if streams else None)
    return ev, ev.table(), ev.accumulate()


def _check(got_tab, got, want, what):
    tab, precision, recall, scores, stats = want
    for k in ROW_COLUMNS:
        assert got_tab[k].dtype == tab[k].dtype and np.array_equal(got_tab[k], tab[k]), (what, k)
    assert np.array_equal(np.signbit(got_tab["score"]), np.signbit(tab["score"])), what
    assert np.array_equal(got.n_gt, tab["n_gt"]) and got.n_rows == len(tab["score"]) and got.n_images == tab["n_images"], what
    assert np.array_equal(got.precision, precision), what
    assert np.array_equal(got.recall, recall), what
    assert np.array_equal(got.scores, scores), what
    worst = max(abs(got.stats[k] - stats[k]) for k in C.STAT_NAMES)
    print(f"{what}: {got.n_rows} rows, n_gt {list(got.n_gt)}, AP {got.stats['AP']:.6f}, max |d stat| {worst:.3e}")
    for k in C.STAT_NAMES:
        assert abs(got.stats[k] - stats[k]) <= 1e-12, (what, k, got.stats[k], stats[k])


def test_hand_worked_image():
    images = [C.hand_case()]
    _, tab, res = _device(images)
    _check(tab, res, C.evaluate(images), "hand-worked")
    for k in C.STAT_NAMES:
        assert abs(res.stats[k] - C.HAND_STATS[k]) <= 1e-12, k
    assert res.metrics()["AP_/barbell"] == res.stats["AP"] and list(res.metrics()) == list(C.STAT_NAMES) + ["AP_/barbell"]


@pytest.mark.parametrize("name", sorted(K.crafted()))
def test_crafted_images_one_rule_each(name):
    images = K.crafted()[name]
    _, tab, res = _device(images)
    _check(tab, res, C.evaluate(images), name)


def test_all_crafted_images_in_one_table():
    images = [im for _, ims in sorted(K.crafted().items()) for im in ims]
    _, tab, res = _device(images, max_batch=8)
    _check(tab, res, C.evaluate(images), "all crafted")


def test_reference_annotations_with_the_synthetic_models_detections(model_path):
    from vbt_amd import synth
    from vbt_amd.interpreter import Interpreter
    ann = K.annotations()
    frames = np.stack([synth.render(synth.background(100 + i), 3 * i) for i in range(len(ann))])
    boxes, scores, _, counts = Interpreter(model_path, max_batch=len(ann)).detect(frames)
    assert counts.max() > 0
    images = [(boxes[i], scores[i], int(counts[i]), a["height"], a["width"], np.asarray(a["boxes"], int).reshape(-1, 4)) for i, a in enumerate(ann)]
    _, tab, res = _device(images)
    assert list(res.n_gt) == [105, 1, 61, 43]
    _check(tab, res, C.evaluate(images), "Lite0 detections")


def test_reference_annotations_with_seeded_detections():
    images = K.annotated()
    want = C.evaluate(images)
    assert min(want[4][k] for k in ("APs", "APm", "APl")) >= 0                # all three area classes are populated
    _, tab, res = _device(images)
    _check(tab, res, want, "seeded detections")


def test_seeded_images_in_batches_and_on_two_streams():
    from vbt_amd import _lib
    L = _lib.lib()
    images = K.seeded()
    want = C.evaluate(images)
    streams = [ctypes.c_void_p(), ctypes.c_void_p()]
    for s in streams:
        _lib.check(L.vbt_stream_create(0, ctypes.byref(s)))
    try:
        results = [_device(images, max_batch=b, streams=streams) for b in (1, 7, 64)]
        for (_, tab, res), b in zip(results, (1, 7, 64)):
            _check(tab, res, want, f"batches of {b}")
        for _, tab, res in results[1:]:
            for k in ROW_COLUMNS:
                assert np.array_equal(tab[k], results[0][1][k]), k
            assert res.stats == results[0][2].stats and np.array_equal(res.precision, results[0][2].precision)
        del results
    finally:
        for s in streams:
            L.vbt_stream_synchronize(s)
            L.vbt_stream_destroy(s)


def test_capacity_is_an_error_not_a_clip():
    from vbt_amd import _lib
    from vbt_amd.evaluate import CocoEvaluator
    images = K.crafted()["25 detections on 3 boxes"] * 2
    bufs = _buffers(images)
    hw, gts = [(im[3], im[4]) for im in images], [im[5] for im in images]
    small = CocoEvaluator(30, 2)                                            # 50 rows come
    small.add(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, hw, gts)
    with pytest.raises(_lib.VbtError, match="50 were produced"):
        small.table()
    with pytest.raises(_lib.VbtError, match="50 were produced"):
        small.accumulate()
    small.reset()                                                           # the call can be repeated after a reset
    small.add(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, hw[:1], gts[:1])
    _check(small.table(), small.accumulate(), C.evaluate(images[:1]), "after reset")
    ev = CocoEvaluator(50, 2)
    gt65 = np.array([[i, i, i + 5, i + 5] for i in range(65)])
    with pytest.raises(_lib.VbtError, match="image 1 .* 65 ground-truth boxes"):
        ev.add(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, hw, [gt65[:64], gt65])
    assert _lib.lib().vbt_last_error().decode().startswith("vbt_coco_add_detections")
    res = ev.accumulate()
    assert len(ev.table()["score"]) == 0 and res.n_images == 0 and list(res.n_gt) == [0, 0, 0, 0]     # nothing was enqueued
    assert all(v == -1 for v in res.stats.values()) and np.all(res.precision == -1)
    three = _buffers(images + images[:1])
    with pytest.raises(_lib.VbtError, match="3 images, the handle takes 2"):
        ev.add(three[0].ptr, three[1].ptr, three[2].ptr, hw + hw[:1], gts + gts[:1])
    assert len(ev.table()["score"]) == 0


def _write_dataset(d):
    """three images of two sizes, one of them a .jpg; returns {name: path}"""
    from PIL import Image
    from vbt_amd import synth
    rng = np.random.Generator(np.random.PCG64(13))
    for k, (h, w) in enumerate(((200, 240), (200, 240), (240, 200))):
        img = synth.render(synth.background(700 + k, max(h, w)), 2 * k)[:h, :w]
        if k == 1:
            Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(os.path.join(d, f"img_{k:03d}.jpg"), quality=92)
        else:
            np.save(os.path.join(d, f"img_{k:03d}.npy"), np.ascontiguousarray(img))
        objs = []
        for _ in range(2):
            y0, x0 = int(rng.integers(0, h - 60)), int(rng.integers(0, w - 60))
            objs.append(("barbell", [y0, x0, int(rng.integers(y0 + 20, h)), int(rng.integers(x0 + 20, w))]))
        objs.append(("person", [0, 0, 5, 5]))
        write_voc(os.path.join(d, f"img_{k:03d}.xml"), f"img_{k:03d}.jpg", h, w, objs)


def test_cli_coco_and_dump_end_to_end(tmp_path, model_path):
    import pandas as pd
    import shutil
    from vbt_amd import evaluate
    d = str(tmp_path / "data")
    os.makedirs(d)
    _write_dataset(d)
    model = str(tmp_path / "lite0_a.vbtm")
    shutil.copy(model_path, model)
    ann = evaluate.read_annotations(d)
    images = [(name, evaluate.find_image(d, name)) for name in ann]
    assert sorted(os.path.splitext(p)[1] for _, p in images) == [".jpg", ".npy", ".npy"]
    want = evaluate.coco_metrics(model, images, ann)
    assert tuple(want) == evaluate.COCO_KEYS and want["AP_/barbell"] == want["AP"]
    df, dump = str(tmp_path / "dfs" / "eval.pkl.gz"), str(tmp_path / "dump")
    base = [sys.executable, "-m", "vbt_amd.cli", "eval", model, "--img_dir", d, "--annotations_dir", d, "--detections_df", df]
    r = subprocess.run(base + ["--coco_dump", dump], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--coco_dump needs --coco" in r.stderr and not os.path.exists(df)
    r = subprocess.run(base + ["--coco", "--coco_dump", dump], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("lite0_a: {")]
    assert len(lines) == 1 and r.stdout.index("lite0_a, AP_50=") < r.stdout.index(lines[0])      # after the existing output
    got = ast.literal_eval(lines[0][len("lite0_a: "):])
    assert got == {k: float(str(np.float32(v))) for k, v in want.items()} and list(got) == list(evaluate.COCO_KEYS)
    # the dump, through the restatement: the same stats
    inst = json.load(open(os.path.join(dump, "instances.json")))
    dets = json.load(open(os.path.join(dump, "lite0_a_detections.json")))
    assert [a["id"] for a in inst["annotations"]] == list(range(1, 7)) and all(a["iscrowd"] == 0 and a["area"] == a["bbox"][2] * a["bbox"][3] for a in inst["annotations"])
    assert inst["categories"] == [{"id": 1, "name": "barbell"}] and [im["id"] for im in inst["images"]] == [1, 2, 3]
    stats = _stats_of_dump(inst, dets)
    for k in C.STAT_NAMES:
        assert abs(stats[k] - want[k]) <= 1e-12, (k, stats[k], want[k])
    # the DataFrame: written because it was missing, not rewritten without --replace_df
    marked = pd.read_pickle(df)
    assert len(marked) > 0
    marked.loc[0, "IoU"] = 0.123456
    marked.to_pickle(df)
    r = subprocess.run(base + ["--coco"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"Loading dataframe '{df}'." in r.stdout and lines[0] in r.stdout
    assert pd.read_pickle(df).loc[0, "IoU"] == 0.123456


def _stats_of_dump(inst, dets):
    """the restatement on the dump's own xywh boxes (no corner arithmetic: the files hold what pycocotools would read)"""
    per_image = {im["id"]: {"gt": [], "det": [], "scores": []} for im in inst["images"]}
    for a in inst["annotations"]:
        per_image[a["image_id"]]["gt"].append(a["bbox"] + [a["area"]])
    for r in dets:
        per_image[r["image_id"]]["det"].append(r["bbox"] + [r["bbox"][2] * r["bbox"][3]])
        per_image[r["image_id"]]["scores"].append(r["score"])
    return C.evaluate([per_image[im["id"]] for im in inst["images"]])[4]
