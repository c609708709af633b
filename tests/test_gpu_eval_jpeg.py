"""`eval` on .jpg files decoded on the GPU (vbt_amd/evaluate.py, vbt_amd/stills.py): a directory of baseline .jpg of three sizes and
samplings, one progressive .jpg and one .png must give EXACTLY the DataFrame that the same pixels give as .npy files (Pillow-decoded,
BGR: the route before the GPU decoder) - Score, Model and IoU, array_equal."""
import os
import shutil

import numpy as np
import pytest

import mjpeg_dec_ref as D
from test_eval_host import write_voc

pytestmark = pytest.mark.gpu

# (H, W), Pillow's subsampling, how many: 4:2:0, 4:4:4, 4:2:2 - interleaved below so that neighbours in a batch differ
KINDS = (((48, 64), 2, 4), ((40, 56), 0, 3), ((33, 17), 1, 3))


def write_datasets(jpg_dir, npy_dir):
    """the same images twice: as .jpg / .png files, and as the .npy of what Pillow decodes from them in BGR order"""
    from PIL import Image
    from vbt_amd import synth
    rng = np.random.Generator(np.random.PCG64(5))
    todo = [(hw, sub, i) for hw, sub, n in KINDS for i in range(n)]
    todo.sort(key=lambda t: t[2])                                                  # round-robin over the kinds
    files = [("jpg", hw, dict(quality=90, subsampling=sub)) for hw, sub, _ in todo]
    files.insert(4, ("jpg", (40, 56), dict(quality=90, subsampling=2, progressive=True)))
    files.insert(7, ("png", (48, 64), {}))
    for k, (ext, (h, w), kw) in enumerate(files):
        img = synth.render(synth.background(700 + k, 64), 3 * k)[:h, :w]
        img = np.ascontiguousarray((img.astype(np.int32) + D.smooth(h, w, k) // 4).clip(0, 255).astype(np.uint8))
        stem = f"img_{k:03d}"
        path = os.path.join(jpg_dir, f"{stem}.{ext}")
        if ext == "jpg":
            with open(path, "wb") as f:
                f.write(D.pil_jpeg(img, **kw))
        else:
            Image.fromarray(img).save(path)
        with Image.open(path) as im:
            np.save(os.path.join(npy_dir, stem + ".npy"), np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1]))
        objs = []
        for _ in range(int(rng.integers(1, 4))):
            y0, x0 = int(rng.integers(0, h - 10)), int(rng.integers(0, w - 10))
            objs.append(("barbell", [y0, x0, int(rng.integers(y0 + 5, h)), int(rng.integers(x0 + 5, w))]))
        for d in (jpg_dir, npy_dir):
            write_voc(os.path.join(d, stem + ".xml"), f"{stem}.{ext}" if d == jpg_dir else f"{stem}.jpg", h, w, objs)
    return [f"img_{k:03d}.{ext}" for k, (ext, _, _) in enumerate(files)]


def same_df(a, b):
    return (len(a) == len(b) and np.array_equal(a["Score"].to_numpy(), b["Score"].to_numpy()) and np.array_equal(a["IoU"].to_numpy(), b["IoU"].to_numpy())
            and list(a["Model"]) == list(b["Model"]))


def test_eval_on_jpg_equals_eval_on_the_decoded_pixels(tmp_path, model_path, monkeypatch):
    import pandas as pd
    from vbt_amd import evaluate
    jpg_dir, npy_dir = str(tmp_path / "jpg"), str(tmp_path / "npy")
    os.makedirs(jpg_dir), os.makedirs(npy_dir)
    names = write_datasets(jpg_dir, npy_dir)
    assert len(names) == 12
    models = [str(tmp_path / "lite0_a.vbtm"), str(tmp_path / "lite0_b.vbtm")]
    for m in models:
        shutil.copy(model_path, m)
    ann = evaluate.read_annotations(jpg_dir)
    ann_npy = evaluate.read_annotations(npy_dir)
    assert list(ann) == names and len(ann_npy) == 12
    heads = {n: evaluate.jpeg_header(os.path.join(jpg_dir, n)) for n in names if n.endswith(".jpg")}
    assert "SOF2" in heads["img_004.jpg"] and sum(not isinstance(h, str) for h in heads.values()) == 10
    assert {h[:2] for h in heads.values() if not isinstance(h, str)} == {(48, 64), (40, 56), (33, 17)}
    assert evaluate.image_size(os.path.join(jpg_dir, "img_000.jpg")) == (48, 64) and evaluate.image_size(os.path.join(jpg_dir, "img_004.jpg")) == (40, 56)

    want = evaluate.create_detections_df(models, npy_dir, ann_npy)                 # today's route: decoded BGR pixels from the host
    assert len(want) > 0 and set(want["Model"]) == {"lite0_a", "lite0_b"}

    # auto: ten files through the GPU decoder, the progressive one and the .png through the host route - and Pillow decodes only those
    import PIL.Image
    opened = []
    real_open = PIL.Image.open
    monkeypatch.setattr(PIL.Image, "open", lambda p, *a, **k: (opened.append(os.path.basename(str(p))), real_open(p, *a, **k))[1])
    images = [(n, os.path.join(jpg_dir, n)) for n in names]
    srt = evaluate.SortedImages(images)
    assert srt.stills == [n for n in names if not isinstance(heads.get(n, ""), str)] and srt.host == ["img_004.jpg", "img_007.png"]
    assert all(srt.data[n] == open(os.path.join(jpg_dir, n), "rb").read() for n in srt.stills)
    assert sum(srt.heads[n][2] for n in srt.stills) == 4 * 72 + 3 * 105 + 3 * 40          # the decoder's block budget here: 723, not the cap of 2^22
    table, order = evaluate.detections_table(models[0], images, ann, sorted_images=srt)
    assert sorted(order) == sorted(names) and order[:10] == srt.stills
    assert set(opened) == {"img_004.jpg", "img_007.png"}
    assert set(np.unique(table["image"])) == set(range(12))                        # every file, the two host-route ones included, has rows
    monkeypatch.undo()

    # the CLI end to end, in its default mode (auto): the DataFrame of the .npy route, exactly
    from click.testing import CliRunner
    from vbt_amd.cli import main
    cli_df = str(tmp_path / "cli" / "eval.pkl.gz")
    base = ["eval", *models, "--img_dir", jpg_dir, "--annotations_dir", jpg_dir, "--detections_df", cli_df]
    r = CliRunner().invoke(main, base)
    assert r.exit_code == 0, r.output
    got = pd.read_pickle(cli_df)
    assert got["Score"].dtype == np.float32 and got["IoU"].dtype == np.float64
    assert same_df(got, want), (len(got), len(want))
    c = evaluate.curves(want, 0.5)
    for m in ("lite0_a", "lite0_b"):
        assert f"{m}, AP_50={c[m].ap:.4f}, AUC={c[m].auc:.4f}" in r.output
    # host equals auto
    assert same_df(evaluate.create_detections_df(models[:1], jpg_dir, ann, jpeg_decode="host"), got[got["Model"] == "lite0_a"])
    # gpu: the file the decoder refuses is an error that names it and the reason, from the API and from the CLI
    with pytest.raises(evaluate.JpegRefused, match=r"img_004\.jpg.*SOF2"):
        evaluate.create_detections_df(models[:1], jpg_dir, ann, jpeg_decode="gpu")
    r = CliRunner().invoke(main, base + ["--replace_df", "--jpeg_decode", "gpu"])
    assert r.exit_code == 2 and "img_004.jpg" in r.output and "SOF2" in r.output, r.output

    # a damaged scan raises, naming the file
    bad_dir = str(tmp_path / "bad")
    shutil.copytree(jpg_dir, bad_dir)
    victim = os.path.join(bad_dir, "img_002.jpg")
    data = open(victim, "rb").read()
    with open(victim, "wb") as f:
        f.write(D.damaged_frame(data))
    status = D.decode(D.damaged_frame(data), with_status=True)[1]
    assert status != 0
    assert issubclass(evaluate.JpegDamaged, ValueError) and not issubclass(evaluate.JpegDamaged, evaluate.JpegRefused)
    r = CliRunner().invoke(main, ["eval", models[0], "--img_dir", bad_dir, "--annotations_dir", jpg_dir, "--detections_df", str(tmp_path / "bad.pkl.gz")])
    assert r.exit_code == 1 and f"img_002.jpg: damaged JPEG scan (status {status}:" in r.output, r.output      # bad data, not bad usage
