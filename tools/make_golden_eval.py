"""Fixtures of the detector evaluation (tests/test_eval_host.py, tests/test_gpu_eval.py), made from the reference tree's DATA:

  tests/golden/eval_annotations.json    the 61 test images of the reference's data/test: file name, height, width, `barbell` boxes
  tests/golden/eval_detections_ref.npz  dfs/eval_detections.pkl.gz (the table the reference's eval.py wrote) as plain arrays
  tests/golden/eval_curves_ref.npz      scikit-learn's curves and scalars on that table, per model, IoU thresholds 0.5 and 0.75

Runs on the build machine only (needs the reference tree, pandas and scikit-learn); no test imports scikit-learn.

    python tools/make_golden_eval.py /path/to/reference
"""
import glob
import json
import os
import sys
import xml.etree.ElementTree as ET

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
IOU_THRESHOLDS = (0.5, 0.75)


def annotations(ref):
    out = []
    for f in sorted(glob.glob(os.path.join(ref, "data", "test", "*.xml"))):
        root = ET.parse(f).getroot()
        size = root.find("size")
        boxes = []
        for o in root.findall("object"):
            if o.find("name").text != "barbell":
                continue
            bb = o.find("bndbox")
            boxes.append([int(bb.find(k).text) for k in ("ymin", "xmin", "ymax", "xmax")])
        out.append({"filename": root.find("filename").text, "height": int(size.find("height").text), "width": int(size.find("width").text),
                    "boxes": boxes})
    return out


def main(ref):
    import pandas as pd
    import sklearn
    from sklearn.metrics import average_precision_score, precision_recall_curve, roc_auc_score, roc_curve

    ann = annotations(ref)
    with open(os.path.join(GOLDEN, "eval_annotations.json"), "w") as f:
        json.dump({"source": "data/test/*.xml of the reference, label 'barbell'; boxes are ymin,xmin,ymax,xmax", "images": ann}, f, indent=0)

    df = pd.read_pickle(os.path.join(ref, "dfs", "eval_detections.pkl.gz"))
    names = list(pd.unique(df["Model"]))
    model = np.asarray([names.index(m) for m in df["Model"]], np.int32)
    score, iou = df["Score"].to_numpy(), df["IoU"].to_numpy()
    assert score.dtype == np.float32 and iou.dtype == np.float64
    np.savez_compressed(os.path.join(GOLDEN, "eval_detections_ref.npz"), score=score, iou=iou, model=model, model_names=np.asarray(names))

    out = {"model_names": np.asarray(names), "iou_thresholds": np.asarray(IOU_THRESHOLDS),
           "versions": np.asarray([f"scikit-learn {sklearn.__version__}", f"numpy {np.__version__}"])}
    for ti, thr in enumerate(IOU_THRESHOLDS):
        for mi in range(len(names)):
            s, lab = score[model == mi], iou[model == mi] > thr
            p, r, t = precision_recall_curve(lab, s)
            fpr, tpr, rt = roc_curve(lab, s)
            k = f"m{mi}_t{ti}_"
            out.update({k + "precision": p, k + "recall": r, k + "pr_thresholds": t, k + "fpr": fpr, k + "tpr": tpr, k + "roc_thresholds": rt,
                        k + "ap": np.float64(average_precision_score(lab, s)), k + "auc": np.float64(roc_auc_score(lab, s))})
    np.savez_compressed(os.path.join(GOLDEN, "eval_curves_ref.npz"), **out)
    print(f"{len(ann)} images, {sum(len(a['boxes']) for a in ann)} boxes, {len(score)} rows, {len(names)} models")


if __name__ == "__main__":
    main(sys.argv[1])
