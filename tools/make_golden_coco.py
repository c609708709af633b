"""Fixture of the COCO metrics (tests/test_coco_ref_host.py), made from the reference tree's DATA:

  tests/golden/coco_log_metrics.json    the metric dicts that model.evaluate / model.evaluate_tflite printed at the end of every
                                        models/*.log of the reference (train.py:64,70), as numbers, with the log's file name and which of
                                        the two lines it was.  Recorded results only.

Runs on the build machine only (needs the reference tree).

    python tools/make_golden_coco.py /path/to/reference
"""
import ast
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl", "ARmax1", "ARmax10", "ARmax100", "ARs", "ARm", "ARl", "AP_/barbell")
LINES = ("evaluate", "evaluate_tflite")          # train.py:64 prints first, train.py:70 second


def main(ref):
    out = []
    for path in sorted(glob.glob(os.path.join(ref, "models", "*.log"))):
        dicts = []
        for line in open(path, encoding="utf-8", errors="replace"):
            line = line.strip()
            if line.startswith("{'AP':") and line.endswith("}"):
                d = ast.literal_eval(line)
                assert tuple(d) == KEYS, (path, tuple(d))
                dicts.append({k: float(v) for k, v in d.items()})
        assert len(dicts) == len(LINES), (path, len(dicts))
        out += [{"log": os.path.basename(path), "line": which, "metrics": d} for which, d in zip(LINES, dicts)]
    with open(os.path.join(GOLDEN, "coco_log_metrics.json"), "w") as f:
        json.dump({"source": "the two metric dicts at the end of every models/*.log of the reference (printed float32 values)", "dicts": out}, f, indent=1)
    print(f"{len(out)} dicts of {len(out) // len(LINES)} logs")


if __name__ == "__main__":
    main(sys.argv[1])
