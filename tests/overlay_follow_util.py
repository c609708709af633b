"""What the follow-mode tests share (tests/test_overlay_follow_host.py, tests/test_gpu_overlay_follow.py): a DataFrame-shaped dict as
the row log a tracker would emit, and the reference's integers (tests/overlay_ref.py, sorted mode) brought into log order."""
import numpy as np

import overlay_ref as R

ROW = np.dtype([("id", "<i8"), ("time", "<f8"), ("x", "<f8"), ("y", "<f8"), ("dx", "<f8"), ("dy", "<f8"), ("h", "<f8"), ("w", "<f8")])
FIELD = dict(zip(R.COLUMNS, ROW.names))            # DataFrame column -> record field
BAD_ROW, ORDER, FRAME_RANGE, FRAME_FULL, REWOUND = 1, 2, 4, 8, 16


def emission_log(data):
    """the 64-byte records of `data` in emission order: by time, the ids of one frame ascending (stable)"""
    n = len(data["id"])
    log = np.zeros(n, ROW)
    for k in R.COLUMNS:
        log[FIELD[k]] = np.asarray(data[k])
    return log[np.lexsort((log["id"], log["time"]))]


def as_data(log):
    return {k: log[FIELD[k]].tolist() for k in R.COLUMNS}


def reference(log, fps, H, W, trail=120):
    """(int64 [n, 8] geometry in LOG order, list of [L, 2] trail centres per log row, the newest first) from the sorted-mode reference"""
    data = as_data(log)
    s = R.sorted_rows(data)
    g = R.geometry(s, fps, H, W, trail=trail)
    order = np.lexsort((log["time"], log["id"]))    # sorted position k holds log row order[k] (both sorts are stable)
    geo = np.zeros_like(g)
    trails = [None] * len(log)
    for k, i in enumerate(order):
        geo[i] = g[k]
        L = int(g[k, 7])
        trails[i] = g[k - L + 1:k + 1, 1:3][::-1]
    return geo, trails


def frames_of(log, fps):
    return np.rint(log["time"] * fps).astype(np.int64)
