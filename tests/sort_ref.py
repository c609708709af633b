"""numpy restatement of `sort.tracker.SortTracker` (sort-track 0.0.8), the commented-out alternative of reference track.py:16,156 that
made the reference's dfs/ result set.  TEST INFRASTRUCTURE ONLY.  The package is not vendored and its text is not copied: this is
the published SORT algorithm [EXTERNAL: Bewley et al., "Simple Online and Realtime Tracking"] in the call shape the reference uses,
with the filter constants and IoU of oracle/ocsort_np.py (the same 7-state filter), fitted to the reference's committed DataFrames
(tests/test_sort_ref_host.py, fixture tests/golden/dfs_sort.npz from tools/make_golden_sort.py).

Per update(dets[N,6] = x1,y1,x2,y2,score,cls):
  1. frame_count += 1
  2. every track predicts (vs clamp, filter predict, age, hit_streak reset after a miss, time_since_update); a track whose predicted
     box holds a NaN is removed
  3. association on IoU alone: the hits of (iou > thr) if every row and column has at most one and there is one at all, else the
     linear assignment on -iou; a pair with iou < thr is undone (its detection goes BEHIND the never-paired ones)
  4. matched tracks: counters, filter update with z = [cx, cy, w*h, w/h] (no 1e-6), score and class of the detection
  5. every unmatched detection starts a track (ids from one counter, starting at id_base)
  6. output, walking the tracks backwards: the POSTERIOR box of every track updated in this frame with hit_streak >= min_hits (or
     frame_count <= min_hits); tracks with time_since_update > max_age are dropped
Counters (`stats`): frames that took the assignment path, births after frame min_hits, deaths, NaN removals, vs clamps of predict.
"""
import numpy as np

from oracle import ocsort_np as oc

COLUMNS = ("id", "time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width")


def convert_bbox_to_z(bbox):
    w = bbox[2] - bbox[0]
    h = bbox[3] - bbox[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.float64(w) / np.float64(h)                 # w / float(h): no 1e-6; h == 0 gives inf (or NaN), as numpy scalars do
    return np.array([bbox[0] + w / 2.0, bbox[1] + h / 2.0, w * h, r]).reshape((4, 1))


def convert_x_to_bbox(x):
    with np.errstate(invalid="ignore"):
        return oc.convert_x_to_bbox(x)


class _Filter(oc.KalmanFilter7):
    """the constants and predict() of the oracle's filter; update() is the plain filterpy update (no freeze / unfreeze)"""

    def update(self, z):
        y = z - np.dot(self.H, self.x)
        PHT = np.dot(self.P, self.H.T)
        S = np.dot(self.H, PHT) + self.R
        K = np.dot(PHT, np.linalg.inv(S))
        self.x = self.x + np.dot(K, y)
        I_KH = self._I - np.dot(K, self.H)
        self.P = np.dot(np.dot(I_KH, self.P), I_KH.T) + np.dot(np.dot(K, self.R), K.T)


class KalmanBoxTracker:
    def __init__(self, det, tid):
        self.kf = _Filter()
        self.kf.x[:4] = convert_bbox_to_z(det)
        self.id = tid
        self.time_since_update = self.hits = self.hit_streak = self.age = 0
        self.conf, self.cls = det[4], det[5]

    def predict(self):
        self.clamped = bool((self.kf.x[6] + self.kf.x[2]) <= 0)
        if self.clamped:
            self.kf.x[6] *= 0.0
        with np.errstate(invalid="ignore"):
            self.kf.predict()
        self.age += 1
        if self.time_since_update > 0:
            self.hit_streak = 0
        self.time_since_update += 1
        return convert_x_to_bbox(self.kf.x)

    def update(self, det):
        self.time_since_update = 0
        self.hits += 1
        self.hit_streak += 1
        with np.errstate(invalid="ignore"):
            self.kf.update(convert_bbox_to_z(det))
        self.conf, self.cls = det[4], det[5]

    def get_state(self):
        return convert_x_to_bbox(self.kf.x)


class SortTracker:
    def __init__(self, max_age=1, min_hits=3, iou_threshold=0.3, id_base=0):
        self.max_age, self.min_hits, self.iou_threshold = max_age, min_hits, iou_threshold
        self.trackers = []
        self.frame_count = 0
        self._count = id_base
        self.stats = {"assignment_frames": 0, "late_births": 0, "deaths": 0, "nan_removals": 0, "vs_clamps": 0}

    def _associate(self, dets, trks):
        if len(trks) == 0 or len(dets) == 0:
            return [], list(range(len(dets)))
        iou = oc.iou_batch(dets, trks)                                      # [det, trk]
        a = (iou > self.iou_threshold).astype(np.int32)
        if a.sum(1).max() == 1 and a.sum(0).max() == 1:
            pairs = np.stack(np.where(a), axis=1)
        else:
            self.stats["assignment_frames"] += 1
            pairs = oc.linear_assignment(-iou)
        um_d = [d for d in range(len(dets)) if d not in pairs[:, 0]]
        matches = []
        for d, t in pairs:
            if iou[d, t] < self.iou_threshold:
                um_d.append(int(d))
            else:
                matches.append((int(d), int(t)))
        return matches, um_d

    def update(self, dets, _=None):
        self.frame_count += 1
        dets = np.asarray(dets, dtype=np.float64).reshape(-1, 6)
        boxes, gone = [], []
        for t, trk in enumerate(self.trackers):
            pos = trk.predict()[0]
            self.stats["vs_clamps"] += trk.clamped
            if np.any(np.isnan(pos)):
                gone.append(t)
            else:
                boxes.append(pos)
        for t in reversed(gone):
            self.trackers.pop(t)
        self.stats["nan_removals"] += len(gone)
        matches, um_d = self._associate(dets, np.asarray(boxes, np.float64).reshape(-1, 4))
        for d, t in matches:
            self.trackers[t].update(dets[d])
        for d in um_d:
            self.trackers.append(KalmanBoxTracker(dets[d], self._count))
            self._count += 1
            self.stats["late_births"] += self.frame_count > self.min_hits
        ret = []
        i = len(self.trackers)
        for trk in reversed(self.trackers):
            if trk.time_since_update < 1 and (trk.hit_streak >= self.min_hits or self.frame_count <= self.min_hits):
                ret.append(np.concatenate((trk.get_state()[0], [trk.id + 1], [trk.cls], [trk.conf])).reshape(1, -1))
            i -= 1
            if trk.time_since_update > self.max_age:
                self.trackers.pop(i)
                self.stats["deaths"] += 1
        return np.concatenate(ret) if ret else np.empty((0, 7))


def track_boxes(frames_dets, times, **kw):
    """Replay of reference track.py:159-234 with the SORT tracker of track.py:156 on precomputed detections (frames without any are
    skipped, track.py:180-181).  Returns (the 8-column dict of track.py:144-145, the tracker's counters)."""
    kw.setdefault("max_age", 30)
    trk = SortTracker(**kw)
    data = {k: [] for k in COLUMNS}
    for dets, t in zip(frames_dets, times):
        if len(dets) == 0:
            continue
        out = trk.update(dets)
        kfx = {k.id: k.kf.x.flatten() for k in trk.trackers}
        for xmin, ymin, xmax, ymax, tid, _, _ in out:
            tid = int(tid)
            dx, dy = kfx[tid - 1][4:6]
            for k, v in zip(COLUMNS, (tid, t, (xmin + xmax) / 2, (ymin + ymax) / 2, dx, dy, abs(ymax - ymin), abs(xmax - xmin))):
                data[k].append(v)
    return data, dict(trk.stats)
