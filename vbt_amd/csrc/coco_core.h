// COCO metrics (include/vbt_hip.h, "COCO metrics"): the per-image and per-row statements as host + device functions, so that the
// kernels of evaluate_coco.hip and a host loop (tests/fuzz/coco_check.cc, built with g++ -fsanitize=address,undefined) run the same
// text.  Plain C++: no HIP header is needed to compile it for the host.
//   coco_det_box / coco_gt_box   the box contract: xywh and area in double
//   coco_iou                     maskApi's bbIou on xywh, no crowd
//   coco_outside                 the area-range rule of a box; coco_bound: the IoU bound of a threshold
//   coco_better                  the order of two candidates of one selection: larger IoU, then later in the ground-truth order
//   coco_gt_pos                  a box's place in "non-ignored first, stable"
//   coco_score_key               descending score as an ascending unsigned key, -0.0 and +0.0 one score
//   coco_precision / coco_recall one point of the curves from integer counts
//   coco_tables                  iouThrs and recThrs as np.linspace makes them (host)
//   coco_evaluate_image          COCOeval.evaluateImg of one image for the four ranges, serial (host): what one wavefront does
//   coco_stats                   the twelve numbers of COCOeval.summarize from the precision / recall arrays (host)
// Every loop is bounded by a count known before it starts (25 detections, 64 boxes, 10 thresholds, 4 ranges).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VBT_HD __host__ __device__
#else
#define VBT_HD
#endif

namespace vbt {

constexpr int COCO_T = 10;       // IoU thresholds
constexpr int COCO_R = 101;      // recall thresholds
constexpr int COCO_A = 4;        // area ranges: all, small, medium, large
constexpr int COCO_M = 3;        // maxDets 1, 10, 100
constexpr int COCO_MAXD = 25;    // detections per image
constexpr int COCO_MAXG = 64;    // ground-truth boxes per image

struct CocoBox {
  double x, y, w, h, area;
};

// normalised float32 corners ymin,xmin,ymax,xmax of a detection on a source image of (height, width)
VBT_HD inline CocoBox coco_det_box(const float* b, int height, int width) {
  CocoBox o;
  o.x = (double)b[1] * (double)width;
  o.y = (double)b[0] * (double)height;
  o.w = (double)b[3] * (double)width - o.x;
  o.h = (double)b[2] * (double)height - o.y;
  o.area = o.w * o.h;
  return o;
}

// integer VOC corners ymin,xmin,ymax,xmax of a ground-truth box
VBT_HD inline CocoBox coco_gt_box(const int32_t* g) {
  CocoBox o;
  o.x = (double)g[1];
  o.y = (double)g[0];
  o.w = (double)g[3] - (double)g[1];
  o.h = (double)g[2] - (double)g[0];
  o.area = o.w * o.h;
  return o;
}

VBT_HD inline double coco_iou(const CocoBox& d, const CocoBox& g) {
  const double iw = fmin(d.x + d.w, g.x + g.w) - fmax(d.x, g.x);
  if (iw <= 0) return 0.0;
  const double ih = fmin(d.y + d.h, g.y + g.h) - fmax(d.y, g.y);
  if (ih <= 0) return 0.0;
  const double i = iw * ih;
  return i / (d.w * d.h + g.w * g.h - i);
}

VBT_HD inline double coco_area_lo(int a) { return a == 2 ? 32.0 * 32.0 : (a == 3 ? 96.0 * 96.0 : 0.0); }
VBT_HD inline double coco_area_hi(int a) { return a == 1 ? 32.0 * 32.0 : (a == 2 ? 96.0 * 96.0 : 1e10); }
VBT_HD inline bool coco_outside(double area, int a) { return area < coco_area_lo(a) || area > coco_area_hi(a); }
VBT_HD inline int coco_max_det(int m) { return m == 0 ? 1 : (m == 1 ? 10 : 100); }
VBT_HD inline double coco_bound(double t) { return fmin(t, 1.0 - 1e-10); }
VBT_HD inline unsigned long long coco_bit(int a, int t) { return 1ull << (a * 10 + t); }

// candidate (v, pos) before candidate (bv, bpos): the larger IoU, on equal IoU the later place in the ground-truth order
VBT_HD inline bool coco_better(double v, int pos, double bv, int bpos) { return v > bv || (v == bv && pos > bpos); }

// place of a box in "non-ignored first, stable": before_same = boxes of its own kind in front of it, n_kept = non-ignored boxes in all
VBT_HD inline int coco_gt_pos(bool ignored, int before_same, int n_kept) { return ignored ? n_kept + before_same : before_same; }

VBT_HD inline uint32_t coco_score_key(float s) {
  if (s == 0.0f) s = 0.0f;
  uint32_t u;
  memcpy(&u, &s, 4);
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

VBT_HD inline double coco_recall(int tp, int npig) { return (double)tp / (double)npig; }
// tp / (fp + tp + np.spacing(1)): the integers add exactly, 2^-52 is one double addition
VBT_HD inline double coco_precision(int tp, int fp) { return (double)tp / ((double)(fp + tp) + 2.220446049250313e-16); }

// np.linspace(.5, .95, 10) and np.linspace(0, 1, 101), bit for bit: numpy multiplies the index by the step (stop - start) / (n - 1)
// and sets the last entry to the stop value itself
inline void coco_tables(double* iou_thrs, double* rec_thrs) {
  const double step = (0.95 - 0.5) / 9.0;
  for (int i = 0; i < COCO_T; i++) iou_thrs[i] = 0.5 + (double)i * step;
  iou_thrs[COCO_T - 1] = 0.95;
  for (int i = 0; i < COCO_R; i++) rec_thrs[i] = (double)i * 0.01;
  rec_thrs[COCO_R - 1] = 1.0;
}

// One image, serially.  count is clamped to 0..25, n_gt <= 64.  Outputs by rank (descending score, stable): score, the index of the
// detection in the input, matched / ignored masks (bit a * 10 + t); npig[a] = boxes of the image not ignored in range a.
// Returns the number of detections.
inline int coco_evaluate_image(const float* boxes, const float* scores, int count, int height, int width, const int32_t* gt, int n_gt,
                               const double* iou_thrs, float* out_score, int32_t* out_det, uint64_t* matched, uint64_t* ignored, int32_t* npig) {
  const int nd = count < 0 ? 0 : (count > COCO_MAXD ? COCO_MAXD : count);
  CocoBox d[COCO_MAXD], g[COCO_MAXG];
  double iou[COCO_MAXD][COCO_MAXG];
  for (int i = 0; i < nd; i++) {
    const uint32_t key = coco_score_key(scores[i]);
    int rank = 0;
    for (int j = 0; j < nd; j++) {
      const uint32_t kj = coco_score_key(scores[j]);
      rank += (kj < key || (kj == key && j < i)) ? 1 : 0;
    }
    out_score[rank] = scores[i];
    out_det[rank] = i;
    d[rank] = coco_det_box(boxes + 4 * i, height, width);
  }
  for (int j = 0; j < n_gt; j++) g[j] = coco_gt_box(gt + 4 * j);
  for (int k = 0; k < nd; k++) {
    matched[k] = ignored[k] = 0;
    for (int j = 0; j < n_gt; j++) iou[k][j] = coco_iou(d[k], g[j]);
  }
  for (int a = 0; a < COCO_A; a++) {
    bool ig[COCO_MAXG];
    int pos[COCO_MAXG], n_kept = 0, seen_kept = 0, seen_ig = 0;
    for (int j = 0; j < n_gt; j++) { ig[j] = coco_outside(g[j].area, a); n_kept += ig[j] ? 0 : 1; }
    for (int j = 0; j < n_gt; j++) pos[j] = coco_gt_pos(ig[j], ig[j] ? seen_ig++ : seen_kept++, n_kept);
    npig[a] = n_kept;
    for (int t = 0; t < COCO_T; t++) {
      const double bound = coco_bound(iou_thrs[t]);
      bool taken[COCO_MAXG];
      for (int j = 0; j < n_gt; j++) taken[j] = false;
      for (int k = 0; k < nd; k++) {
        int best = -1;
        for (int pass = 0; pass < 2 && best < 0; pass++) {       // non-ignored boxes; only if none qualifies, the ignored ones
          double bv = -1.0;
          int bp = -1;
          for (int j = 0; j < n_gt; j++) {
            if (taken[j] || ig[j] != (pass == 1) || !(iou[k][j] >= bound)) continue;
            if (coco_better(iou[k][j], pos[j], bv, bp)) { bv = iou[k][j]; bp = pos[j]; best = j; }
          }
        }
        if (best >= 0) {
          taken[best] = true;
          matched[k] |= coco_bit(a, t);
          if (ig[best]) ignored[k] |= coco_bit(a, t);
        } else if (coco_outside(d[k].area, a)) {
          ignored[k] |= coco_bit(a, t);
        }
      }
    }
  }
  return nd;
}

// the mean over entries > -1 of a slice, summed in index order; -1 for none
struct CocoMean {
  double sum = 0.0;
  int n = 0;
  void add(double v) { if (v > -1.0) { sum += v; n++; } }
  double get() const { return n ? sum / (double)n : -1.0; }
};

// precision [T][R][A][M], recall [T][A][M] -> AP, AP50, AP75, APs, APm, APl, ARmax1, ARmax10, ARmax100, ARs, ARm, ARl
inline void coco_stats(const double* precision, const double* recall, double* stats) {
  auto ap = [&](int t0, int t1, int a) {
    CocoMean m;
    for (int t = t0; t < t1; t++)
      for (int r = 0; r < COCO_R; r++) m.add(precision[((t * COCO_R + r) * COCO_A + a) * COCO_M + 2]);
    return m.get();
  };
  auto ar = [&](int a, int md) {
    CocoMean m;
    for (int t = 0; t < COCO_T; t++) m.add(recall[(t * COCO_A + a) * COCO_M + md]);
    return m.get();
  };
  stats[0] = ap(0, COCO_T, 0); stats[1] = ap(0, 1, 0); stats[2] = ap(5, 6, 0);
  stats[3] = ap(0, COCO_T, 1); stats[4] = ap(0, COCO_T, 2); stats[5] = ap(0, COCO_T, 3);
  stats[6] = ar(0, 0); stats[7] = ar(0, 1); stats[8] = ar(0, 2);
  stats[9] = ar(1, 2); stats[10] = ar(2, 2); stats[11] = ar(3, 2);
}

}  // namespace vbt
