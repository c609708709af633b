// Detector evaluation on the device for gfx950 (MI355X): ground-truth matching and PR / ROC curves.
//
// Replaces (reference eval.py):
//   scaled_bbox + calculate_iou + match_bboxes over every image of a batch          eval.py:57-71,74-93,96-153,182-205
//   Label = IoU > iou_threshold                                                     eval.py:515
//   sklearn.metrics.precision_recall_curve / average_precision_score                eval.py:232,245
//   sklearn.metrics.roc_curve (drop_intermediate=True) / roc_auc_score              eval.py:360,370
// Execution model.  Matching: ONE WAVEFRONT PER IMAGE - lane j owns detection column j of the padded square cost matrix, the
// assignment is the tracker's lane-parallel shortest-augmenting-path solver (lap.h: scipy's tie rule, which decides the order of the
// dummy rows and with it the row order of the table).  A second, single-wavefront kernel appends the batch's rows to the device table
// in image order, so the table's row order is the reference's whatever order the wavefronts finished in.
// Curves: ONE WORKGROUP per call walks the whole table: a stable LSD radix sort (4-bit digits, every thread owns a contiguous chunk)
// of (descending score, label), then chunked scans for the cumulative counts at each distinct score, the drop_intermediate
// compaction and the two sums.  All counts are integers and every rate is one IEEE double division of two exactly representable
// integers, so the curve points equal scikit-learn's bit for bit; AP / AUC differ from numpy's by the summation order only.
#include "common.h"
#include "dev_mem.h"
#include "hip_handles.h"
#include "lap.h"

#include <algorithm>

namespace vbt {

constexpr int EV_MAXD = VBT_MAX_DETECTIONS;
constexpr int EV_THREADS = 512;   // curve kernel workgroup
constexpr int EV_STAGES = 4;      // pinned staging slots of vbt_eval_add_detections (uploads in flight)

// device-resident table state
struct EvalState {
  int n_rows;      // rows appended so far (counts rows that did not fit, too: the size a reader needs)
  int overflow;    // rows were dropped: the table is not usable
  int n_images;    // images added so far
  int pad;
};

struct EvalTable {
  float* score;
  double* iou;
  int* image;
  int* det;
  int* gt;
  int cap;
};

// per-batch scratch of the match kernel: [B][25] rows + [B] counts
struct EvalBatch {
  float* score;
  double* iou;
  int* det;
  int* gt;
  int* cnt;
};

struct MatchShared {
  double cost[MAXT][MAXT];
  long long dbox[EV_MAXD][4];
  int r2c[MAXT];
  LapShared lap;
};

// calculate_iou (eval.py:74-93) on integer boxes ymin,xmin,ymax,xmax: int64 arithmetic as numpy's, one double division
__device__ inline double iou_int(const long long* d, const int* g) {
  const long long g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
  const long long iy0 = d[0] > g0 ? d[0] : g0, ix0 = d[1] > g1 ? d[1] : g1;
  const long long iy1 = d[2] < g2 ? d[2] : g2, ix1 = d[3] < g3 ? d[3] : g3;
  const long long ih = iy1 - iy0 > 0 ? iy1 - iy0 : 0, iw = ix1 - ix0 > 0 ? ix1 - ix0 : 0;
  const long long inter = ih * iw;
  const long long uni = (d[2] - d[0]) * (d[3] - d[1]) + (g2 - g0) * (g3 - g1) - inter;
  return uni > 0 ? (double)inter / (double)uni : 0.0;
}

// meta [B][4] = height, width, first ground-truth box, number of ground-truth boxes; gt [*][4] = ymin,xmin,ymax,xmax
__global__ __launch_bounds__(64) void eval_match_kernel(const float* boxes, const float* scores, const int* counts, const int* meta,
                                                        const int* gt, EvalBatch out) {
  __shared__ MatchShared sh;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int height = meta[b * 4 + 0], width = meta[b * 4 + 1], g0 = meta[b * 4 + 2], n_gt = meta[b * 4 + 3];
  int n_pred = counts[b];
  n_pred = n_pred < 0 ? 0 : (n_pred > EV_MAXD ? EV_MAXD : n_pred);
  const int n = n_gt > n_pred ? n_gt : n_pred;
  if (n == 0 || n_pred == 0) {      // no detection: every assignment goes to a dummy column and is dropped (eval.py:146-149)
    if (lane == 0) out.cnt[b] = 0;
    return;
  }
  // scaled_bbox (eval.py:57-71): float32 corner -> double, times height / 1.0 resp. width / 1.0, truncated towards zero
  if (lane < n_pred) {
    const float* bx = boxes + ((size_t)b * EV_MAXD + lane) * 4;
    const double hf = (double)height / 1.0, wf = (double)width / 1.0;
    sh.dbox[lane][0] = (long long)((double)bx[0] * hf);
    sh.dbox[lane][1] = (long long)((double)bx[1] * wf);
    sh.dbox[lane][2] = (long long)((double)bx[2] * hf);
    sh.dbox[lane][3] = (long long)((double)bx[3] * wf);
  }
  __syncthreads();
  // 1 - iou_matrix, padded to n x n with IoU 0 (eval.py:122-143): lane = column
  for (int i = 0; i < n; i++) {
    if (lane < n) {
      double v = 0.0;
      if (i < n_gt && lane < n_pred) v = iou_int(sh.dbox[lane], gt + (size_t)(g0 + i) * 4);
      sh.cost[i][lane] = 1.0 - v;
    }
  }
  __syncthreads();
  lap_solve(&sh.cost[0][0], MAXT, false, n, n, sh.r2c, sh.lap, lane);
  // rows in idx_gt order, dummy columns dropped (eval.py:146-149)
  const int col = lane < n ? sh.r2c[lane] : n_pred;
  const bool keep = lane < n && col < n_pred;
  const unsigned long long m = __ballot(keep);
  if (keep) {
    const int k = __popcll(m & ((1ull << lane) - 1ull));
    const size_t o = (size_t)b * EV_MAXD + k;
    out.score[o] = scores[(size_t)b * EV_MAXD + col];
    out.iou[o] = lane < n_gt ? iou_int(sh.dbox[col], gt + (size_t)(g0 + lane) * 4) : 0.0;   // iou_matrix[idx_gt, idx_pred]; dummy rows hold 0
    out.det[o] = col;
    out.gt[o] = lane;
  }
  if (lane == 0) out.cnt[b] = __popcll(m);
}

// the batch's rows behind the table's, in image order; one wavefront
__global__ __launch_bounds__(64) void eval_append_kernel(EvalBatch in, int B, EvalTable t, EvalState* st) {
  __shared__ int base_of[64];
  const int lane = threadIdx.x;
  int base = st->n_rows;
  const int image0 = st->n_images;
  int lost = 0;
  __syncthreads();
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int b = b0 + lane;
    const int c = b < B ? in.cnt[b] : 0;
    int incl = c;   // inclusive wave scan
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    base_of[lane] = base + incl - c;
    __syncthreads();
    const int nb = B - b0 < 64 ? B - b0 : 64;
    for (int i = 0; i < nb; i++) {
      const int ci = in.cnt[b0 + i], dst = base_of[i] + lane;
      if (lane < ci) {
        if (dst < t.cap) {
          const size_t s = (size_t)(b0 + i) * EV_MAXD + lane;
          t.score[dst] = in.score[s];
          t.iou[dst] = in.iou[s];
          t.image[dst] = image0 + b0 + i;
          t.det[dst] = in.det[s];
          t.gt[dst] = in.gt[s];
        } else {
          lost = 1;
        }
      }
    }
    base += __shfl(incl, 63);
    __syncthreads();
  }
  const int any_lost = __ballot(lost) != 0ull;
  if (lane == 0) {
    st->n_rows = base;
    st->n_images = image0 + B;
    if (any_lost) st->overflow = 1;
  }
}

// ------------------------------------------------------------------------------------------
// curves
// ------------------------------------------------------------------------------------------
struct CurveHead {
  int n_rows, n_pos, n_neg, n_pr, n_roc, flags;
  double ap, auc;
};

struct CurveWork {
  unsigned long long *e0, *e1;   // [n] sort buffers: (key << 1) | label, ascending key = descending score
  int *tps, *fps;                // [n] cumulative counts at each distinct score
  unsigned char* keep;           // [n] drop_intermediate
  double *prec, *rec;            // [n + 1]
  float* pthr;                   // [n]
  double *fpr, *tpr;             // [n + 1]
  float* rthr;                   // [n + 1]
  CurveHead* head;
};

// ascending key <=> descending score; -0.0 and +0.0 are one score, as numpy compares them
__device__ inline unsigned score_key(float s) {
  if (s == 0.0f) s = 0.0f;
  const unsigned u = __float_as_uint(s);
  const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}
__device__ inline float key_score(unsigned k) {
  const unsigned asc = ~k;
  const unsigned u = (asc & 0x80000000u) ? (asc & 0x7fffffffu) : ~asc;
  return __uint_as_float(u);
}

// exclusive scan of one int per thread over the workgroup; returns the total.  tmp: EV_THREADS + 1 ints of LDS.
__device__ inline int block_excl_scan(int v, int* tmp, int* total) {
  const int t = threadIdx.x;
  tmp[t] = v;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int i = 0; i < EV_THREADS; i++) { const int x = tmp[i]; tmp[i] = run; run += x; }
    tmp[EV_THREADS] = run;
  }
  __syncthreads();
  const int r = tmp[t];
  *total = tmp[EV_THREADS];
  __syncthreads();
  return r;
}

__device__ inline double block_sum_f64(double v, double* tmp) {
  const int t = threadIdx.x;
  tmp[t] = v;
  __syncthreads();
  if (t == 0) {
    double run = 0.0;
    for (int i = 0; i < EV_THREADS; i++) run += tmp[i];
    tmp[0] = run;
  }
  __syncthreads();
  const double r = tmp[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(EV_THREADS) void eval_curve_kernel(const float* scores, const double* ious, const int* n_dev, int n_arg,
                                                               double thr, CurveWork w) {
  __shared__ int digit_cnt[16 * EV_THREADS];
  __shared__ int itmp[EV_THREADS + 1];
  __shared__ double dtmp[EV_THREADS];
  const int t = threadIdx.x;
  const int n = n_dev ? *n_dev : n_arg;
  const int chunk = (n + EV_THREADS - 1) / EV_THREADS;
  const int lo = min(n, t * chunk), hi = min(n, lo + chunk);
  const double NaN = __builtin_nan("");

  // ---- Label = IoU > iou_threshold (eval.py:515), packed behind the score key ----
  for (int i = lo; i < hi; i++) w.e0[i] = ((unsigned long long)score_key(scores[i]) << 1) | (ious[i] > thr ? 1ull : 0ull);
  __syncthreads();

  // ---- stable LSD radix sort on the 32 key bits, 4 bits a pass; thread t owns elements [lo, hi) of the pass's input ----
  unsigned long long *src = w.e0, *dst = w.e1;
  for (int pass = 0; pass < 8; pass++) {
    const int shift = 1 + 4 * pass;
    for (int d = 0; d < 16; d++) digit_cnt[d * EV_THREADS + t] = 0;
    for (int i = lo; i < hi; i++) digit_cnt[(int)((src[i] >> shift) & 15ull) * EV_THREADS + t] += 1;
    __syncthreads();
    // exclusive scan of digit_cnt in (digit, thread) order: thread t owns entries [16 t, 16 t + 16)
    int s = 0;
    for (int j = 0; j < 16; j++) s += digit_cnt[16 * t + j];
    int total;
    int run = block_excl_scan(s, itmp, &total);
    for (int j = 0; j < 16; j++) { const int x = digit_cnt[16 * t + j]; digit_cnt[16 * t + j] = run; run += x; }
    __syncthreads();
    for (int i = lo; i < hi; i++) {
      const unsigned long long e = src[i];
      const int slot = (int)((e >> shift) & 15ull) * EV_THREADS + t;
      dst[digit_cnt[slot]++] = e;
    }
    __syncthreads();
    unsigned long long* x = src; src = dst; dst = x;
  }
  // 8 passes: the sorted table is back in e0 (= src)

  // ---- cumulative tps / fps at the last row of each distinct score (_binary_clf_curve) ----
  int c_pos = 0, c_grp = 0;
  for (int i = lo; i < hi; i++) {
    const unsigned long long e = src[i];
    c_pos += (int)(e & 1ull);
    c_grp += (i == n - 1 || (src[i + 1] >> 1) != (e >> 1)) ? 1 : 0;
  }
  int n_pos, D;
  int pos = block_excl_scan(c_pos, itmp, &n_pos);
  int grp = block_excl_scan(c_grp, itmp, &D);
  for (int i = lo; i < hi; i++) {
    const unsigned long long e = src[i];
    pos += (int)(e & 1ull);
    if (i == n - 1 || (src[i + 1] >> 1) != (e >> 1)) {
      w.tps[grp] = pos;
      w.fps[grp] = 1 + i - pos;
      w.pthr[D - 1 - grp] = key_score((unsigned)(e >> 1));
      grp++;
    }
  }
  const int n_neg = n - n_pos;
  __syncthreads();

  // ---- precision / recall (reversed, with the final (1, 0) point), AP, and the drop_intermediate marks ----
  const int gchunk = (D + EV_THREADS - 1) / EV_THREADS;
  const int glo = min(D, t * gchunk), ghi = min(D, glo + gchunk);
  double ap_part = 0.0;
  int c_keep = 0;
  for (int k = glo; k < ghi; k++) {
    const int tp = w.tps[k], fp = w.fps[k];
    const double p = (double)tp / (double)(tp + fp);
    const double r = n_pos > 0 ? (double)tp / (double)n_pos : NaN;
    w.prec[D - 1 - k] = p;
    w.rec[D - 1 - k] = r;
    // -sum(diff(recall) * precision[:-1]) over the reversed arrays: the point after k (reversed) is k - 1, or the final (1, 0)
    const double r_next = k > 0 ? (n_pos > 0 ? (double)w.tps[k - 1] / (double)n_pos : NaN) : 0.0;
    ap_part += (r_next - r) * p;
    bool kp = k == 0 || k == D - 1;
    if (!kp) {
      const long long d2f = (long long)w.fps[k + 1] - 2ll * fp + (long long)w.fps[k - 1];
      const long long d2t = (long long)w.tps[k + 1] - 2ll * tp + (long long)w.tps[k - 1];
      kp = d2f != 0 || d2t != 0;
    }
    w.keep[k] = kp ? 1 : 0;
    c_keep += kp ? 1 : 0;
  }
  if (t == 0) { w.prec[D] = 1.0; w.rec[D] = 0.0; }
  const double ap_sum = block_sum_f64(ap_part, dtmp);
  int R;
  int kpos = block_excl_scan(c_keep, itmp, &R);

  // ---- ROC: the leading (0, 0) point with threshold +inf, then the kept points ----
  if (t == 0) {
    w.fpr[0] = n_neg > 0 ? 0.0 / (double)n_neg : NaN;
    w.tpr[0] = n_pos > 0 ? 0.0 / (double)n_pos : NaN;
    w.rthr[0] = __builtin_inff();
  }
  for (int k = glo; k < ghi; k++) {
    if (!w.keep[k]) continue;
    kpos++;
    w.fpr[kpos] = n_neg > 0 ? (double)w.fps[k] / (double)n_neg : NaN;
    w.tpr[kpos] = n_pos > 0 ? (double)w.tps[k] / (double)n_pos : NaN;
    w.rthr[kpos] = w.pthr[D - 1 - k];
  }
  __syncthreads();
  // ---- AUC, trapezoid rule: sum(diff(fpr) * (tpr[1:] + tpr[:-1]) / 2) ----
  const int rchunk = (R + EV_THREADS - 1) / EV_THREADS;   // R intervals between R + 1 points
  const int rlo = min(R, t * rchunk), rhi = min(R, rlo + rchunk);
  double auc_part = 0.0;
  for (int r = rlo; r < rhi; r++) auc_part += (w.fpr[r + 1] - w.fpr[r]) * (w.tpr[r + 1] + w.tpr[r]) / 2.0;
  const double auc_sum = block_sum_f64(auc_part, dtmp);
  if (t == 0) {
    CurveHead h;
    h.n_rows = n; h.n_pos = n_pos; h.n_neg = n_neg; h.n_pr = D + 1; h.n_roc = R + 1;
    h.flags = (n_pos == 0 ? VBT_EVAL_NO_POSITIVES : 0) | (n_neg == 0 ? VBT_EVAL_NO_NEGATIVES : 0);
    h.ap = n_pos > 0 ? (-ap_sum > 0.0 ? -ap_sum : 0.0) : NaN;   // max(0.0, ...): scikit-learn clips a -0.0
    h.auc = (n_pos > 0 && n_neg > 0) ? auc_sum : NaN;
    *w.head = h;
  }
}

}  // namespace vbt

using namespace vbt;

// owner of the twelve arrays of a CurveWork; view is what the kernel takes
struct CurveBufs {
  DevBuf<unsigned long long> e0, e1;
  DevBuf<int> tps, fps;
  DevBuf<unsigned char> keep;
  DevBuf<double> prec, rec, fpr, tpr;
  DevBuf<float> pthr, rthr;
  DevBuf<CurveHead> head;
  CurveWork view{};
};

struct vbt_eval {
  int device = 0, max_batch = 0, rows_cap = 0;
  // owners of the table's and the per-call scratch's arrays; tab and batch are what the kernels take
  DevBuf<float> tab_score, batch_score;
  DevBuf<double> tab_iou, batch_iou;
  DevBuf<int> tab_image, tab_det, tab_gt, batch_det, batch_gt, batch_cnt;
  EvalTable tab{};
  EvalBatch batch{};
  DevBuf<EvalState> state;
  // staging of (meta, ground truth) uploads: EV_STAGES pinned slots + their device twins, an event each
  struct Stage {
    PinnedBuf<int> host;
    DevBuf<int> dev;
    Event ev;
    bool used = false;
  } stage[EV_STAGES];
  size_t stage_ints = 0;
  int next_stage = 0;
  hipStream_t last_stream = nullptr;
  Event done;                       // end of the last call's kernels: a call on another stream waits for it (shared scratch and staging)
  bool done_used = false;
  int images_host = 0;
  CurveBufs work;
  int work_cap = -1;
};

namespace {

int work_alloc(CurveBufs& w, int n) {
  const size_t m = (size_t)std::max(n, 1);
  hipError_t e = hipSuccess;
  auto get = [&](auto& buf, size_t count) { if (e == hipSuccess) e = buf.alloc(count); };
  get(w.e0, m); get(w.e1, m); get(w.tps, m); get(w.fps, m); get(w.keep, m);
  get(w.prec, m + 1); get(w.rec, m + 1); get(w.pthr, m);
  get(w.fpr, m + 1); get(w.tpr, m + 1); get(w.rthr, m + 1); get(w.head, 1);
  if (e != hipSuccess) {
    set_error("hipMalloc failed for the curve workspace of %d rows: %s", n, hipGetErrorString(e));
    w = CurveBufs{};
    return VBT_ERR_HIP;
  }
  w.view = CurveWork{w.e0.get(), w.e1.get(), w.tps.get(), w.fps.get(), w.keep.get(), w.prec.get(), w.rec.get(), w.pthr.get(),
                     w.fpr.get(), w.tpr.get(), w.rthr.get(), w.head.get()};
  return VBT_OK;
}

// curve kernel on device arrays + the read-back; n_dev (device row count) or n
int curves_run(CurveWork& w, const float* d_scores, const double* d_ious, const int* n_dev, int n, double thr, hipStream_t st,
               vbt_eval_summary* s, double* precision, double* recall, float* pr_thresholds, int pr_cap, double* fpr, double* tpr,
               float* roc_thresholds, int roc_cap) {
  eval_curve_kernel<<<1, EV_THREADS, 0, st>>>(d_scores, d_ious, n_dev, n, thr, w);
  VBT_HIP_CHECK(hipGetLastError());
  CurveHead h;
  VBT_HIP_CHECK(hipMemcpyAsync(&h, w.head, sizeof(h), hipMemcpyDeviceToHost, st));
  VBT_HIP_CHECK(hipStreamSynchronize(st));
  s->n_rows = h.n_rows; s->n_pos = h.n_pos; s->n_neg = h.n_neg; s->n_pr = h.n_pr; s->n_roc = h.n_roc; s->flags = h.flags;
  s->ap = h.ap; s->auc = h.auc;
  if (h.n_pr > pr_cap || h.n_roc > roc_cap) {
    set_error("%d PR points / %d ROC points, buffers hold %d / %d", h.n_pr, h.n_roc, pr_cap, roc_cap);
    return VBT_ERR_CAPACITY;
  }
  if (precision) VBT_HIP_CHECK(hipMemcpyAsync(precision, w.prec, 8 * (size_t)h.n_pr, hipMemcpyDeviceToHost, st));
  if (recall) VBT_HIP_CHECK(hipMemcpyAsync(recall, w.rec, 8 * (size_t)h.n_pr, hipMemcpyDeviceToHost, st));
  if (pr_thresholds && h.n_pr > 1) VBT_HIP_CHECK(hipMemcpyAsync(pr_thresholds, w.pthr, 4 * (size_t)(h.n_pr - 1), hipMemcpyDeviceToHost, st));
  if (fpr) VBT_HIP_CHECK(hipMemcpyAsync(fpr, w.fpr, 8 * (size_t)h.n_roc, hipMemcpyDeviceToHost, st));
  if (tpr) VBT_HIP_CHECK(hipMemcpyAsync(tpr, w.tpr, 8 * (size_t)h.n_roc, hipMemcpyDeviceToHost, st));
  if (roc_thresholds) VBT_HIP_CHECK(hipMemcpyAsync(roc_thresholds, w.rthr, 4 * (size_t)h.n_roc, hipMemcpyDeviceToHost, st));
  VBT_HIP_CHECK(hipStreamSynchronize(st));
  return VBT_OK;
}

// the device row count after everything enqueued so far (synchronises the handle's stream)
int read_state(vbt_eval* e, EvalState* out) {
  VBT_HIP_CHECK(hipMemcpyAsync(out, e->state.get(), sizeof(EvalState), hipMemcpyDeviceToHost, e->last_stream));
  VBT_HIP_CHECK(hipStreamSynchronize(e->last_stream));
  if (out->overflow) {
    set_error("vbt_eval: the table holds %d rows, %d were produced", e->rows_cap, out->n_rows);
    return VBT_ERR_CAPACITY;
  }
  return VBT_OK;
}

}  // namespace

extern "C" {

int vbt_eval_create(int device, int max_batch, int rows_cap, vbt_eval** out) {
  if (!out || max_batch < 1 || max_batch > 4096 || rows_cap < 1) { set_error("vbt_eval_create: bad argument"); return VBT_ERR_ARG; }
  *out = nullptr;
  if (int rc = use_device("vbt_eval_create", device)) return rc;
  std::unique_ptr<vbt_eval> e(new vbt_eval());
  e->device = device; e->max_batch = max_batch; e->rows_cap = rows_cap;
  e->stage_ints = (size_t)max_batch * 4 + (size_t)max_batch * VBT_EVAL_MAX_GT * 4;
  hipError_t err = hipSuccess;
  auto get = [&](auto& buf, size_t count) { if (err == hipSuccess) err = buf.alloc(count); };
  const size_t r = (size_t)rows_cap, s = (size_t)max_batch * EV_MAXD;
  get(e->tab_score, r); get(e->tab_iou, r); get(e->tab_image, r); get(e->tab_det, r); get(e->tab_gt, r);
  get(e->batch_score, s); get(e->batch_iou, s); get(e->batch_det, s); get(e->batch_gt, s); get(e->batch_cnt, (size_t)max_batch);
  get(e->state, 1);
  for (vbt_eval::Stage& st : e->stage) {
    get(st.dev, e->stage_ints);
    get(st.host, e->stage_ints);
    if (err == hipSuccess) err = st.ev.create(hipEventDisableTiming);
  }
  if (err == hipSuccess) err = e->done.create(hipEventDisableTiming);
  if (err == hipSuccess) err = hipMemset(e->state.get(), 0, sizeof(EvalState));
  if (err != hipSuccess) {
    set_error("vbt_eval_create: allocation failed: %s", hipGetErrorString(err));
    return VBT_ERR_HIP;
  }
  e->tab = EvalTable{e->tab_score.get(), e->tab_iou.get(), e->tab_image.get(), e->tab_det.get(), e->tab_gt.get(), rows_cap};
  e->batch = EvalBatch{e->batch_score.get(), e->batch_iou.get(), e->batch_det.get(), e->batch_gt.get(), e->batch_cnt.get()};
  if (int rc = work_alloc(e->work, rows_cap)) return rc;
  e->work_cap = rows_cap;
  *out = e.release();
  return VBT_OK;
}

void vbt_eval_destroy(vbt_eval* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  (void)hipDeviceSynchronize();
  delete e;
}

int vbt_eval_reset(vbt_eval* e) {
  if (!e) { set_error("NULL vbt_eval"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(e->device));
  VBT_HIP_CHECK(hipDeviceSynchronize());
  VBT_HIP_CHECK(hipMemset(e->state.get(), 0, sizeof(EvalState)));
  e->images_host = 0;
  return VBT_OK;
}

int vbt_eval_add_detections(vbt_eval* e, const float* boxes_dev, const float* scores_dev, const int32_t* counts_dev, int B,
                            const int32_t* hw_host, const int32_t* gt_offsets_host, const int32_t* gt_boxes_host, void* stream) {
  if (!e || !boxes_dev || !scores_dev || !counts_dev || !hw_host || !gt_offsets_host || B < 1) {
    set_error("vbt_eval_add_detections: bad argument");
    return VBT_ERR_ARG;
  }
  if (B > e->max_batch) { set_error("vbt_eval_add_detections: %d images, the handle takes %d per call", B, e->max_batch); return VBT_ERR_CAPACITY; }
  const int g_first = gt_offsets_host[0];
  for (int b = 0; b < B; b++) {
    const int n_gt = gt_offsets_host[b + 1] - gt_offsets_host[b];
    if (n_gt < 0 || hw_host[2 * b] < 1 || hw_host[2 * b + 1] < 1) {
      set_error("vbt_eval_add_detections: image %d of the call: decreasing ground-truth offsets or an empty image size", b);
      return VBT_ERR_ARG;
    }
    if (n_gt > VBT_EVAL_MAX_GT) {
      set_error("vbt_eval_add_detections: image %d (number %d of the call) has %d ground-truth boxes, the matcher takes %d", e->images_host + b, b,
                n_gt, VBT_EVAL_MAX_GT);
      return VBT_ERR_CAPACITY;
    }
  }
  const int total = gt_offsets_host[B] - g_first;
  if (total > 0 && !gt_boxes_host) { set_error("vbt_eval_add_detections: NULL ground-truth boxes"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  // the per-batch scratch, the staging slots and the table are shared by all calls: a call on another stream runs after the last one
  if (e->done_used && st != e->last_stream) VBT_HIP_CHECK(hipStreamWaitEvent(st, e->done.get(), 0));
  vbt_eval::Stage& sg = e->stage[e->next_stage];
  if (sg.used) VBT_HIP_CHECK(hipEventSynchronize(sg.ev.get()));   // the caller is EV_STAGES uploads ahead of the device
  int* h = sg.host.get();
  for (int b = 0; b < B; b++) {
    h[4 * b + 0] = hw_host[2 * b];
    h[4 * b + 1] = hw_host[2 * b + 1];
    h[4 * b + 2] = gt_offsets_host[b] - g_first;
    h[4 * b + 3] = gt_offsets_host[b + 1] - gt_offsets_host[b];
  }
  if (total > 0) memcpy(h + 4 * (size_t)B, gt_boxes_host + 4 * (size_t)g_first, sizeof(int) * 4 * (size_t)total);
  VBT_HIP_CHECK(hipMemcpyAsync(sg.dev.get(), h, sizeof(int) * 4 * ((size_t)B + total), hipMemcpyHostToDevice, st));
  VBT_HIP_CHECK(hipEventRecord(sg.ev.get(), st));
  sg.used = true;
  e->next_stage = (e->next_stage + 1) % EV_STAGES;
  eval_match_kernel<<<B, 64, 0, st>>>(boxes_dev, scores_dev, counts_dev, sg.dev.get(), sg.dev.get() + 4 * (size_t)B, e->batch);
  VBT_HIP_CHECK(hipGetLastError());
  eval_append_kernel<<<1, 64, 0, st>>>(e->batch, B, e->tab, e->state.get());
  VBT_HIP_CHECK(hipGetLastError());
  VBT_HIP_CHECK(hipEventRecord(e->done.get(), st));
  e->done_used = true;
  e->last_stream = st;
  e->images_host += B;
  return VBT_OK;
}

int vbt_eval_table(vbt_eval* e, int* n_rows, float* scores, double* ious, int32_t* image, int32_t* det_idx, int32_t* gt_idx, int cap) {
  if (!e || !n_rows) { set_error("vbt_eval_table: bad argument"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(e->device));
  EvalState s;
  const int rc = read_state(e, &s);
  *n_rows = s.n_rows;
  if (rc) return rc;
  if (!scores && !ious && !image && !det_idx && !gt_idx) return VBT_OK;
  if (s.n_rows > cap) { set_error("vbt_eval_table: %d rows, buffers hold %d", s.n_rows, cap); return VBT_ERR_CAPACITY; }
  const size_t n = (size_t)s.n_rows;
  if (n == 0) return VBT_OK;
  if (scores) VBT_HIP_CHECK(hipMemcpy(scores, e->tab.score, 4 * n, hipMemcpyDeviceToHost));
  if (ious) VBT_HIP_CHECK(hipMemcpy(ious, e->tab.iou, 8 * n, hipMemcpyDeviceToHost));
  if (image) VBT_HIP_CHECK(hipMemcpy(image, e->tab.image, 4 * n, hipMemcpyDeviceToHost));
  if (det_idx) VBT_HIP_CHECK(hipMemcpy(det_idx, e->tab.det, 4 * n, hipMemcpyDeviceToHost));
  if (gt_idx) VBT_HIP_CHECK(hipMemcpy(gt_idx, e->tab.gt, 4 * n, hipMemcpyDeviceToHost));
  return VBT_OK;
}

int vbt_eval_curves(vbt_eval* e, double iou_threshold, vbt_eval_summary* s, double* precision, double* recall, float* pr_thresholds,
                    int pr_cap, double* fpr, double* tpr, float* roc_thresholds, int roc_cap) {
  if (!e || !s) { set_error("vbt_eval_curves: bad argument"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(e->device));
  EvalState es;
  if (int rc = read_state(e, &es)) return rc;
  // the row count is read by the kernel from the device state: the table never leaves the device for this call
  return curves_run(e->work.view, e->tab.score, e->tab.iou, &e->state.get()->n_rows, 0, iou_threshold, e->last_stream, s, precision, recall,
                    pr_thresholds, pr_cap, fpr, tpr, roc_thresholds, roc_cap);
}

int vbt_eval_curves_from_table(const float* scores, const double* ious, int n, double iou_threshold, int device, vbt_eval_summary* s,
                               double* precision, double* recall, float* pr_thresholds, int pr_cap, double* fpr, double* tpr,
                               float* roc_thresholds, int roc_cap) {
  if (!s || n < 0 || (n > 0 && (!scores || !ious))) { set_error("vbt_eval_curves_from_table: bad argument"); return VBT_ERR_ARG; }
  for (int i = 0; i < n; i++)
    if (scores[i] != scores[i]) { set_error("vbt_eval_curves_from_table: score %d is NaN", i); return VBT_ERR_ARG; }
  if (int rc = use_device("vbt_eval_curves_from_table", device)) return rc;
  CurveBufs w;      // with ds and di freed when the function returns: curves_run ends with a synchronisation of its stream
  if (int rc = work_alloc(w, n)) return rc;
  DevBuf<float> ds;
  DevBuf<double> di;
  const size_t m = (size_t)std::max(n, 1);
  if (ds.alloc(m) != hipSuccess || di.alloc(m) != hipSuccess) {
    set_error("vbt_eval_curves_from_table: hipMalloc failed for %d rows", n);
    return VBT_ERR_HIP;
  }
  if (n > 0 && (hipMemcpy(ds.get(), scores, 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(di.get(), ious, 8 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess)) {
    set_error("vbt_eval_curves_from_table: upload failed");
    return VBT_ERR_HIP;
  }
  return curves_run(w.view, ds.get(), di.get(), nullptr, n, iou_threshold, nullptr, s, precision, recall, pr_thresholds, pr_cap, fpr, tpr,
                    roc_thresholds, roc_cap);
}

}  // extern "C"
