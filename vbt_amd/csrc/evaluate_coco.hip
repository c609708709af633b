// COCO detection metrics on the device for gfx950 (MI355X): the numbers model.evaluate prints at the end of the reference's
// training logs (train.py:64,70): COCOeval's evaluateImg / accumulate / summarize, one category, no crowd boxes.
// The per-image and per-row statements are coco_core.h's (host + device); this unit is how they are spread over the machine.
// Matching: ONE WAVEFRONT PER IMAGE - lane g owns ground-truth box g (at most 64), lane k < 25 also owns the detection of rank k.  The
// IoU of a (detection, box) pair depends on neither range nor threshold: it is computed once into LDS, one column per lane.  For each
// of the 4 ranges x 10 thresholds the detections are walked in score order; one selection is one ballot (does any box qualify) and,
// if one does, one butterfly reduction of (IoU, place in the ground-truth order).  A second, single-wavefront kernel appends the
// batch's rows to the table in image order and adds up the non-ignored box counts, so the table does not depend on the order the
// wavefronts finished in and no atomic is needed.
// Accumulate: ONE WORKGROUP sorts the table (the stable LSD radix sort of evaluate.hip's curve kernel, here on (key, row)), then ONE
// WORKGROUP PER (range, maxDets, threshold) - 120 - walks the sorted rows in per-thread chunks: counts, scans, the right-to-left
// precision envelope as a suffix maximum, and the row of each recall threshold found where the recall steps over it.  Counts are
// integers and every entry is coco_precision / coco_recall of two of them, so the arrays equal numpy's bit for bit.
#include "common.h"
#include "coco_core.h"
#include "dev_mem.h"
#include "hip_handles.h"

#include <algorithm>

namespace vbt {

constexpr int CO_THREADS = 512;   // sort and accumulate workgroups
constexpr int CO_STAGES = 4;      // pinned staging slots of vbt_coco_add_detections (uploads in flight)
static_assert(COCO_MAXD == VBT_MAX_DETECTIONS && COCO_MAXG == VBT_EVAL_MAX_GT, "coco_core.h and the header disagree");

struct CocoState {
  int n_rows;      // rows appended so far (counts rows that did not fit, too)
  int overflow;    // rows were dropped: the table is not usable
  int n_images;    // images added so far
  int pad;
  int n_gt[COCO_A];   // non-ignored ground-truth boxes per range
};

struct CocoTable {
  float* score;
  int* image;
  int* rank;
  unsigned long long* matched;
  unsigned long long* ignored;
  int cap;
};

// per-batch scratch of the match kernel: [B][25] rows, [B] counts, [B][4] non-ignored boxes
struct CocoBatch {
  float* score;
  unsigned long long* matched;
  unsigned long long* ignored;
  int* cnt;
  int* npig;
};

struct CocoMatchShared {
  double iou[COCO_MAXD][64];   // [rank][box]: lane g reads and writes column g only
  CocoBox dbox[COCO_MAXD];     // by rank
  float score[COCO_MAXD];      // by rank
};

// meta [B][4] = height, width, first ground-truth box, number of ground-truth boxes; gt [*][4] = ymin,xmin,ymax,xmax
__global__ __launch_bounds__(64) void coco_match_kernel(const float* boxes, const float* scores, const int* counts, const int* meta,
                                                        const int* gt, const double* iou_thrs, CocoBatch out) {
  __shared__ CocoMatchShared sh;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int height = meta[b * 4 + 0], width = meta[b * 4 + 1], g0 = meta[b * 4 + 2];
  int n_gt = meta[b * 4 + 3];
  n_gt = n_gt < 0 ? 0 : (n_gt > COCO_MAXG ? COCO_MAXG : n_gt);
  int n_det = counts[b];
  n_det = n_det < 0 ? 0 : (n_det > COCO_MAXD ? COCO_MAXD : n_det);
  if (n_det == 0 && n_gt == 0) {      // evaluateImg returns None: the image contributes nothing
    if (lane == 0) out.cnt[b] = 0;
    if (lane < COCO_A) out.npig[b * COCO_A + lane] = 0;
    return;
  }
  // detections by descending score, stable: the rank of a detection is the number of detections in front of it
  const float s = lane < n_det ? scores[(size_t)b * COCO_MAXD + lane] : 0.0f;
  const unsigned key = coco_score_key(s);
  int rank = 0;
  for (int j = 0; j < n_det; j++) {
    const unsigned kj = __shfl(key, j);
    rank += (kj < key || (kj == key && j < lane)) ? 1 : 0;
  }
  if (lane < n_det) {
    sh.score[rank] = s;
    sh.dbox[rank] = coco_det_box(boxes + ((size_t)b * COCO_MAXD + lane) * 4, height, width);
  }
  __syncthreads();
  const bool has = lane < n_gt;
  CocoBox g{};
  if (has) g = coco_gt_box(gt + (size_t)(g0 + lane) * 4);
  for (int k = 0; k < n_det; k++) sh.iou[k][lane] = has ? coco_iou(sh.dbox[k], g) : 0.0;
  const double d_area = lane < n_det ? sh.dbox[lane].area : 0.0;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long m_mask = 0ull, i_mask = 0ull;      // of the detection of rank `lane`
  for (int a = 0; a < COCO_A; a++) {
    const bool ig = has && coco_outside(g.area, a);
    const unsigned long long kept_lanes = __ballot(has && !ig), ig_lanes = __ballot(ig);
    const int n_kept = __popcll(kept_lanes);
    const int pos = coco_gt_pos(ig, __popcll((ig ? ig_lanes : kept_lanes) & below), n_kept);
    if (lane == 0) out.npig[b * COCO_A + a] = n_kept;
    const bool d_out = lane < n_det && coco_outside(d_area, a);
    for (int t = 0; t < COCO_T; t++) {
      const double bound = coco_bound(iou_thrs[t]);
      const unsigned long long bit = coco_bit(a, t);
      bool taken = false;
      for (int k = 0; k < n_det; k++) {
        const double v = sh.iou[k][lane];
        const bool cand = has && !taken && v >= bound;
        unsigned long long c = __ballot(cand && !ig);
        const bool from_ignored = c == 0ull;
        if (from_ignored) c = __ballot(cand && ig);      // only if no non-ignored box qualifies
        if (c == 0ull) {
          if (lane == k && d_out) i_mask |= bit;           // unmatched and its own area outside the range
          continue;
        }
        const bool in = (c >> lane) & 1ull;
        double bv = in ? v : -1.0;
        int bp = in ? pos : -1;
        for (int d = 32; d >= 1; d >>= 1) {
          const double ov = __shfl_xor(bv, d);
          const int op = __shfl_xor(bp, d);
          if (coco_better(ov, op, bv, bp)) { bv = ov; bp = op; }
        }
        if (in && pos == bp) taken = true;                 // places are distinct: one lane
        if (lane == k) {
          m_mask |= bit;
          if (from_ignored) i_mask |= bit;
        }
      }
    }
  }
  if (lane < n_det) {
    const size_t o = (size_t)b * COCO_MAXD + lane;
    out.score[o] = sh.score[lane];
    out.matched[o] = m_mask;
    out.ignored[o] = i_mask;
  }
  if (lane == 0) out.cnt[b] = n_det;
}

// the batch's rows behind the table's, in image order, and its box counts onto the state's; one wavefront
__global__ __launch_bounds__(64) void coco_append_kernel(CocoBatch in, int B, CocoTable t, CocoState* st) {
  __shared__ int base_of[64];
  const int lane = threadIdx.x;
  int base = st->n_rows;
  const int image0 = st->n_images;
  int lost = 0;
  int npig[COCO_A] = {0, 0, 0, 0};
  __syncthreads();
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int b = b0 + lane;
    const int c = b < B ? in.cnt[b] : 0;
    if (b < B)
      for (int a = 0; a < COCO_A; a++) npig[a] += in.npig[b * COCO_A + a];
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
          const size_t s = (size_t)(b0 + i) * COCO_MAXD + lane;
          t.score[dst] = in.score[s];
          t.image[dst] = image0 + b0 + i;
          t.rank[dst] = lane;
          t.matched[dst] = in.matched[s];
          t.ignored[dst] = in.ignored[s];
        } else {
          lost = 1;
        }
      }
    }
    base += __shfl(incl, 63);
    __syncthreads();
  }
  for (int a = 0; a < COCO_A; a++)
    for (int d = 32; d >= 1; d >>= 1) npig[a] += __shfl_xor(npig[a], d);
  const int any_lost = __ballot(lost) != 0ull;
  if (lane == 0) {
    st->n_rows = base;
    st->n_images = image0 + B;
    if (any_lost) st->overflow = 1;
    for (int a = 0; a < COCO_A; a++) st->n_gt[a] += npig[a];
  }
}

// ------------------------------------------------------------------------------------------
// accumulate
// ------------------------------------------------------------------------------------------
struct CocoWork {
  unsigned long long *e0, *e1;   // [cap] sort buffers: (key << 32) | row, ascending key = descending score
  float* score;                  // [cap] the table's columns in sorted order
  int* rank;
  unsigned long long* matched;
  unsigned long long* ignored;
  double* precision;             // [T][R][A][M]
  double* recall;                // [T][A][M]
  double* scores;                // [T][R][A][M]
};

// exclusive scan of one int per thread over the workgroup; returns the total.  tmp: CO_THREADS + 1 ints of LDS.
__device__ inline int coco_excl_scan(int v, int* tmp, int* total) {
  const int t = threadIdx.x;
  tmp[t] = v;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int i = 0; i < CO_THREADS; i++) { const int x = tmp[i]; tmp[i] = run; run += x; }
    tmp[CO_THREADS] = run;
  }
  __syncthreads();
  const int r = tmp[t];
  *total = tmp[CO_THREADS];
  __syncthreads();
  return r;
}

// the table's rows (at most cap of them) in stable descending-score order, every column gathered
__global__ __launch_bounds__(CO_THREADS) void coco_sort_kernel(CocoTable tab, const CocoState* st, CocoWork w) {
  __shared__ int digit_cnt[16 * CO_THREADS];
  __shared__ int itmp[CO_THREADS + 1];
  const int t = threadIdx.x;
  const int n = min(st->n_rows, tab.cap);
  const int chunk = (n + CO_THREADS - 1) / CO_THREADS;
  const int lo = min(n, t * chunk), hi = min(n, lo + chunk);
  for (int i = lo; i < hi; i++) w.e0[i] = ((unsigned long long)coco_score_key(tab.score[i]) << 32) | (unsigned long long)(unsigned)i;
  __syncthreads();
  // stable LSD radix sort on the 32 key bits, 4 bits a pass; thread t owns elements [lo, hi) of the pass's input
  unsigned long long *src = w.e0, *dst = w.e1;
  for (int pass = 0; pass < 8; pass++) {
    const int shift = 32 + 4 * pass;
    for (int d = 0; d < 16; d++) digit_cnt[d * CO_THREADS + t] = 0;
    for (int i = lo; i < hi; i++) digit_cnt[(int)((src[i] >> shift) & 15ull) * CO_THREADS + t] += 1;
    __syncthreads();
    // exclusive scan of digit_cnt in (digit, thread) order: thread t owns entries [16 t, 16 t + 16)
    int s = 0;
    for (int j = 0; j < 16; j++) s += digit_cnt[16 * t + j];
    int total;
    int run = coco_excl_scan(s, itmp, &total);
    for (int j = 0; j < 16; j++) { const int x = digit_cnt[16 * t + j]; digit_cnt[16 * t + j] = run; run += x; }
    __syncthreads();
    for (int i = lo; i < hi; i++) {
      const unsigned long long e = src[i];
      const int slot = (int)((e >> shift) & 15ull) * CO_THREADS + t;
      dst[digit_cnt[slot]++] = e;
    }
    __syncthreads();
    unsigned long long* x = src; src = dst; dst = x;
  }
  // 8 passes: the sorted table is back in e0 (= src)
  for (int i = t; i < n; i += CO_THREADS) {
    const int r = (int)(unsigned)(src[i] & 0xffffffffull);
    w.score[i] = tab.score[r];
    w.rank[i] = tab.rank[r];
    w.matched[i] = tab.matched[r];
    w.ignored[i] = tab.ignored[r];
  }
}

// COCOeval.accumulate for one (range a, maxDets m, threshold t) = blockIdx.x / 30, / 10 % 3, % 10
__global__ __launch_bounds__(CO_THREADS) void coco_accumulate_kernel(CocoWork w, const CocoState* st, int cap, const double* rec_thrs) {
  __shared__ int itmp[CO_THREADS + 1];
  __shared__ double dtmp[CO_THREADS];
  __shared__ double q[COCO_R], ss[COCO_R];
  const int tid = threadIdx.x;
  const int a = blockIdx.x / (COCO_M * COCO_T), m = (blockIdx.x / COCO_T) % COCO_M, t = blockIdx.x % COCO_T;
  const int n = min(st->n_rows, cap), npig = st->n_gt[a], max_det = coco_max_det(m);
  const unsigned long long bit = coco_bit(a, t);
  const size_t out_r = (size_t)(t * COCO_A + a) * COCO_M + m;
  if (npig == 0) {      // the whole slice stays -1
    for (int r = tid; r < COCO_R; r += CO_THREADS) {
      const size_t o = ((size_t)(t * COCO_R + r) * COCO_A + a) * COCO_M + m;
      w.precision[o] = -1.0;
      w.scores[o] = -1.0;
    }
    if (tid == 0) w.recall[out_r] = -1.0;
    return;
  }
  for (int r = tid; r < COCO_R; r += CO_THREADS) { q[r] = 0.0; ss[r] = 0.0; }
  const int chunk = (n + CO_THREADS - 1) / CO_THREADS;
  const int lo = min(n, tid * chunk), hi = min(n, lo + chunk);
  // rows with rank < maxDets; tp = matched & !ignored, fp = !matched & !ignored
  int c_keep = 0, c_tp = 0, c_fp = 0;
  for (int i = lo; i < hi; i++) {
    if (w.rank[i] >= max_det) continue;
    const bool mt = (w.matched[i] & bit) != 0ull, ig = (w.ignored[i] & bit) != 0ull;
    c_keep++;
    c_tp += (mt && !ig) ? 1 : 0;
    c_fp += (!mt && !ig) ? 1 : 0;
  }
  int n_keep, n_tp, n_fp;
  const int keep0 = coco_excl_scan(c_keep, itmp, &n_keep);
  const int tp0 = coco_excl_scan(c_tp, itmp, &n_tp);
  const int fp0 = coco_excl_scan(c_fp, itmp, &n_fp);
  // the largest precision of the chunk, then of everything behind the chunk: pr[i-1] = max(pr[i-1], pr[i]) from the right is a suffix maximum
  double cmax = -1.0;
  {
    int tp = tp0, fp = fp0;
    for (int i = lo; i < hi; i++) {
      if (w.rank[i] >= max_det) continue;
      const bool mt = (w.matched[i] & bit) != 0ull, ig = (w.ignored[i] & bit) != 0ull;
      tp += (mt && !ig) ? 1 : 0;
      fp += (!mt && !ig) ? 1 : 0;
      cmax = fmax(cmax, coco_precision(tp, fp));
    }
  }
  dtmp[tid] = cmax;
  __syncthreads();
  if (tid == 0) {
    double run = -1.0;
    for (int i = CO_THREADS - 1; i >= 0; i--) { const double x = dtmp[i]; dtmp[i] = run; run = fmax(run, x); }
  }
  __syncthreads();
  // from the right: the envelope, and searchsorted(rc, recThrs, 'left') - threshold r belongs to the first kept row whose recall reaches it
  {
    double run = dtmp[tid];
    int tp = tp0 + c_tp, fp = fp0 + c_fp, j = keep0 + c_keep - 1;      // inclusive counts and the kept index of the row at hand
    for (int i = hi - 1; i >= lo; i--) {
      if (w.rank[i] >= max_det) continue;
      const bool mt = (w.matched[i] & bit) != 0ull, ig = (w.ignored[i] & bit) != 0ull;
      const int is_tp = (mt && !ig) ? 1 : 0, is_fp = (!mt && !ig) ? 1 : 0;
      run = fmax(run, coco_precision(tp, fp));
      if (j == 0 || is_tp) {
        const double rc = coco_recall(tp, npig), rc_prev = j == 0 ? -1.0 : coco_recall(tp - is_tp, npig);
        int r = rc_prev < 0.0 ? 0 : max(0, (int)(rc_prev * 100.0) - 1);
        while (r < COCO_R && rec_thrs[r] <= rc_prev) r++;
        while (r < COCO_R && rec_thrs[r] <= rc) {
          q[r] = run;
          ss[r] = (double)w.score[i];
          r++;
        }
      }
      tp -= is_tp;
      fp -= is_fp;
      j--;
    }
  }
  __syncthreads();
  for (int r = tid; r < COCO_R; r += CO_THREADS) {
    const size_t o = ((size_t)(t * COCO_R + r) * COCO_A + a) * COCO_M + m;
    w.precision[o] = q[r];
    w.scores[o] = ss[r];
  }
  if (tid == 0) w.recall[out_r] = n_keep ? coco_recall(n_tp, npig) : 0.0;
}

}  // namespace vbt

using namespace vbt;

struct vbt_coco {
  int device = 0, max_batch = 0, rows_cap = 0;
  // owners of the table's, the per-call scratch's and the accumulate workspace's arrays; tab, batch and work are what the kernels take
  DevBuf<float> tab_score, batch_score, work_score;
  DevBuf<int> tab_image, tab_rank, batch_cnt, batch_npig, work_rank;
  DevBuf<unsigned long long> tab_matched, tab_ignored, batch_matched, batch_ignored, work_e0, work_e1, work_matched, work_ignored;
  DevBuf<double> out_precision, out_recall, out_scores, thrs;      // thrs: iouThrs [10] then recThrs [101]
  CocoTable tab{};
  CocoBatch batch{};
  CocoWork work{};
  DevBuf<CocoState> state;
  // staging of (meta, ground truth) uploads: CO_STAGES pinned slots + their device twins, an event each
  struct Stage {
    PinnedBuf<int> host;
    DevBuf<int> dev;
    Event ev;
    bool used = false;
  } stage[CO_STAGES];
  size_t stage_ints = 0;
  int next_stage = 0;
  hipStream_t last_stream = nullptr;
  Event done;                       // end of the last call's kernels: a call on another stream waits for it (shared scratch and staging)
  bool done_used = false;
  int images_host = 0;
};

namespace {

constexpr size_t CO_PR = (size_t)COCO_T * COCO_R * COCO_A * COCO_M, CO_RC = (size_t)COCO_T * COCO_A * COCO_M;

// the device state after everything enqueued so far (synchronises the handle's stream)
int coco_read_state(vbt_coco* c, CocoState* out) {
  VBT_HIP_CHECK(hipMemcpyAsync(out, c->state.get(), sizeof(CocoState), hipMemcpyDeviceToHost, c->last_stream));
  VBT_HIP_CHECK(hipStreamSynchronize(c->last_stream));
  if (out->overflow) {
    set_error("vbt_coco: the table holds %d rows, %d were produced", c->rows_cap, out->n_rows);
    return VBT_ERR_CAPACITY;
  }
  return VBT_OK;
}

}  // namespace

extern "C" {

int vbt_coco_create(int device, int max_batch, int rows_cap, vbt_coco** out) {
  if (!out || max_batch < 1 || max_batch > 4096 || rows_cap < 1) { set_error("vbt_coco_create: bad argument"); return VBT_ERR_ARG; }
  *out = nullptr;
  if (int rc = use_device("vbt_coco_create", device)) return rc;
  std::unique_ptr<vbt_coco> c(new vbt_coco());
  c->device = device; c->max_batch = max_batch; c->rows_cap = rows_cap;
  c->stage_ints = (size_t)max_batch * 4 + (size_t)max_batch * VBT_EVAL_MAX_GT * 4;
  hipError_t err = hipSuccess;
  auto get = [&](auto& buf, size_t count) { if (err == hipSuccess) err = buf.alloc(count); };
  const size_t r = (size_t)rows_cap, s = (size_t)max_batch * COCO_MAXD;
  get(c->tab_score, r); get(c->tab_image, r); get(c->tab_rank, r); get(c->tab_matched, r); get(c->tab_ignored, r);
  get(c->batch_score, s); get(c->batch_matched, s); get(c->batch_ignored, s); get(c->batch_cnt, (size_t)max_batch);
  get(c->batch_npig, (size_t)max_batch * COCO_A);
  get(c->work_e0, r); get(c->work_e1, r); get(c->work_score, r); get(c->work_rank, r); get(c->work_matched, r); get(c->work_ignored, r);
  get(c->out_precision, CO_PR); get(c->out_recall, CO_RC); get(c->out_scores, CO_PR); get(c->thrs, (size_t)COCO_T + COCO_R);
  get(c->state, 1);
  for (vbt_coco::Stage& st : c->stage) {
    get(st.dev, c->stage_ints);
    get(st.host, c->stage_ints);
    if (err == hipSuccess) err = st.ev.create(hipEventDisableTiming);
  }
  if (err == hipSuccess) err = c->done.create(hipEventDisableTiming);
  if (err == hipSuccess) err = hipMemset(c->state.get(), 0, sizeof(CocoState));
  double tables[COCO_T + COCO_R];
  coco_tables(tables, tables + COCO_T);      // computed on the host, as numpy computes them
  if (err == hipSuccess) err = hipMemcpy(c->thrs.get(), tables, sizeof(tables), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    set_error("vbt_coco_create: allocation failed: %s", hipGetErrorString(err));
    return VBT_ERR_HIP;
  }
  c->tab = CocoTable{c->tab_score.get(), c->tab_image.get(), c->tab_rank.get(), c->tab_matched.get(), c->tab_ignored.get(), rows_cap};
  c->batch = CocoBatch{c->batch_score.get(), c->batch_matched.get(), c->batch_ignored.get(), c->batch_cnt.get(), c->batch_npig.get()};
  c->work = CocoWork{c->work_e0.get(), c->work_e1.get(), c->work_score.get(), c->work_rank.get(), c->work_matched.get(), c->work_ignored.get(),
                     c->out_precision.get(), c->out_recall.get(), c->out_scores.get()};
  *out = c.release();
  return VBT_OK;
}

void vbt_coco_destroy(vbt_coco* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  delete c;
}

int vbt_coco_reset(vbt_coco* c) {
  if (!c) { set_error("NULL vbt_coco"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(c->device));
  VBT_HIP_CHECK(hipDeviceSynchronize());
  VBT_HIP_CHECK(hipMemset(c->state.get(), 0, sizeof(CocoState)));
  c->images_host = 0;
  return VBT_OK;
}

int vbt_coco_add_detections(vbt_coco* c, const float* boxes_dev, const float* scores_dev, const int32_t* counts_dev, int B,
                            const int32_t* hw_host, const int32_t* gt_offsets_host, const int32_t* gt_boxes_host, void* stream) {
  if (!c || !boxes_dev || !scores_dev || !counts_dev || !hw_host || !gt_offsets_host || B < 1) {
    set_error("vbt_coco_add_detections: bad argument");
    return VBT_ERR_ARG;
  }
  if (B > c->max_batch) { set_error("vbt_coco_add_detections: %d images, the handle takes %d per call", B, c->max_batch); return VBT_ERR_CAPACITY; }
  const int g_first = gt_offsets_host[0];
  for (int b = 0; b < B; b++) {
    const int n_gt = gt_offsets_host[b + 1] - gt_offsets_host[b];
    if (n_gt < 0 || hw_host[2 * b] < 1 || hw_host[2 * b + 1] < 1) {
      set_error("vbt_coco_add_detections: image %d of the call: decreasing ground-truth offsets or an empty image size", b);
      return VBT_ERR_ARG;
    }
    if (n_gt > VBT_EVAL_MAX_GT) {
      set_error("vbt_coco_add_detections: image %d (number %d of the call) has %d ground-truth boxes, the matcher takes %d", c->images_host + b, b,
                n_gt, VBT_EVAL_MAX_GT);
      return VBT_ERR_CAPACITY;
    }
  }
  const int total = gt_offsets_host[B] - g_first;
  if (total > 0 && !gt_boxes_host) { set_error("vbt_coco_add_detections: NULL ground-truth boxes"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  // the per-batch scratch, the staging slots and the table are shared by all calls: a call on another stream runs after the last one
  if (c->done_used && st != c->last_stream) VBT_HIP_CHECK(hipStreamWaitEvent(st, c->done.get(), 0));
  vbt_coco::Stage& sg = c->stage[c->next_stage];
  if (sg.used) VBT_HIP_CHECK(hipEventSynchronize(sg.ev.get()));   // the caller is CO_STAGES uploads ahead of the device
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
  c->next_stage = (c->next_stage + 1) % CO_STAGES;
  coco_match_kernel<<<B, 64, 0, st>>>(boxes_dev, scores_dev, counts_dev, sg.dev.get(), sg.dev.get() + 4 * (size_t)B, c->thrs.get(), c->batch);
  VBT_HIP_CHECK(hipGetLastError());
  coco_append_kernel<<<1, 64, 0, st>>>(c->batch, B, c->tab, c->state.get());
  VBT_HIP_CHECK(hipGetLastError());
  VBT_HIP_CHECK(hipEventRecord(c->done.get(), st));
  c->done_used = true;
  c->last_stream = st;
  c->images_host += B;
  return VBT_OK;
}

int vbt_coco_table(vbt_coco* c, int* n_rows, float* scores, int32_t* image, int32_t* rank, uint64_t* matched, uint64_t* ignored, int cap) {
  if (!c || !n_rows) { set_error("vbt_coco_table: bad argument"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(c->device));
  CocoState s;
  const int rc = coco_read_state(c, &s);
  *n_rows = s.n_rows;
  if (rc) return rc;
  if (!scores && !image && !rank && !matched && !ignored) return VBT_OK;
  if (s.n_rows > cap) { set_error("vbt_coco_table: %d rows, buffers hold %d", s.n_rows, cap); return VBT_ERR_CAPACITY; }
  const size_t n = (size_t)s.n_rows;
  if (n == 0) return VBT_OK;
  if (scores) VBT_HIP_CHECK(hipMemcpy(scores, c->tab.score, 4 * n, hipMemcpyDeviceToHost));
  if (image) VBT_HIP_CHECK(hipMemcpy(image, c->tab.image, 4 * n, hipMemcpyDeviceToHost));
  if (rank) VBT_HIP_CHECK(hipMemcpy(rank, c->tab.rank, 4 * n, hipMemcpyDeviceToHost));
  if (matched) VBT_HIP_CHECK(hipMemcpy(matched, c->tab.matched, 8 * n, hipMemcpyDeviceToHost));
  if (ignored) VBT_HIP_CHECK(hipMemcpy(ignored, c->tab.ignored, 8 * n, hipMemcpyDeviceToHost));
  return VBT_OK;
}

int vbt_coco_accumulate(vbt_coco* c, vbt_coco_summary* s, double* precision, double* recall, double* scores) {
  if (!c || !s) { set_error("vbt_coco_accumulate: bad argument"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(c->device));
  CocoState cs;
  if (int rc = coco_read_state(c, &cs)) return rc;
  hipStream_t st = c->last_stream;
  // the row and box counts are read by the kernels from the device state: the table never leaves the device for this call
  coco_sort_kernel<<<1, CO_THREADS, 0, st>>>(c->tab, c->state.get(), c->work);
  VBT_HIP_CHECK(hipGetLastError());
  coco_accumulate_kernel<<<COCO_A * COCO_M * COCO_T, CO_THREADS, 0, st>>>(c->work, c->state.get(), c->rows_cap, c->thrs.get() + COCO_T);
  VBT_HIP_CHECK(hipGetLastError());
  std::vector<double> pr(CO_PR), rc(CO_RC);
  VBT_HIP_CHECK(hipMemcpyAsync(pr.data(), c->work.precision, 8 * CO_PR, hipMemcpyDeviceToHost, st));
  VBT_HIP_CHECK(hipMemcpyAsync(rc.data(), c->work.recall, 8 * CO_RC, hipMemcpyDeviceToHost, st));
  if (scores) VBT_HIP_CHECK(hipMemcpyAsync(scores, c->work.scores, 8 * CO_PR, hipMemcpyDeviceToHost, st));
  VBT_HIP_CHECK(hipStreamSynchronize(st));
  coco_stats(pr.data(), rc.data(), s->stats);
  s->n_images = cs.n_images;
  s->n_rows = cs.n_rows;
  for (int a = 0; a < COCO_A; a++) s->n_gt[a] = cs.n_gt[a];
  if (precision) memcpy(precision, pr.data(), 8 * CO_PR);
  if (recall) memcpy(recall, rc.data(), 8 * CO_RC);
  return VBT_OK;
}

}  // extern "C"
