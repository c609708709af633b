// Clip close of the on-device tracker (tracker.hip): export id selection, the rows of the winner, the rep analysis of those rows and the
// packed records the host reads; vbt_analyze / vbt_window_means, the same scans on rows handed in by the caller.
#include "common.h"
#include "rep_analysis.h"
#include "tracker_host.h"

namespace vbt {

// metrics: [n_clips][MAXPH][VT_METRICS] (M: rep metrics on; else not read)
template <bool M>
__global__ __launch_bounds__(64) void analyze_kernel(const double* cols, const int* T, int stride_rows, VtParams p, double* scratch,
                                                     double* phases, double* metrics, int* nph, ClipList l) {
  const int clip = listed_clip(l);
  if (threadIdx.x != 0) return;
  analyze_track<M>(cols + (size_t)clip * stride_rows * 7, T[clip], p, scratch + (size_t)clip * stride_rows * 5,
                phases + (size_t)clip * MAXPH * 6, M ? metrics + (size_t)clip * MAXPH * VT_METRICS : nullptr, nph + clip);
}

// pandas rolling(window, min_periods=1).mean() (window > 0) / expanding(min_periods=1).mean() (window == 0) of every
// column of a row-major [T][ncols] table; lane = column (plot.py:90-95, kinovea.py:99-105, qualysis.py:113-117).
__global__ __launch_bounds__(64) void window_means_kernel(const double* rows, int T, int ncols, const int* windows, double* out) {
  const int c = threadIdx.x;
  if (c >= ncols) return;
  const int w = windows[c];
  RollMean r;
  r.init();
  for (int i = 0; i < T; i++) {
    double v = rows[(size_t)i * ncols + c];
    if (w >= 0) {
      if (w > 0 && i >= w) r.remove(rows[(size_t)(i - w) * ncols + c]);
      r.add(v);
      v = r.mean();
    }
    out[(size_t)i * ncols + c] = v;
  }
}

// end of clip: live tracks compete for the export id too; then gather the rows of the winner.
__global__ __launch_bounds__(64) void select_gather_kernel(ClipState* states, const Row* rows, int rows_cap, double* cols, int* T,
                                                           int* best_ids, ClipList l) {
  const int clip = listed_clip(l), lane = threadIdx.x;
  ClipState& st = states[clip];
  __shared__ int s_best;
  if (lane == 0) {
    const int bi = export_id(st);
    s_best = bi;
    best_ids[clip] = bi;
  }
  __syncthreads();
  const int best = s_best;
  const Row* r = rows + (size_t)clip * rows_cap;
  double* c = cols + (size_t)clip * rows_cap * 7;
  const int n = st.nrows;
  int outn = 0;  // stable, ordered gather with ballots
  for (int base = 0; base < n; base += 64) {
    int i = base + lane;
    bool hit = i < n && best >= 0 && r[i].id == best;
    unsigned long long m = __ballot(hit);
    if (hit) {
      double* o = c + (size_t)(outn + __popcll(m & ((1ull << lane) - 1ull))) * 7;
      o[0] = r[i].time; o[1] = r[i].x; o[2] = r[i].y; o[3] = r[i].dx; o[4] = r[i].dy; o[5] = r[i].h; o[6] = r[i].w;
    }
    outn += __popcll(m);
  }
  if (lane == 0) T[clip] = outn;
}

// Clip close: everything the host reads per clip, packed into one block so that ONE copy fetches it:
//   record c = { int best_id, n_rows, n_phases, overflow ; double phases[cap][6] }
// On a clip list (vbt_pipeline_close_clips, cap = MAXPH) the records of the listed clips only, straight into pinned host memory.
// metrics != null: the metrics of those phases too, clip c's min(n_phases, cap) records at mdst + c * mstride doubles.
__global__ __launch_bounds__(64) void pack_summary_kernel(const ClipState* states, const int* best, const int* nph, const double* phases,
                                                          int cap, unsigned char* out, ClipList l, const double* metrics, double* mdst,
                                                          size_t mstride) {
  const int clip = listed_clip(l), lane = threadIdx.x;
  const size_t rec = 16 + (size_t)cap * 48;
  unsigned char* o = out + clip * rec;
  const int n = nph[clip];
  if (lane == 0) {
    int* h = (int*)o;
    h[0] = best[clip]; h[1] = states[clip].nrows; h[2] = n; h[3] = states[clip].overflow | states[clip].rows_overflow;
  }
  double* ph = (double*)(o + 16);
  const double* src = phases + (size_t)clip * MAXPH * 6;
  for (int i = lane; i < min(n, cap) * 6; i += 64) ph[i] = src[i];
  if (metrics) {
    const double* ms = metrics + (size_t)clip * MAXPH * VT_METRICS;
    double* md = mdst + clip * mstride;
    for (int i = lane; i < min(n, cap) * VT_METRICS; i += 64) md[i] = ms[i];
  }
}

// Slot close (vbt_pipeline_close_clips): the first n_rows rows of every listed clip's log - the 64-byte records of vbt_tracker_rows_all -
// into out_rows + clip * rows_cap (device memory: the slot's log is overwritten as soon as its next clip steps).  One workgroup per clip.
__global__ __launch_bounds__(64) void close_rows_kernel(const ClipState* states, const Row* rows, int rows_cap, ClipList l, Row* out_rows) {
  const int clip = l.clip[blockIdx.x], lane = threadIdx.x;
  const int nr = states[clip].nrows;   // <= rows_cap (the log never grows past it)
  const uint4* rs = (const uint4*)(rows + (size_t)clip * rows_cap);   // 4 x 16 bytes per row
  uint4* rd = (uint4*)(out_rows + (size_t)clip * rows_cap);
  for (int i = lane; i < nr * 4; i += 64) rd[i] = rs[i];
}

}  // namespace vbt

using namespace vbt;

namespace {

// export id + rep analysis of the clips of l (no list: of every clip), enqueue only
void enqueue_analysis(vbt_tracker* t, double plate_diameter, double diff_threshold, double min_distance, const ClipList& l, hipStream_t st) {
  const int nb = l.n ? l.n : t->n_clips;
  const VtParams vp{plate_diameter, diff_threshold, min_distance, 1, 1};
  select_gather_kernel<<<nb, 64, 0, st>>>(t->states.get(), t->rows.get(), t->rows_cap, t->cols.get(), t->T.get(), t->best.get(), l);
  if (t->rep_metrics)
    analyze_kernel<true><<<nb, 64, 0, st>>>(t->cols.get(), t->T.get(), t->rows_cap, vp, t->scratch.get(), t->phases.get(), t->metrics.get(), t->nph.get(), l);
  else
    analyze_kernel<false><<<nb, 64, 0, st>>>(t->cols.get(), t->T.get(), t->rows_cap, vp, t->scratch.get(), t->phases.get(), nullptr, t->nph.get(), l);
}

}  // namespace

namespace vbt {

int unpack_phases(const char* what, long long id, const unsigned char* src, int n, double* phases6, size_t c, int cap) {
  if (n > cap) { set_error("%s %lld: %d phases, buffer holds %d", what, id, n, cap); return VBT_ERR_CAPACITY; }
  if (n > 0) memcpy(phases6 + c * cap * 6, src, (size_t)n * 48);
  return VBT_OK;
}

int check_clip_list(const char* fn, const int32_t* clips, int n, int n_clips) {
  if (!clips || n < 1) { set_error("%s: a list of at least one clip required", fn); return VBT_ERR_ARG; }
  std::vector<char> seen((size_t)n_clips, 0);
  for (int i = 0; i < n; i++) {
    const int c = clips[i];
    if (c < 0 || c >= n_clips) { set_error("%s: clip %d outside the %d clips", fn, c, n_clips); return VBT_ERR_ARG; }
    if (seen[(size_t)c]) { set_error("%s: clip %d listed twice", fn, c); return VBT_ERR_ARG; }
    seen[(size_t)c] = 1;
  }
  return VBT_OK;
}

int tracker_close_clips(vbt_tracker* t, const int32_t* clips, int n, double plate_diameter, double diff_threshold, double min_distance,
                        unsigned char* head, double* mhead, void* out_rows, hipStream_t st) {
  RoctxRange range("vbt:close_clips");
  for (int i0 = 0; i0 < n; i0 += CLIP_LIST) {
    const ClipList l = clip_list(clips, i0, n);
    enqueue_analysis(t, plate_diameter, diff_threshold, min_distance, l, st);
    pack_summary_kernel<<<l.n, 64, 0, st>>>(t->states.get(), t->best.get(), t->nph.get(), t->phases.get(), MAXPH, head, l,
                                            mhead ? t->metrics.get() : nullptr, mhead, (size_t)MAXPH * VT_METRICS);
    close_rows_kernel<<<l.n, 64, 0, st>>>(t->states.get(), t->rows.get(), t->rows_cap, l, (Row*)out_rows);
  }
  VBT_HIP_CHECK(hipGetLastError());
  return vbt_tracker_reset_clips(t, clips, n, (void*)st);
}

}  // namespace vbt

extern "C" {

int vbt_tracker_finish(vbt_tracker* t, double plate_diameter, double diff_threshold, double min_distance, void* stream) {
  RoctxRange range("vbt:finish");
  if (!t) { set_error("NULL tracker"); return VBT_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  enqueue_analysis(t, plate_diameter, diff_threshold, min_distance, ClipList{}, st);
  VBT_HIP_CHECK(hipGetLastError());
  t->finished = true;
  t->finish_stream = st;
  return VBT_OK;
}

int vbt_tracker_phases(vbt_tracker* t, int clip, int32_t* best_id, double* phases6, int cap, int* P) {
  if (!t || !best_id || !phases6 || !P || clip < 0 || clip >= t->n_clips) { set_error("bad argument"); return VBT_ERR_ARG; }
  if (!t->finished) { set_error("vbt_tracker_phases before vbt_tracker_finish"); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipDeviceSynchronize());
  StateHeader st;   // a clip that dropped births or rows has no export id to stand behind: refused as vbt_tracker_rows refuses it
  if (int rc = fetch_state_header(t, clip, &st)) return rc;
  if (int rc = check_state_header(t, clip, st, t->rows_cap)) return rc;
  int n = 0;
  VBT_HIP_CHECK(hipMemcpy(&n, t->nph.get() + clip, sizeof(int), hipMemcpyDeviceToHost));
  VBT_HIP_CHECK(hipMemcpy(best_id, t->best.get() + clip, sizeof(int), hipMemcpyDeviceToHost));
  if (n > cap) { set_error("clip %d has %d phases, buffer holds %d", clip, n, cap); return VBT_ERR_CAPACITY; }
  if (n) VBT_HIP_CHECK(hipMemcpy(phases6, t->phases.get() + (size_t)clip * MAXPH * 6, sizeof(double) * 6 * n, hipMemcpyDeviceToHost));
  *P = n;
  return VBT_OK;
}

// vbt_analyze (metrics8 == nullptr) / vbt_analyze_metrics
static int analyze_rows(const char* fn, const double* cols7, int T, int preprocess, int flush, double plate_diameter, double diff_threshold,
                        double min_distance, double* phases6, double* metrics8, int cap, int* P, int device) {
  if (!cols7 && T > 0) { set_error("%s: NULL rows", fn); return VBT_ERR_ARG; }
  if (!phases6 || !P || T < 0) { set_error("%s: bad argument", fn); return VBT_ERR_ARG; }
  if (int rc = use_device(fn, device)) return rc;
  *P = 0;
  if (T == 0) return VBT_OK;
  DevBuf<double> dc, ds, dp, dm;   // freed on every way out; on the good one after the last blocking copy
  DevBuf<int> dn, dT;
  VBT_HIP_CHECK(dc.alloc((size_t)7 * T));
  VBT_HIP_CHECK(ds.alloc((size_t)5 * T));
  VBT_HIP_CHECK(dp.alloc((size_t)6 * MAXPH));
  if (metrics8) VBT_HIP_CHECK(dm.alloc((size_t)VT_METRICS * MAXPH));
  VBT_HIP_CHECK(dn.alloc(1));
  VBT_HIP_CHECK(dT.alloc(1));
  VBT_HIP_CHECK(hipMemcpy(dc.get(), cols7, sizeof(double) * 7 * T, hipMemcpyHostToDevice));
  VBT_HIP_CHECK(hipMemcpy(dT.get(), &T, sizeof(int), hipMemcpyHostToDevice));
  VtParams vp{plate_diameter, diff_threshold, min_distance, preprocess, flush};
  if (metrics8) analyze_kernel<true><<<1, 64>>>(dc.get(), dT.get(), T, vp, ds.get(), dp.get(), dm.get(), dn.get(), ClipList{});
  else analyze_kernel<false><<<1, 64>>>(dc.get(), dT.get(), T, vp, ds.get(), dp.get(), nullptr, dn.get(), ClipList{});
  int n = 0;
  hipError_t e = hipMemcpy(&n, dn.get(), sizeof(int), hipMemcpyDeviceToHost);
  if (e != hipSuccess) { set_error("analyze kernel failed: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
  if (n > cap) { set_error("%d phases, buffer holds %d", n, cap); return VBT_ERR_CAPACITY; }
  if (n) (void)hipMemcpy(phases6, dp.get(), sizeof(double) * 6 * n, hipMemcpyDeviceToHost);
  if (n && metrics8) VBT_HIP_CHECK(hipMemcpy(metrics8, dm.get(), sizeof(double) * VT_METRICS * n, hipMemcpyDeviceToHost));
  *P = n;
  return VBT_OK;
}

int vbt_analyze(const double* cols7, int T, int preprocess, int flush, double plate_diameter, double diff_threshold,
                double min_distance, double* phases6, int cap, int* P, int device) {
  return analyze_rows("vbt_analyze", cols7, T, preprocess, flush, plate_diameter, diff_threshold, min_distance, phases6, nullptr, cap, P, device);
}

int vbt_analyze_metrics(const double* cols7, int T, int preprocess, int flush, double plate_diameter, double diff_threshold,
                        double min_distance, double* phases6, double* metrics8, int cap, int* P, int device) {
  if (!metrics8) { set_error("vbt_analyze_metrics: bad argument"); return VBT_ERR_ARG; }
  return analyze_rows("vbt_analyze_metrics", cols7, T, preprocess, flush, plate_diameter, diff_threshold, min_distance, phases6, metrics8, cap, P,
                      device);
}

int vbt_tracker_rep_metrics_enable(vbt_tracker* t) {
  if (!t) { set_error("NULL tracker"); return VBT_ERR_ARG; }
  if (t->rep_metrics) return VBT_OK;
  if (t->stepped) { set_error("vbt_tracker_rep_metrics_enable: the tracker has been stepped (enable before the first update, or after a reset)"); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(t->device));
  if (t->metrics.alloc((size_t)t->n_clips * MAXPH * VT_METRICS) != hipSuccess) {
    (void)hipGetLastError();
    set_error("vbt_tracker_rep_metrics_enable: hipMalloc of the metrics failed (%d clips)", t->n_clips);
    return VBT_ERR_HIP;
  }
  t->rep_metrics = true;
  if (!live_metrics_alloc(t)) {
    t->rep_metrics = false;
    t->metrics.reset();
    (void)hipGetLastError();
    set_error("vbt_tracker_rep_metrics_enable: hipMalloc of the live metrics failed (%d clips, phase_cap %d)", t->n_clips, t->lc.phase_cap);
    return VBT_ERR_HIP;
  }
  return VBT_OK;
}

int vbt_tracker_rep_metrics(vbt_tracker* t, int clip, double* metrics8, int cap, int* P) {
  if (!t || !metrics8 || !P || clip < 0 || clip >= t->n_clips) { set_error("vbt_tracker_rep_metrics: bad argument"); return VBT_ERR_ARG; }
  if (!t->rep_metrics) { set_error("vbt_tracker_rep_metrics: rep metrics are not enabled (vbt_tracker_rep_metrics_enable)"); return VBT_ERR_STATE; }
  if (!t->finished) { set_error("vbt_tracker_rep_metrics before vbt_tracker_finish"); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipDeviceSynchronize());
  StateHeader st;   // (refused as vbt_tracker_phases refuses it)
  if (int rc = fetch_state_header(t, clip, &st)) return rc;
  if (int rc = check_state_header(t, clip, st, t->rows_cap)) return rc;
  int n = 0;
  VBT_HIP_CHECK(hipMemcpy(&n, t->nph.get() + clip, sizeof(int), hipMemcpyDeviceToHost));
  if (n > cap) { set_error("clip %d has %d phases, buffer holds %d", clip, n, cap); return VBT_ERR_CAPACITY; }
  if (n) VBT_HIP_CHECK(hipMemcpy(metrics8, t->metrics.get() + (size_t)clip * MAXPH * VT_METRICS, sizeof(double) * VT_METRICS * n, hipMemcpyDeviceToHost));
  *P = n;
  return VBT_OK;
}

int vbt_window_means(const double* rows, int T, int ncols, const int32_t* windows, double* out, int device) {
  if (T < 0 || ncols < 1 || ncols > 64 || !windows || (T > 0 && (!rows || !out))) { set_error("vbt_window_means: bad argument"); return VBT_ERR_ARG; }
  if (int rc = use_device("vbt_window_means", device, /*set_current=*/false)) return rc;
  if (T == 0) return VBT_OK;
  VBT_HIP_CHECK(hipSetDevice(device));
  DevBuf<double> din, dout;   // freed on every way out; on the good one after the blocking copy of the result
  DevBuf<int> dw;
  const size_t cells = (size_t)T * ncols, bytes = sizeof(double) * cells;
  VBT_HIP_CHECK(din.alloc(cells));
  VBT_HIP_CHECK(dout.alloc(cells));
  VBT_HIP_CHECK(dw.alloc((size_t)ncols));
  VBT_HIP_CHECK(hipMemcpy(din.get(), rows, bytes, hipMemcpyHostToDevice));
  VBT_HIP_CHECK(hipMemcpy(dw.get(), windows, sizeof(int) * ncols, hipMemcpyHostToDevice));
  window_means_kernel<<<1, 64>>>(din.get(), T, ncols, dw.get(), dout.get());
  hipError_t e = hipMemcpy(out, dout.get(), bytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { set_error("window means kernel failed: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
  return VBT_OK;
}

// Clip close, host side: one pack kernel, ONE asynchronous copy into pinned memory, ONE stream synchronisation (on the
// stream vbt_tracker_finish ran on - not a device-wide one).
// metrics8 != nullptr (vbt_tracker_summary_ex): the block carries, behind the n_clips records, n_clips x pcap metrics records.
static int tracker_summary(vbt_tracker* t, int32_t* best_ids, int32_t* n_rows, int32_t* n_phases, int32_t* overflow, double* phases6,
                           double* metrics8, int cap) {
  const int n = t->n_clips;
  const int pcap = std::min(cap, MAXPH);   // phases packed per clip (a clip never holds more than MAXPH); cap stays the caller's stride
  const size_t rec = 16 + (size_t)pcap * 48, mrec = (size_t)pcap * VT_METRICS * sizeof(double);
  const size_t bytes = rec * n + (metrics8 ? mrec * n : 0);
  VBT_HIP_CHECK(t->summary.reserve(bytes));
  hipStream_t st = t->finish_stream;
  pack_summary_kernel<<<n, 64, 0, st>>>(t->states.get(), t->best.get(), t->nph.get(), t->phases.get(), pcap, t->summary.dev(), ClipList{},
                                        metrics8 ? t->metrics.get() : nullptr, (double*)(t->summary.dev() + rec * n), (size_t)pcap * VT_METRICS);
  VBT_HIP_CHECK(t->summary.fetch(bytes, st));
  for (int c = 0; c < n; c++) {
    const unsigned char* r = t->summary.host() + c * rec;
    const int* h = (const int*)r;
    best_ids[c] = h[0]; n_rows[c] = h[1]; n_phases[c] = h[2]; overflow[c] = h[3];
    if (int rc = unpack_phases("clip", c, r + 16, h[2], phases6, (size_t)c, cap)) return rc;
    if (metrics8) unpack_metrics(t->summary.host() + rec * n + c * mrec, h[2], metrics8, (size_t)c, cap);
  }
  return VBT_OK;
}

int vbt_tracker_summary(vbt_tracker* t, int32_t* best_ids, int32_t* n_rows, int32_t* n_phases, int32_t* overflow, double* phases6, int cap) {
  if (!t || !best_ids || !n_rows || !n_phases || !overflow || !phases6 || cap < 1) { set_error("bad argument"); return VBT_ERR_ARG; }
  if (!t->finished) { set_error("vbt_tracker_summary before vbt_tracker_finish"); return VBT_ERR_STATE; }
  return tracker_summary(t, best_ids, n_rows, n_phases, overflow, phases6, nullptr, cap);
}

int vbt_tracker_summary_ex(vbt_tracker* t, int32_t* best_ids, int32_t* n_rows, int32_t* n_phases, int32_t* overflow, double* phases6,
                           double* metrics8, int cap) {
  if (!t || !best_ids || !n_rows || !n_phases || !overflow || !phases6 || !metrics8 || cap < 1) { set_error("vbt_tracker_summary_ex: bad argument"); return VBT_ERR_ARG; }
  if (!t->rep_metrics) { set_error("vbt_tracker_summary_ex: rep metrics are not enabled (vbt_tracker_rep_metrics_enable)"); return VBT_ERR_STATE; }
  if (!t->finished) { set_error("vbt_tracker_summary_ex before vbt_tracker_finish"); return VBT_ERR_STATE; }
  return tracker_summary(t, best_ids, n_rows, n_phases, overflow, phases6, metrics8, cap);
}

// DataFrame rows of EVERY clip (all ids, emission order) in one strided copy: rows_host = [n_clips][cap] records of
// 64 bytes {int64 id; double time, x, y, dx, dy, norm_plate_height, norm_plate_width} (reference track.py:227-234).
// counts[c] = rows of clip c.  rows_host may be pinned (then the copy is one DMA) or pageable.
int vbt_tracker_rows_dev(vbt_tracker* t, int clip, const void** rows_dev, const int32_t** nrows_dev, int* rows_cap) {
  if (!t || !rows_dev || !nrows_dev || !rows_cap) { set_error("vbt_tracker_rows_dev: NULL argument"); return VBT_ERR_ARG; }
  if (clip < 0 || clip >= t->n_clips) { set_error("vbt_tracker_rows_dev: clip %d outside the %d clips", clip, t->n_clips); return VBT_ERR_ARG; }
  static_assert(sizeof(Row) == 64 && sizeof(int) == sizeof(int32_t), "row record and its counter");
  *rows_dev = t->rows.get() + (size_t)clip * t->rows_cap;
  *nrows_dev = (const int32_t*)((const char*)(t->states.get() + clip) + offsetof(ClipState, nrows));
  *rows_cap = t->rows_cap;
  return VBT_OK;
}

int vbt_tracker_rows_all(vbt_tracker* t, int32_t* counts, void* rows_host, int cap, void* stream) {
  if (!t || !counts || !rows_host || cap < 1) { set_error("vbt_tracker_rows_all: bad argument"); return VBT_ERR_ARG; }
  static_assert(sizeof(Row) == 64, "row record");
  hipStream_t st = (hipStream_t)stream;
  const int n = t->n_clips;
  std::vector<StateHeader> heads;
  if (int rc = fetch_state_headers(t, &heads, st)) return rc;
  int most = 0;
  for (int c = 0; c < n; c++) {
    if (int rc = check_state_header(t, c, heads[c], cap)) return rc;
    counts[c] = heads[c]->nrows;
    most = std::max(most, heads[c]->nrows);
  }
  if (most > 0) {
    VBT_HIP_CHECK(hipMemcpy2DAsync(rows_host, sizeof(Row) * (size_t)cap, t->rows.get(), sizeof(Row) * (size_t)t->rows_cap, sizeof(Row) * (size_t)most, n,
                                   hipMemcpyDeviceToHost, st));
    VBT_HIP_CHECK(hipStreamSynchronize(st));
  }
  return VBT_OK;
}

}  // extern "C"
