// The on-device trackers and row assembly for gfx950 (MI355X): the step kernels, the handle, the per-clip read-backs.  One step is
// ocsort_step.h (OC-SORT, the default) or - a handle made by vbt_tracker_create_sort - sort_step.h (SortTracker, the reference's
// commented-out alternative, track.py:16,156): each is its own association around the phases of step_phases.h, on the filter of
// box_filter.h and the state of tracker_state.h, and the kernels here are templates on the algorithm.  The detection list loaders and the
// state's LDS copy are clip_io.h; export id selection + rep analysis at the clip close are tracker_analysis.hip, the live rep analysis
// tracker_live.hip.
//
// Replaces, per clip (reference track.py:157-234, plot.py:33-47,87-95):
//   ocsort.OCSort(max_age=30, asso_func="diou", iou_threshold=0.1).update(dets, [])   track.py:157,186
//   the kf.x[4:6] read-back and the 8-column row assembly                               track.py:189-234
//   the max-cumulative-distance id selection of the export                              track.py:107-115
//   rolling(5)/expanding means + VelocityTracker scan                                  plot.py:87-95,33-47
// Execution model: ONE WAVEFRONT PER CLIP (clips are independent, frames of a clip are strictly
// sequential: Kalman + phase state).  Lane t owns live tracker t (<= 64 per clip): predict, IoU /
// direction-cost columns, Kalman update and row emission are lane-parallel; the linear assignment
// is a shortest-augmenting-path solver with lanes = columns and wave min-reductions; list
// maintenance (births, deletions) uses ballots.  All arithmetic is FP64 with contraction off and
// follows the op order of the numpy formulation, so the Kalman velocities are bit-identical to
// the reference's committed DataFrames (tests/test_gpu_tracker.py).
//   The 7-state SORT filter decouples into three (position, velocity) 2x2 filters (cx, cy, s) and a
// scalar one (r): F/H/Q/R never couple them, so the dense 7x7 products of the numpy formulation
// reduce EXACTLY (same roundings; the dropped terms are exact zeros) to the closed forms below.
#include <cmath>

#include "common.h"
#include "tracker_host.h"

namespace vbt {

// Phase timers of a tracker step (developer builds only: VBT_EXTRA_CXXFLAGS=-DVBT_TRK_PROF): s_memtime deltas per phase, accumulated
// by lane 0 of every wavefront; read back with vbt_tracker_prof_read.  TrkClock is the step's clock, handed to a shared phase that
// marks inside its body; it is empty in every other build.
#ifdef VBT_TRK_PROF
__device__ unsigned long long g_trk_prof[16];
struct TrkClock { unsigned long long t; };
#define TRK_T0() TrkClock _tp{__builtin_amdgcn_s_memtime()}
#define TRK_MARK(i) do { unsigned long long _tn = __builtin_amdgcn_s_memtime(); if (threadIdx.x == 0) atomicAdd(&g_trk_prof[i], _tn - _tp.t); _tp.t = _tn; } while (0)
#else
struct TrkClock {};
#define TRK_T0() TrkClock _tp
#define TRK_MARK(i) do {} while (0)
#endif

// MAXPH (phases kept per clip) is defined in tracker_state.h
static_assert(CLOSED_HEAD_BYTES == 16 + (size_t)MAXPH * 48, "slot close record (common.h)");

}  // namespace vbt

#include "clip_io.h"
#include "ocsort_step.h"
#include "sort_step.h"

namespace vbt {

// The step kernels below exist once per algorithm, selected at compile time: SORT = false walks ocsort_step (OCSort, track.py:157),
// SORT = true sort_step (SortTracker, track.py:16,156).  The handle's `sort` flag picks the instantiation at every launch.
template <bool SORT>
__device__ __forceinline__ void clip_step(ClipState& st, Row* rows, int rows_cap, StepShared& sh, int nd, double time, const TrackParams& p,
                                          double q44, double q66, int lane) {
  if constexpr (SORT) sort_step(st, rows, rows_cap, sh, nd, time, p, q44, q66, lane);
  else ocsort_step(st, rows, rows_cap, sh, nd, time, p, q44, q66, lane);
}
// host-provided detections of a frame -> the detection list, by one lane (OC-SORT gates them by score, SORT takes all)
template <bool SORT>
__device__ __forceinline__ int put_host(StepShared& sh, const double (*d)[6], int n, double det_thresh) {
  if constexpr (SORT) return put_host_detections_all(sh, d, n);
  else return put_host_detections(sh, d, n, det_thresh);
}

// Frames come either as double detections (host-provided, OCSort.update call shape) ...
template <bool SORT>
__global__ __launch_bounds__(64) void tracker_kernel(ClipState* states, Row* rows, int rows_cap, const double* dets,
                                                     const int* counts, const double* times, int F, int nclips, TrackParams p,
                                                     double q44, double q66) {
  __shared__ StepShared sh;
  const int clip = blockIdx.x, lane = threadIdx.x;
  ClipState& st = states[clip];
  Row* myrows = rows + (size_t)clip * rows_cap;
  for (int f = 0; f < F; f++) {
    const int n = counts[(size_t)f * nclips + clip];
    if (n <= 0) continue;  // reference track.py:180-181: the tracker is not stepped on empty frames
    const double* d = dets + ((size_t)f * nclips + clip) * MAXD * 6;
    __syncthreads();
    if (lane == 0) sh.flag = put_host<SORT>(sh, (const double (*)[6])d, n, p.det_thresh);
    __syncthreads();
    clip_step<SORT>(st, myrows, rows_cap, sh, sh.flag, times[(size_t)f * nclips + clip], p, q44, q66, lane);
  }
}

// The reference's own call shape - tracker.update(dets, []) once per frame on ONE clip, then tracker.trackers[i].id / .kf.x
// (track.py:186-199): the frame's detections and its time stamp travel in the kernel arguments (no allocation, no host-to-device
// copy), and what the caller reads back afterwards - update()'s rows and every live tracker's id + kf.x - is packed into one small
// block that comes back with ONE stream-ordered copy into pinned memory (the per-call path used to cost three hipMalloc, three
// blocking copies and two device-wide synchronisations).
struct OneFrameArg {
  double det[MAXD][6];
  double time;
  int n;
};
constexpr int VIEW_DOUBLES = 2 + MAXD * 9 + MAXT * 8;   // last_n, ntrk | last_out[25][9] | per tracker: id, x[7]
template <bool SORT>
__global__ __launch_bounds__(64) void tracker_one_kernel(ClipState* states, Row* rows, int rows_cap, int clip, OneFrameArg a, TrackParams p,
                                                         double q44, double q66, double* view) {
  __shared__ StepShared sh;
  const int lane = threadIdx.x;
  ClipState& st = states[clip];
  if (lane == 0) sh.flag = put_host<SORT>(sh, a.det, a.n, p.det_thresh);
  __syncthreads();
  clip_step<SORT>(st, rows + (size_t)clip * rows_cap, rows_cap, sh, sh.flag, a.time, p, q44, q66, lane);
  __syncthreads();
  if (lane == 0) { view[0] = (double)st.last_n; view[1] = (double)st.ntrk; }
  for (int i = lane; i < MAXD * 9; i += 64) view[2 + i] = (&st.last_out[0][0])[i];
  if (lane < st.ntrk) {
    const Trk& k = st.trk[st.order[lane]];
    double* o = view + 2 + MAXD * 9 + lane * 8;
    o[0] = (double)k.id;
    for (int j = 0; j < 7; j++) o[1 + j] = k.x[j];
  }
}

// ... or straight from the detector's device outputs (fused pipeline): applies the detection
// threshold of reference odt.py:70-75 and the reorder of odt.py:102-118.
// slot = position in the detector batch; clip = tracker state it feeds (map == nullptr: the same index; a negative entry
// or a negative time: the slot carries no frame in this step)
// The per-step metadata (frame time and clip of every slot) travels as a kernel argument: no host-to-device copy, no
// host buffer that has to outlive the call.  64 slots per launch; larger batches take several launches (slot0).
constexpr int META_SLOTS = 64;
struct StepMeta {
  double time[META_SLOTS];
  int clip[META_SLOTS];
};
template <bool SORT>
__global__ __launch_bounds__(64) void tracker_from_det_kernel(ClipState* states, Row* rows, int rows_cap, const float* boxes,
                                                              const float* scores, const int* counts, StepMeta meta, int slot0,
                                                              float det_threshold, TrackParams p, double q44, double q66) {
  __shared__ StepShared sh;
  const int slot = slot0 + blockIdx.x, lane = threadIdx.x;
  const int clip = meta.clip[blockIdx.x];
  const double frame_time = meta.time[blockIdx.x];
  if (clip < 0 || !(frame_time >= 0.0)) return;
  ClipState& st = states[clip];
  const int nd = load_slot_detections(sh, boxes, scores, counts, slot, det_threshold, p.det_thresh, lane);
  __syncthreads();
  if (nd < 0) return;
  clip_step<SORT>(st, rows + (size_t)clip * rows_cap, rows_cap, sh, nd, frame_time, p, q44, q66, lane);
}

// Time-batched form (the reference's unit of work is ONE video, track.py:85-126,159-247): the detector batch holds RUNS of
// consecutive frames of a clip instead of one frame of each of B clips - the detector is stateless, so a single clip fills
// the whole batch.  One wavefront per run walks its frames in order (frame f of the run sits in detector slot
// slot0 + f * slot_stride); the frame time is frame_count / fps (track.py:161,169) with frame_count = frame0 + f * frame_step,
// one IEEE division like the reference's.  Run descriptors travel in the kernel arguments (64 runs per launch).
constexpr int META_RUNS = 64;
struct RunMeta {
  int clip, slot0, slot_stride, n_frames, frame0, frame_step;
  double fps;
};
struct SeqMeta {
  RunMeta run[META_RUNS];
};
// A run of SEQ_LDS_MIN frames or more keeps the clip's tracker state in LDS for the whole walk: the header and the live
// tracks (a few KB) are copied in once and written back once, and every Kalman / association step in between works on LDS
// instead of on dependent global round trips (one clip alone: 21 us -> see DESIGN.md per frame).
constexpr int SEQ_LDS_MIN = 6;
template <bool SORT>
__global__ __launch_bounds__(64) void tracker_seq_kernel(ClipState* states, Row* rows, int rows_cap, const float* boxes,
                                                         const float* scores, const int* counts, SeqMeta meta,
                                                         float det_threshold, TrackParams p, double q44, double q66, int lds_state) {
  __shared__ StepShared sh;
  extern __shared__ __attribute__((aligned(16))) unsigned char seq_dyn[];   // ClipState copy (only when lds_state != 0)
  const int lane = threadIdx.x;
  const RunMeta r = meta.run[blockIdx.x];
  if (r.clip < 0) return;
  ClipState* gst = &states[r.clip];
  ClipState* st = gst;
  const bool cached = lds_state != 0 && r.n_frames >= lds_state;   // lds_state = shortest run that is worth the copy in and out
  if (cached) {
    ClipState* lst = (ClipState*)seq_dyn;
    clip_state_copy<true>(lst, gst, sh.um_t, lane);
    st = lst;
  }
  Row* myrows = rows + (size_t)r.clip * rows_cap;
  // Two copies of the walk, one per home of the state: in each the compiler knows the address space of every access to the clip state
  // (LDS: ds_read / ds_write; global memory: global_load / global_store).  With one copy on a pointer that may be either, every
  // access was a FLAT instruction - slower to issue, and each one counted on both wait counters, so that every wait drained both
  // queues (the walk was 5 600 instructions with 270 flat accesses and 240 waits).
  auto walk = [&](ClipState& state) {
    RawDet cur = fetch_slot_detections(boxes, scores, counts, r.slot0, lane);
    for (int f = 0; f < r.n_frames; f++) {
      // frame f + 1's detections are requested now and looked at in the next iteration (the last frame re-requests itself)
      const RawDet nxt = fetch_slot_detections(boxes, scores, counts, r.slot0 + min(f + 1, r.n_frames - 1) * r.slot_stride, lane);
      __syncthreads();  // the previous frame's readers of sh.det are done
      const int nd = put_slot_detections(sh, cur, det_threshold, p.det_thresh, lane);
      __syncthreads();
      cur = nxt;
      if (nd < 0) continue;
      const double frame_time = (double)(r.frame0 + f * r.frame_step) / r.fps;
      clip_step<SORT>(state, myrows, rows_cap, sh, nd, frame_time, p, q44, q66, lane);
    }
  };
  if (cached) walk(*(ClipState*)seq_dyn);
  else walk(*gst);
  if (cached) {   // write the state back: header + every slot that is live now (slots freed during the walk need no copy)
    __syncthreads();
    clip_state_copy<false>(st, gst, sh.um_t, lane);
  }
}

__global__ void init_states_kernel(ClipState* states, int n, int id_base) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  init_state(states[i], id_base);
}

// A fresh clip in every listed slot (vbt_tracker_reset_clips), one workgroup per listed clip: its ClipState as init_states_kernel leaves it
// and - live analysis on (clips != nullptr) - its LiveClip and LIVE_ENTRIES entries as live_init_kernel leaves them.
__global__ __launch_bounds__(64) void reset_clips_kernel(ClipState* states, LiveClip* clips, LiveEntry* ents, ClipList l, int id_base) {
  const int clip = l.clip[blockIdx.x], lane = threadIdx.x;
  if (lane == 0) init_state(states[clip], id_base);
  if (!clips) return;
  if (lane == 0) live_clip_init(clips[clip]);
  for (int e = lane; e < LIVE_ENTRIES; e += 64) live_entry_free(ents[(size_t)clip * LIVE_ENTRIES + e]);
}

}  // namespace vbt

using namespace vbt;

int vbt::fetch_state_header(vbt_tracker* t, int clip, StateHeader* h) {
  VBT_HIP_CHECK(hipMemcpy(h->bytes, t->states.get() + clip, sizeof(h->bytes), hipMemcpyDeviceToHost));
  return VBT_OK;
}

int vbt::fetch_state_headers(vbt_tracker* t, std::vector<StateHeader>* h, hipStream_t st) {
  h->resize((size_t)t->n_clips);
  VBT_HIP_CHECK(hipMemcpy2DAsync(h->data(), sizeof(StateHeader), t->states.get(), sizeof(ClipState), sizeof(StateHeader), t->n_clips,
                                 hipMemcpyDeviceToHost, st));
  VBT_HIP_CHECK(hipStreamSynchronize(st));
  return VBT_OK;
}

int vbt::check_sort_params(const char* who, const vbt_sort_params* sp) {
  if (!sp) { set_error("%s: NULL parameters", who); return VBT_ERR_ARG; }
  if (sp->max_age < 0 || sp->min_hits < 0) { set_error("%s: max_age and min_hits must be >= 0", who); return VBT_ERR_ARG; }
  if (!std::isfinite(sp->iou_threshold)) { set_error("%s: iou_threshold must be finite", who); return VBT_ERR_ARG; }
  if (sp->id_base < 0 || sp->id_base > VBT_SORT_MAX_ID_BASE) { set_error("%s: id_base must be in [0, %d]", who, VBT_SORT_MAX_ID_BASE); return VBT_ERR_ARG; }
  return VBT_OK;
}

int vbt::tracker_use_sort(vbt_tracker* t, const vbt_sort_params* sp) {
  if (!t) { set_error("NULL tracker"); return VBT_ERR_ARG; }
  if (int rc = check_sort_params("SORT parameters", sp)) return rc;
  if (t->stepped) { set_error("the tracker has been stepped: its algorithm is fixed"); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(t->device));
  t->sort = true;
  t->id_base = sp->id_base;
  t->p = TrackParams{};
  t->p.max_age = sp->max_age; t->p.min_hits = sp->min_hits; t->p.iou_thr = sp->iou_threshold;
  t->p.delta_t = 1;                      // (unused by sort_step)
  t->p.det_thresh = -HUGE_VAL;           // no score gate: put_slot_detections keeps every detection at or above det_threshold
  return vbt_tracker_reset(t);           // clip states with next_id = id_base
}

int vbt::check_state_header(const vbt_tracker* t, int clip, const StateHeader& h, int cap) {
  if (h->overflow > 0) { set_error("clip %d: more than %d live tracks (%d births dropped)", clip, MAXT, h->overflow); return VBT_ERR_CAPACITY; }
  if (h->rows_overflow > 0) { set_error("clip %d: row capacity %d exceeded by %d", clip, t->rows_cap, h->rows_overflow); return VBT_ERR_CAPACITY; }
  if (h->nrows > cap) { set_error("clip %d has %d rows, buffer holds %d", clip, h->nrows, cap); return VBT_ERR_CAPACITY; }
  return VBT_OK;
}

namespace {

// What tracker_one_kernel packs for `clip` - last_n, ntrk | last_out[25][9] | per tracker: id, x[7] - wherever it comes from: the
// one-frame path brought it back already (view_clip), any other path left it in the clip's state, whose first `state_bytes` are read
// and laid out the same way in `tmp`.
int clip_view(vbt_tracker* t, int clip, size_t state_bytes, std::vector<double>* tmp, const double** view) {
  if (t->view_clip == clip) { *view = (const double*)t->view.host(); return VBT_OK; }
  VBT_HIP_CHECK(hipDeviceSynchronize());
  std::vector<char> buf(state_bytes);
  VBT_HIP_CHECK(hipMemcpy(buf.data(), t->states.get() + clip, buf.size(), hipMemcpyDeviceToHost));
  const ClipState* st = (const ClipState*)buf.data();
  tmp->assign(VIEW_DOUBLES, 0.0);
  double* v = tmp->data();
  v[0] = (double)st->last_n; v[1] = (double)st->ntrk;
  memcpy(v + 2, st->last_out, sizeof(st->last_out));
  if (state_bytes == sizeof(ClipState))
    for (int i = 0; i < st->ntrk; i++) {
      const Trk& k = st->trk[st->order[i]];
      double* o = v + 2 + MAXD * 9 + i * 8;
      o[0] = (double)k.id;
      memcpy(o + 1, k.x, sizeof(k.x));
    }
  *view = v;
  return VBT_OK;
}

}  // namespace

extern "C" {

int vbt_tracker_create(int n_clips, int rows_cap, const vbt_tracker_params* prm, int device, vbt_tracker** out) {
  if (!out || !prm || n_clips < 1 || rows_cap < 1) { set_error("vbt_tracker_create: bad argument"); return VBT_ERR_ARG; }
  if (prm->delta_t < 1 || prm->delta_t > 3) { set_error("delta_t must be 1..3"); return VBT_ERR_ARG; }
  *out = nullptr;
  if (int rc = use_device("vbt_tracker_create", device)) return rc;
  std::unique_ptr<vbt_tracker> t(new vbt_tracker());
  t->n_clips = n_clips; t->rows_cap = rows_cap; t->device = device;
  t->p.max_age = prm->max_age; t->p.min_hits = prm->min_hits; t->p.delta_t = prm->delta_t; t->p.asso = prm->asso;
  t->p.iou_thr = prm->iou_threshold; t->p.inertia = prm->inertia; t->p.det_thresh = prm->det_thresh;
  // Q = eye(7); Q[-1,-1] *= 0.01; Q[4:,4:] *= 0.01
  double q = 1.0;
  q *= 0.01;
  t->q44 = q;
  double q6 = 1.0;
  q6 *= 0.01;
  q6 *= 0.01;
  t->q66 = q6;
  // in this order, up to the first failure.  The clip-close record buffers (device + pinned host) at their largest size: no allocation
  // on the first close
  const size_t n = (size_t)n_clips, nr = n * rows_cap;
  auto no = [](hipError_t e) { return e != hipSuccess; };
  const char* failed = no(t->states.alloc(n))                                 ? "tracker state"
                       : no(t->rows.alloc(nr))                                ? "rows"
                       : no(t->cols.alloc(7 * nr))                            ? "cols"
                       : no(t->scratch.alloc(5 * nr))                         ? "scratch"
                       : no(t->phases.alloc(6 * MAXPH * n))                   ? "phases"
                       : no(t->nph.alloc(n))                                  ? "nph"
                       : no(t->T.alloc(n))                                    ? "T"
                       : no(t->best.alloc(n))                                 ? "best"
                       : no(t->summary.reserve((16 + (size_t)MAXPH * 48) * n)) ? (t->summary.dev() ? "pinned summary" : "summary")
                       : no(t->view.reserve(sizeof(double) * VIEW_DOUBLES))   ? (t->view.dev() ? "pinned view" : "view")
                                                                              : nullptr;
  if (failed) { set_error("hipMalloc failed for %s", failed); return VBT_ERR_HIP; }
  init_states_kernel<<<(n_clips + 63) / 64, 64>>>(t->states.get(), n_clips, t->id_base);
  VBT_HIP_CHECK(hipDeviceSynchronize());
  *out = t.release();
  return VBT_OK;
}

int vbt_tracker_create_sort(int n_clips, int rows_cap, const vbt_sort_params* sp, int device, vbt_tracker** out) {
  if (!out || !sp || n_clips < 1 || rows_cap < 1) { set_error("vbt_tracker_create_sort: bad argument"); return VBT_ERR_ARG; }
  *out = nullptr;
  if (int rc = check_sort_params("vbt_tracker_create_sort", sp)) return rc;
  // the handle, its buffers and fresh clip states are those of any tracker; then the algorithm and its parameters
  const vbt_tracker_params base = {sp->max_age, sp->min_hits, 1, 0, sp->iou_threshold, 0.0, 0.0};
  vbt_tracker* t = nullptr;
  if (int rc = vbt_tracker_create(n_clips, rows_cap, &base, device, &t)) return rc;
  std::unique_ptr<vbt_tracker> owner(t);
  if (int rc = tracker_use_sort(t, sp)) return rc;
  *out = owner.release();
  return VBT_OK;
}

void vbt_tracker_destroy(vbt_tracker* t) { delete t; }

int vbt_tracker_reset(vbt_tracker* t) {
  if (!t) { set_error("NULL tracker"); return VBT_ERR_ARG; }
  init_states_kernel<<<(t->n_clips + 63) / 64, 64>>>(t->states.get(), t->n_clips, t->id_base);
  if (t->live) live_init(t);
  VBT_HIP_CHECK(hipDeviceSynchronize());
  t->finished = false;
  t->view_clip = -1;
  t->stepped = false;
  return VBT_OK;
}

int vbt_tracker_reset_clips(vbt_tracker* t, const int32_t* clips, int n, void* stream) {
  if (!t) { set_error("NULL tracker"); return VBT_ERR_ARG; }
  if (int rc = check_clip_list("vbt_tracker_reset_clips", clips, n, t->n_clips)) return rc;
  VBT_HIP_CHECK(hipSetDevice(t->device));
  hipStream_t st = (hipStream_t)stream;
  for (int i0 = 0; i0 < n; i0 += CLIP_LIST) {
    const ClipList l = clip_list(clips, i0, n);
    reset_clips_kernel<<<l.n, 64, 0, st>>>(t->states.get(), t->live ? t->lb.clips : nullptr, t->live ? t->lb.ents : nullptr, l, t->id_base);
  }
  VBT_HIP_CHECK(hipGetLastError());
  t->view_clip = -1;
  return VBT_OK;
}

int vbt_tracker_update(vbt_tracker* t, const double* dets, const int32_t* counts, const double* times, int F) {
  RoctxRange range("vbt:track");
  if (!t || !dets || !counts || !times || F < 1) { set_error("vbt_tracker_update: bad argument"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(t->device));
  t->view_clip = -1;
  if (F == 1 && t->n_clips == 1) {   // OCSort.update(dets, []) of the reference's loop: everything in the kernel arguments
    if (counts[0] <= 0) return VBT_OK;   // (track.py:180-181: the tracker is not stepped on empty frames)
    OneFrameArg a;
    a.n = std::min((int)counts[0], MAXD);
    a.time = times[0];
    memcpy(a.det, dets, sizeof(double) * 6 * a.n);
    (t->sort ? tracker_one_kernel<true> : tracker_one_kernel<false>)<<<1, 64, 0, nullptr>>>(t->states.get(), t->rows.get(), t->rows_cap, 0, a, t->p, t->q44, t->q66,
                                                                                              (double*)t->view.dev());
    VBT_HIP_CHECK(hipGetLastError());
    if (int rc = live_after(t, nullptr)) return rc;
    VBT_HIP_CHECK(t->view.fetch(sizeof(double) * VIEW_DOUBLES, nullptr));
    t->view_clip = 0;
    t->finished = false;
    return VBT_OK;
  }
  size_t nd = (size_t)F * t->n_clips;
  DevBuf<double> dd, dt;   // freed on every way out; on the good one after the device-wide synchronisation below
  DevBuf<int> dc;
  VBT_HIP_CHECK(dd.alloc(nd * MAXD * 6));
  VBT_HIP_CHECK(dc.alloc(nd));
  VBT_HIP_CHECK(dt.alloc(nd));
  VBT_HIP_CHECK(hipMemcpy(dd.get(), dets, nd * MAXD * 6 * sizeof(double), hipMemcpyHostToDevice));
  VBT_HIP_CHECK(hipMemcpy(dc.get(), counts, nd * sizeof(int), hipMemcpyHostToDevice));
  VBT_HIP_CHECK(hipMemcpy(dt.get(), times, nd * sizeof(double), hipMemcpyHostToDevice));
  (t->sort ? tracker_kernel<true> : tracker_kernel<false>)<<<t->n_clips, 64>>>(t->states.get(), t->rows.get(), t->rows_cap, dd.get(), dc.get(), dt.get(), F, t->n_clips,
                                                                               t->p, t->q44, t->q66);
  const int lrc = live_after(t, nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) { set_error("tracker kernel failed: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
  if (lrc != VBT_OK) return lrc;
  t->finished = false;
  return VBT_OK;
}

// One tracker step for slots [0, n_slots): launches of at most META_SLOTS workgroups, metadata in the kernel arguments.
static int launch_steps(vbt_tracker* t, const float* boxes_dev, const float* scores_dev, const int32_t* counts_dev, const int32_t* clip_of_slot,
                        const double* times, int n_slots, float det_threshold, hipStream_t st) {
  RoctxRange range("vbt:track");
  if (((uintptr_t)boxes_dev & 15) != 0) { set_error("tracker update: boxes_dev must be 16-byte aligned"); return VBT_ERR_ARG; }
  for (int s0 = 0; s0 < n_slots; s0 += META_SLOTS) {
    const int nb = std::min(META_SLOTS, n_slots - s0);
    StepMeta meta;
    for (int i = 0; i < nb; i++) {
      meta.time[i] = times[s0 + i];
      meta.clip[i] = clip_of_slot ? clip_of_slot[s0 + i] : s0 + i;
    }
    (t->sort ? tracker_from_det_kernel<true> : tracker_from_det_kernel<false>)<<<nb, 64, 0, st>>>(t->states.get(), t->rows.get(), t->rows_cap, boxes_dev, scores_dev,
                                                                                                 counts_dev, meta, s0, det_threshold, t->p, t->q44, t->q66);
  }
  VBT_HIP_CHECK(hipGetLastError());
  if (int rc = live_after(t, st)) return rc;
  t->finished = false;
  t->view_clip = -1;
  return VBT_OK;
}

int vbt_tracker_update_from_detections(vbt_tracker* t, const float* boxes_dev, const float* scores_dev, const int32_t* counts_dev,
                                       const double* times_host, float det_threshold, void* stream) {
  if (!t || !boxes_dev || !scores_dev || !counts_dev || !times_host) { set_error("bad argument"); return VBT_ERR_ARG; }
  return launch_steps(t, boxes_dev, scores_dev, counts_dev, nullptr, times_host, t->n_clips, det_threshold, (hipStream_t)stream);
}

int vbt_tracker_update_from_slots(vbt_tracker* t, const float* boxes_dev, const float* scores_dev, const int32_t* counts_dev,
                                  const int32_t* clip_of_slot_host, const double* times_host, int n_slots, float det_threshold,
                                  void* stream) {
  if (!t || !boxes_dev || !scores_dev || !counts_dev || !clip_of_slot_host || !times_host || n_slots < 1 || n_slots > t->n_clips) {
    set_error("vbt_tracker_update_from_slots: bad argument (n_slots must be in [1, n_clips])");
    return VBT_ERR_ARG;
  }
  for (int i = 0; i < n_slots; i++) {
    if (clip_of_slot_host[i] >= t->n_clips) { set_error("slot %d -> clip %d, tracker has %d clips", i, clip_of_slot_host[i], t->n_clips); return VBT_ERR_ARG; }
    for (int j = 0; j < i; j++)
      if (clip_of_slot_host[i] >= 0 && clip_of_slot_host[i] == clip_of_slot_host[j]) { set_error("clip %d sits in two slots", clip_of_slot_host[i]); return VBT_ERR_ARG; }
  }
  return launch_steps(t, boxes_dev, scores_dev, counts_dev, clip_of_slot_host, times_host, n_slots, det_threshold, (hipStream_t)stream);
}

int vbt_tracker_update_from_detections_seq(vbt_tracker* t, const float* boxes_dev, const float* scores_dev, const int32_t* counts_dev,
                                           int n_slots, const vbt_run* runs_host, int n_runs, float det_threshold, void* stream) {
  RoctxRange range("vbt:track");
  if (!t || !boxes_dev || !scores_dev || !counts_dev || !runs_host || n_runs < 1 || n_slots < 1) {
    set_error("vbt_tracker_update_from_detections_seq: bad argument");
    return VBT_ERR_ARG;
  }
  if (((uintptr_t)boxes_dev & 15) != 0) { set_error("vbt_tracker_update_from_detections_seq: boxes_dev must be 16-byte aligned"); return VBT_ERR_ARG; }
  // every run stays inside the detector batch and no clip appears twice (two wavefronts would step one Kalman state)
  std::vector<char> seen((size_t)t->n_clips, 0);
  for (int i = 0; i < n_runs; i++) {
    const vbt_run& r = runs_host[i];
    if (r.clip < 0) continue;  // an empty descriptor
    if (r.clip >= t->n_clips) { set_error("run %d: clip %d, tracker has %d clips", i, r.clip, t->n_clips); return VBT_ERR_ARG; }
    if (seen[r.clip]) { set_error("run %d: clip %d appears in two runs of one call", i, r.clip); return VBT_ERR_ARG; }
    seen[r.clip] = 1;
    if (r.n_frames < 1 || r.frame0 < 1 || r.frame_step < 1 || !(r.fps > 0.0)) { set_error("run %d: n_frames, frame0, frame_step >= 1 and fps > 0 required", i); return VBT_ERR_ARG; }
    const long long last = (long long)r.slot0 + (long long)(r.n_frames - 1) * r.slot_stride;
    if (r.slot0 < 0 || r.slot0 >= n_slots || last < 0 || last >= n_slots) {
      set_error("run %d: slots %d..%lld outside the detector batch of %d", i, r.slot0, last, n_slots);
      return VBT_ERR_ARG;
    }
    if ((long long)r.frame0 + (long long)(r.n_frames - 1) * r.frame_step > 0x7fffffffLL) { set_error("run %d: frame number overflow", i); return VBT_ERR_ARG; }
  }
  hipStream_t st = (hipStream_t)stream;
  VBT_HIP_CHECK(hipSetDevice(t->device));     // (the LDS opt-in below is a per-device function attribute)
  for (int r0 = 0; r0 < n_runs; r0 += META_RUNS) {
    const int nb = std::min(META_RUNS, n_runs - r0);
    SeqMeta meta;
    for (int i = 0; i < nb; i++) {
      const vbt_run& r = runs_host[r0 + i];
      meta.run[i] = RunMeta{r.clip, r.slot0, r.slot_stride, r.n_frames, r.frame0, r.frame_step, r.fps};
    }
    int longest = 0;
    for (int i = 0; i < nb; i++) longest = std::max(longest, meta.run[i].clip >= 0 ? meta.run[i].n_frames : 0);
    static const bool lds_off = getenv("VBT_SEQ_NO_LDS") != nullptr;
    static const int lds_min = getenv("VBT_SEQ_LDS_MIN") ? std::max(1, atoi(getenv("VBT_SEQ_LDS_MIN"))) : SEQ_LDS_MIN;
    int lds_state = (longest >= lds_min && !lds_off) ? lds_min : 0;
    if (lds_state) {
      // opt in to the dynamic LDS of the cached state once per device; if the runtime refuses, the walk works on global memory
      static int attr_state[2][64] = {{0}};   // per algorithm and device: 0 = not tried, 1 = granted, -1 = refused
      const int di = t->device < 64 ? t->device : 63;
      int& as = attr_state[t->sort ? 1 : 0][di];
      if (as == 0)
        as = hipFuncSetAttribute(t->sort ? reinterpret_cast<const void*>(&tracker_seq_kernel<true>) : reinterpret_cast<const void*>(&tracker_seq_kernel<false>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(ClipState)) == hipSuccess ? 1 : -1;
      if (as < 0) lds_state = 0;
    }
    (t->sort ? tracker_seq_kernel<true> : tracker_seq_kernel<false>)<<<nb, 64, lds_state ? sizeof(ClipState) : 0, st>>>(
        t->states.get(), t->rows.get(), t->rows_cap, boxes_dev, scores_dev, counts_dev, meta, det_threshold, t->p, t->q44, t->q66, lds_state);
  }
  VBT_HIP_CHECK(hipGetLastError());
  if (int rc = live_after(t, st)) return rc;
  t->finished = false;
  t->view_clip = -1;
  return VBT_OK;
}

#ifdef VBT_TRK_PROF
int vbt_tracker_prof_read(unsigned long long* out16, int reset) {
  VBT_HIP_CHECK(hipDeviceSynchronize());
  VBT_HIP_CHECK(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_trk_prof), sizeof(unsigned long long) * 16));
  if (reset) {
    unsigned long long z[16] = {0};
    VBT_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_trk_prof), z, sizeof(z)));
  }
  return VBT_OK;
}
#endif

int vbt_tracker_last_output(vbt_tracker* t, int clip, double* out7, double* vel2, int cap, int* M) {
  if (!t || !out7 || !vel2 || !M || clip < 0 || clip >= t->n_clips) { set_error("bad argument"); return VBT_ERR_ARG; }
  std::vector<double> tmp;
  const double* view = nullptr;
  if (int rc = clip_view(t, clip, offsetof(ClipState, trk), &tmp, &view)) return rc;
  const int n = std::min((int)view[0], cap);
  for (int i = 0; i < n; i++) {
    const double* lo = view + 2 + i * 9;
    for (int j = 0; j < 7; j++) out7[i * 7 + j] = lo[j];
    vel2[i * 2] = lo[7];
    vel2[i * 2 + 1] = lo[8];
  }
  *M = n;
  return VBT_OK;
}

int vbt_tracker_status(vbt_tracker* t, int clip, int32_t* n_rows, int32_t* n_trackers, int32_t* overflow, int32_t* rows_overflow,
                       int32_t* frame_count) {
  if (!t || clip < 0 || clip >= t->n_clips) { set_error("bad argument"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipDeviceSynchronize());
  StateHeader st;
  if (int rc = fetch_state_header(t, clip, &st)) return rc;
  if (n_rows) *n_rows = st->nrows;
  if (n_trackers) *n_trackers = st->ntrk;
  if (overflow) *overflow = st->overflow;
  if (rows_overflow) *rows_overflow = st->rows_overflow;
  if (frame_count) *frame_count = st->frame_count;
  return VBT_OK;
}

int vbt_tracker_get_trackers(vbt_tracker* t, int clip, int32_t* ids, double* kfx, int cap, int* n) {
  if (!t || !ids || !kfx || !n || clip < 0 || clip >= t->n_clips) { set_error("bad argument"); return VBT_ERR_ARG; }
  std::vector<double> tmp;
  const double* view = nullptr;
  if (int rc = clip_view(t, clip, sizeof(ClipState), &tmp, &view)) return rc;
  const int m = std::min((int)view[1], cap);
  for (int i = 0; i < m; i++) {
    const double* o = view + 2 + MAXD * 9 + i * 8;
    ids[i] = (int32_t)o[0];
    for (int j = 0; j < 7; j++) kfx[i * 7 + j] = o[1 + j];
  }
  *n = m;
  return VBT_OK;
}

int vbt_tracker_rows(vbt_tracker* t, int clip, int64_t* id, double* cols7, int cap, int* n) {
  if (!t || !id || !cols7 || !n || clip < 0 || clip >= t->n_clips) { set_error("bad argument"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipDeviceSynchronize());
  StateHeader st;
  if (int rc = fetch_state_header(t, clip, &st)) return rc;
  if (int rc = check_state_header(t, clip, st, cap)) return rc;
  int m = st->nrows;
  std::vector<Row> r(m);
  if (m) VBT_HIP_CHECK(hipMemcpy(r.data(), t->rows.get() + (size_t)clip * t->rows_cap, sizeof(Row) * m, hipMemcpyDeviceToHost));
  for (int i = 0; i < m; i++) {
    id[i] = r[i].id;
    double* o = cols7 + (size_t)i * 7;
    o[0] = r[i].time; o[1] = r[i].x; o[2] = r[i].y; o[3] = r[i].dx; o[4] = r[i].dy; o[5] = r[i].h; o[6] = r[i].w;
  }
  *n = m;
  return VBT_OK;
}

}  // extern "C"
