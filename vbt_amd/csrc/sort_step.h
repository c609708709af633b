// One SortTracker.update() (sort-track 0.0.8, the commented-out alternative of reference track.py:16,156) for one clip by one wavefront,
// in ocsort_step's execution model: lane t owns live track t, FP64 with contraction off, the op order of the numpy formulation
// (tests/sort_ref.py).  Device code, included by tracker.hip.  sort_step is the shared phases of step_phases.h - predict_and_drop_nan,
// gate_and_assign, births, emit_and_delete - around what is SORT's own: the cost on IoU alone, the undoing of pairs below the threshold
// and the list of detections to start tracks from.
//   What SORT does not have: the direction term of the cost, the second association on last observations, the freeze / unfreeze
// re-update, update(None), the score gate.  What it does differently: z is built with r = w / h (no 1e-6), a row is the filter's
// POSTERIOR box, not the observation, and a track dropped for a NaN box competes for the export id (its rows are in the log).  Trk /
// ClipState keep their layout: the OC-SORT-only fields of a track are set at birth and never read, so the clip close, the live analysis,
// the overlay's readers and clip_state_copy work on a SORT clip unchanged.
#pragma once
#include "step_phases.h"

namespace vbt {

// convert_bbox_to_z of SORT: r = w / float(h), without OC-SORT's 1e-6 (a zero-height box gives r = inf or NaN - see predict_and_drop_nan)
__device__ inline void sort_bbox_to_z(const double* b, double z[4]) {
  double w = b[2] - b[0], h = b[3] - b[1];
  z[0] = b[0] + w / 2.0;
  z[1] = b[1] + h / 2.0;
  z[2] = w * h;
  z[3] = w / h;
}

// KalmanBoxTracker.update(bbox) of SORT: counters, one filter update, the detection's score and class
__device__ inline void sort_trk_update(Trk& k, const double* det_in) {
  KfCore c;
  core_load(c, k);
  const double det[6] = {det_in[0], det_in[1], det_in[2], det_in[3], det_in[4], det_in[5]};   // in registers before the first store
  k.time_since_update = 0;
  k.hits += 1;
  k.hit_streak += 1;
  double z[4];
  sort_bbox_to_z(det, z);
  kf_update_math(c, z);
  core_store(k, c);
  k.conf = det[4];
  k.cls = det[5];
}

// get_state(): a row is the posterior, whatever the observation was
__device__ inline void sort_row_box(const Trk& k, double bx[4]) { x_to_bbox(k.x, bx); }

__device__ void sort_step(ClipState& st, Row* rows, int rows_cap, StepShared& sh, int nd, double time, const TrackParams& p,
                          double q44, double q66, int lane) {
  TRK_T0();
  if (lane == 0) st.frame_count += 1;
  const int T = predict_and_drop_nan<true>(st, sh, q44, q66, lane);
  const int slot = lane < T ? st.order[lane] : 0;
  TRK_MARK(0);   // predict
  // ---- association on IoU alone: the (detection, track) entries dealt to the 64 lanes pair by pair ----
  {
    const int npairs = nd * T;
    for (int p0 = 0; p0 < npairs; p0 += 64) {
      const int pr = p0 + lane;
      if (pr < npairs) {
        const int d = pr / T, t = pr - d * T;
        const double io = iou_xyxy(sh.det[d], sh.tbox[t]);
        sh.iou[d][t] = io;
        sh.cost[d][t] = -io;
      }
    }
  }
  if (lane < MAXD) sh.d2t[lane] = -1;
  __syncthreads();
  const int my_det = gate_and_assign(sh, nd, T, p.iou_thr, lane, _tp);   // detection matched to this lane's track
  TRK_MARK(2);   // assignment
  // d2t[d]: track position paired with detection d (-1: none); a pair with IoU below the threshold is undone, its detection then
  // counts as unmatched BEHIND the never-paired ones (the reference appends it to the list), which is the order of the births
  const bool was_paired = lane < T && my_det >= 0;
  bool rejected = false;
  if (was_paired) {
    rejected = sh.iou[my_det][lane] < p.iou_thr;
    sh.d2t[my_det] = rejected ? -2 : lane;
  }
  __syncthreads();
  if (was_paired && !rejected) sort_trk_update(st.trk[slot], sh.det[my_det]);
  TRK_MARK(11);  // matched Kalman updates
  {
    const unsigned long long below = (1ull << lane) - 1ull;
    const int dt_ = lane < nd ? sh.d2t[lane] : 0;
    const bool un_d = lane < nd && dt_ == -1, rj_d = lane < nd && dt_ == -2;
    const unsigned long long mU = __ballot(un_d), mR = __ballot(rj_d);
    const int nU = __popcll(mU);
    if (un_d) sh.um_d[__popcll(mU & below)] = lane;          // (nd <= MAXD: every position is below MAXD)
    if (rj_d) sh.um_d[nU + __popcll(mR & below)] = lane;
    if (lane == 0) sh.n_um_d = nU + __popcll(mR);
  }
  __syncthreads();
  TRK_MARK(3);   // unmatched list
  births<sort_bbox_to_z>(st, sh, lane);
  TRK_MARK(5);   // births
  emit_and_delete<sort_row_box>(st, rows, rows_cap, time, p, lane);
  TRK_MARK(6);   // emission + deletion
#ifdef VBT_TRK_PROF
  if (threadIdx.x == 0) { atomicAdd(&g_trk_prof[8], 1ull); atomicAdd(&g_trk_prof[9], (unsigned long long)nd); atomicAdd(&g_trk_prof[10], (unsigned long long)st.ntrk); }
#endif
}

}  // namespace vbt
