// One SortTracker.update() (sort-track 0.0.8, the commented-out alternative of reference track.py:16,156) for one clip by one wavefront,
// beside ocsort_step and in its execution model: lane t owns live track t, FP64 with contraction off, the op order of the numpy
// formulation (tests/sort_ref.py).  Device code, included by tracker.hip after ocsort_step.h, whose filter blocks (kf_predict,
// kf_update_math, x_to_bbox, iou_xyxy), StepShared and assignment solver (lap.h) it uses as they are.
//   What SORT does not have: the direction term of the cost, the second association on last observations, the freeze / unfreeze
// re-update, update(None), the score gate.  What it does differently: z is built with r = w / h (no 1e-6), and a row is the filter's
// POSTERIOR box, not the observation.  Trk / ClipState keep their layout: the OC-SORT-only fields of a track are set at birth and
// never read; cum / cum_c / prev_x / prev_y, last_out, best_cum / best_id are kept as ocsort_step keeps them, so the clip close, the
// live analysis, the overlay's readers and clip_state_copy work on a SORT clip unchanged.
//   Predict with its NaN removal and emission with its deletions repeat ocsort_step's text rather than share a function with it: the
// OC-SORT step is compiled from the same text as before this file existed.
#pragma once
#include "ocsort_step.h"

namespace vbt {

// convert_bbox_to_z of SORT: r = w / float(h), without OC-SORT's 1e-6 (a zero-height box gives r = inf or NaN - see the NaN removal)
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

// Host-provided detections -> the detection list, by ONE lane: all of them, order kept (SORT has no score gate)
__device__ __forceinline__ int put_host_detections_all(StepShared& sh, const double (*d)[6], int n) {
  const int m = min(n, MAXD);
  for (int i = 0; i < m; i++)
    for (int j = 0; j < 6; j++) sh.det[i][j] = d[i][j];
  return m;
}

__device__ void sort_step(ClipState& st, Row* rows, int rows_cap, StepShared& sh, int nd, double time, const TrackParams& p,
                          double q44, double q66, int lane) {
  TRK_T0();
  if (lane == 0) st.frame_count += 1;
  int T = st.ntrk;
  // ---- predict (KalmanBoxTracker.predict) ----
  bool isnan_box = false;
  if (lane < T) {
    Trk& k = st.trk[st.order[lane]];
    KfCore c;
    core_load(c, k);
    if ((c.x[6] + c.x[2]) <= 0.0) c.x[6] *= 0.0;
    kf_predict(c, q44, q66);
    core_store(k, c);
    k.age += 1;
    if (k.time_since_update > 0) k.hit_streak = 0;
    k.time_since_update += 1;
    double bx[4];
    x_to_bbox(c.x, bx);
    isnan_box = (bx[0] != bx[0]) || (bx[1] != bx[1]) || (bx[2] != bx[2]) || (bx[3] != bx[3]);
#pragma unroll
    for (int i = 0; i < 4; i++) sh.tbox[lane][i] = bx[i];
  }
  // np.ma.compress_rows(np.ma.masked_invalid(trks)) + pop: a track whose predicted box holds a NaN leaves the list (stable compaction).
  // A detection of zero height gets here one frame after its birth: r = w / 0 = inf, s = 0, w = sqrt(0 * inf) = NaN.
  // Bounds: only lanes < T write, to positions np_ < popcount(keep) <= T <= MAXT of order[] / tbox[]; the cleared slots are slots of
  // live lanes (slot < MAXT = 64 bits of `used`).
  unsigned long long nanmask = __ballot(isnan_box);
  if (nanmask) {
    unsigned long long keep = ~nanmask & (T >= 64 ? ~0ull : ((1ull << T) - 1ull));
    int slot = lane < T ? st.order[lane] : 0;
    double bx[4] = {0, 0, 0, 0};
    if (lane < T)
      for (int i = 0; i < 4; i++) bx[i] = sh.tbox[lane][i];
    __syncthreads();
    {  // slots of the dropped tracks go back to the pool: one lane clears their bits (no atomics: the state may sit in LDS)
      unsigned long long nm = nanmask, clr = 0ull;
      while (nm) {
        const int l = __ffsll((long long)nm) - 1;
        nm &= nm - 1;
        clr |= 1ull << __shfl(slot, l);
      }
      if (lane == 0) st.used &= ~clr;
    }
    // a track that leaves here is finished too: it competes for the export id like one that dies of age (its rows are in the log)
    for (unsigned long long dead = nanmask; dead; dead &= dead - 1) {
      if (lane == __ffsll((long long)dead) - 1) {
        const Trk& k = st.trk[slot];
        if (k.nrows >= 2 && (k.cum > st.best_cum || (k.cum == st.best_cum && k.id + 1 < st.best_id))) { st.best_cum = k.cum; st.best_id = k.id + 1; }
      }
      __syncthreads();
    }
    if (lane < T && !isnan_box) {
      int np_ = __popcll(keep & ((1ull << lane) - 1ull));
      st.order[np_] = slot;
      for (int i = 0; i < 4; i++) sh.tbox[np_][i] = bx[i];
    }
    T = __popcll(keep);
    if (lane == 0) st.ntrk = T;
  }
  __syncthreads();
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
  __syncthreads();
  int colsum = 0;
  if (lane < T)
    for (int d = 0; d < nd; d++) colsum += sh.iou[d][lane] > p.iou_thr ? 1 : 0;
  TRK_MARK(1);   // cost matrix
  if (lane < MAXD) sh.d2t[lane] = -1;
  __syncthreads();
  const int maxcol = wave_max_i32(colsum);
  int maxrow = 0;
  for (int d = 0; d < nd; d++) {
    unsigned long long m = __ballot(lane < T && sh.iou[d][lane] > p.iou_thr);
    maxrow = max(maxrow, __popcll(m));
  }
  int my_det = -1;  // detection matched to this lane's track
  if (nd > 0 && T > 0) {
    if (maxrow == 1 && maxcol == 1) {   // (a.sum(1).max() == 1 and a.sum(0).max() == 1: the hits are the matches)
      if (lane < T)
        for (int d = 0; d < nd; d++)
          if (sh.iou[d][lane] > p.iou_thr) my_det = d;
    } else {                            // linear assignment on -iou
      if (nd <= T) {
        lap_solve(&sh.cost[0][0], MAXT, false, nd, T, sh.r2c, sh.lap, lane);
        if (lane < T)
          for (int d = 0; d < nd; d++)
            if (sh.r2c[d] == lane) my_det = d;
      } else {
        lap_solve(&sh.cost[0][0], MAXT, true, T, nd, sh.r2c, sh.lap, lane);
        if (lane < T) my_det = sh.r2c[lane];
      }
    }
  }
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
  // ---- births: one new track per unmatched detection, in list order.  A 65th live track is not stored: the birth is counted in
  // `overflow` (vbt_tracker_status, VBT_ERR_CAPACITY at the read-backs) and nothing is written - the slot comes from the free bits of
  // `used`, of which there is at least one while ntrk < MAXT, and order[] is written at ntrk < MAXT only. ----
  const int nud = sh.n_um_d;
  if (lane == 0) {
    for (int i = 0; i < nud; i++) {
      if (st.ntrk >= MAXT) { st.overflow += 1; continue; }
      int s = __ffsll((long long)~st.used) - 1;
      st.used |= 1ull << s;
      Trk& k = st.trk[s];
      const double* dt = sh.det[sh.um_d[i]];
      double z[4];
      sort_bbox_to_z(dt, z);
      for (int j = 0; j < 7; j++) k.x[j] = j < 4 ? z[j] : 0.0;
      for (int b = 0; b < 3; b++) { k.B[b][0] = 10.0; k.B[b][1] = 0.0; k.B[b][2] = 0.0; k.B[b][3] = 10000.0; }
      k.Pr = 10.0;
      k.has_saved = 0; k.observed = 0; k.gap = 0; k.has_obs = 0; k.has_vel = 0;   // OC-SORT-only fields: set, never read
      for (int j = 0; j < 5; j++) k.last_obs[j] = -1.0;
      for (int j = 0; j < 4; j++) { k.obs_age[j] = -1; k.last_z[j] = 0.0; }
      k.vel[0] = k.vel[1] = 0.0;
      k.time_since_update = 0; k.hits = 0; k.hit_streak = 0; k.age = 0; k.nrows = 0;
      k.cum = 0.0; k.cum_c = 0.0; k.prev_x = 0.0; k.prev_y = 0.0;
      k.conf = dt[4]; k.cls = dt[5];
      k.id = st.next_id++;
      st.order[st.ntrk++] = s;
    }
  }
  __syncthreads();
  TRK_MARK(5);   // births
  // ---- emission (reverse list order) + deletion ----
  T = st.ntrk;
  bool emit = false, keep = true;
  int myslot = 0;
  if (lane < T) {
    myslot = st.order[lane];
    const Trk& k = st.trk[myslot];
    emit = k.time_since_update < 1 && (k.hit_streak >= p.min_hits || st.frame_count <= p.min_hits);
    keep = !(k.time_since_update > p.max_age);
  }
  unsigned long long em = __ballot(emit);
  const int nem = __popcll(em);
  const int base = st.nrows;
  if (emit) {
    Trk& k = st.trk[myslot];
    int ridx = lane >= 63 ? 0 : __popcll(em >> (lane + 1));  // rows of later tracks come first
    double bx[4];
    x_to_bbox(k.x, bx);   // get_state(): the posterior, whatever the observation was
    double xc = (bx[0] + bx[2]) / 2.0, yc = (bx[1] + bx[3]) / 2.0;
    if (ridx < MAXD) {
      double* lo = st.last_out[ridx];
      lo[0] = bx[0]; lo[1] = bx[1]; lo[2] = bx[2]; lo[3] = bx[3];
      lo[4] = (double)(k.id + 1); lo[5] = k.cls; lo[6] = k.conf; lo[7] = k.x[4]; lo[8] = k.x[5];
    }
    if (base + ridx < rows_cap) {
      Row r;
      r.id = k.id + 1; r.time = time; r.x = xc; r.y = yc; r.dx = k.x[4]; r.dy = k.x[5];
      r.h = fabs(bx[3] - bx[1]); r.w = fabs(bx[2] - bx[0]);
      rows[base + ridx] = r;
    }
    // running path length of this id (reference track.py:109-113: sqrt(dx^2+dy^2), cumulative per id)
    if (k.nrows > 0) {
      double ex = xc - k.prev_x, ey = yc - k.prev_y;
      double dist = sqrt(ex * ex + ey * ey);
      double yk = dist - k.cum_c;
      double tk = k.cum + yk;
      k.cum_c = (tk - k.cum) - yk;
      k.cum = tk;
    }
    k.prev_x = xc; k.prev_y = yc; k.nrows += 1;
  }
  if (lane == 0) {
    st.last_n = min(nem, MAXD);
    if (base + nem > rows_cap) { st.rows_overflow += base + nem - rows_cap; st.nrows = rows_cap; }
    else st.nrows = base + nem;
  }
  unsigned long long km = __ballot(lane < T && keep);
  if (km != (T >= 64 ? ~0ull : ((1ull << T) - 1ull))) {
    __syncthreads();
    if (lane < T && keep) st.order[__popcll(km & ((1ull << lane) - 1ull))] = myslot;
    {
      unsigned long long dm = ~km & (T >= 64 ? ~0ull : ((1ull << T) - 1ull)), clr = 0ull;
      while (dm) {
        const int l = __ffsll((long long)dm) - 1;
        dm &= dm - 1;
        clr |= 1ull << __shfl(myslot, l);
      }
      if (lane == 0) st.used &= ~clr;
    }
    // a finished track competes for the export id (max cumulative distance; ties -> lower id); the few deaths of a frame are serialised
    unsigned long long dead = ~km & (T >= 64 ? ~0ull : ((1ull << T) - 1ull));
    while (dead) {
      int l = __ffsll((long long)dead) - 1;
      dead &= dead - 1;
      if (lane == l) {
        const Trk& k = st.trk[myslot];
        if (k.nrows >= 2 && (k.cum > st.best_cum || (k.cum == st.best_cum && k.id + 1 < st.best_id))) { st.best_cum = k.cum; st.best_id = k.id + 1; }
      }
      __syncthreads();
    }
    if (lane == 0) st.ntrk = __popcll(km);
  }
  __syncthreads();
  TRK_MARK(6);   // emission + deletion
#ifdef VBT_TRK_PROF
  if (threadIdx.x == 0) { atomicAdd(&g_trk_prof[8], 1ull); atomicAdd(&g_trk_prof[9], (unsigned long long)nd); atomicAdd(&g_trk_prof[10], (unsigned long long)st.ntrk); }
#endif
}

}  // namespace vbt
