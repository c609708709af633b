// The phases that one update() of either tracker - ocsort_step.h, sort_step.h - is made of, each written once: predict with the NaN
// drop, gate + assignment, births, emission + deletion, and the two list helpers under them.  Execution model of both steps: ONE
// wavefront per clip (the workgroup is that wavefront, so a ballot or a shuffle sees every lane), lane t = live track t = slot
// st.order[t], FP64 with contraction off.  Every phase is called by ALL 64 lanes with wave-uniform arguments and ends on the barrier it
// states, after which its writes to the clip state (global memory or LDS) and to StepShared are visible to every lane.  Device code,
// included by tracker.hip after its phase timer (TrkClock, TRK_T0 / TRK_MARK).
#pragma once
#include "box_filter.h"
#include "lap.h"

namespace vbt {

struct StepShared {
  double det[MAXD][6];
  double tbox[MAXT][4];
  double tq[MAXT][5];  // per tracker: previous-observation centre (x, y), its validity, velocity direction (x, y)
  double iou[MAXD][MAXT];
  double cost[MAXD][MAXT];
  int d2t[MAXD];      // detection -> tracker position paired by the first association (or -1)
  int rej[MAXD];      // that pair was rejected (IoU below threshold)
  int taken[MAXD];    // detection consumed by a tracker (first or second association)
  int r2c[MAXT];      // assignment scratch
  int um_d[MAXD];     // unmatched detections, in the reference's list order
  int um_t[MAXT];
  int n_um_d, n_um_t, flag;
  LapShared lap;
};

// lanes of the T live tracks (T <= MAXT = 64: a shift by 64 is not defined)
__device__ __forceinline__ unsigned long long live_mask(int T) { return T >= 64 ? ~0ull : ((1ull << T) - 1ull); }

// The tracks on the lanes of `dead` leave the clip: their slots go back to the pool and - compete - each enters the export id's
// competition, the few deaths of a frame one after the other with a barrier behind each.
// Entry: `dead` is uniform and within live_mask(T); slot = this lane's st.order[lane] (0 on lanes >= T: never selected); the lanes'
// earlier writes to their tracks are behind a barrier.  Exit: st.used is cleared by lane 0 alone, without atomics (the state may sit in
// LDS); best_cum / best_id are final behind the last barrier (compete only).  st.order and st.ntrk are the caller's.
__device__ __forceinline__ void retire(ClipState& st, unsigned long long dead, int slot, int lane, bool compete) {
  unsigned long long clr = 0ull;
  for (unsigned long long m = dead; m; m &= m - 1) clr |= 1ull << __shfl(slot, __ffsll((long long)m) - 1);   // slot < MAXT = the 64 bits of `used`
  if (lane == 0) st.used &= ~clr;
  if (!compete) return;
  for (unsigned long long m = dead; m; m &= m - 1) {
    if (lane == __ffsll((long long)m) - 1) finished_track_competes(st, st.trk[slot]);
    __syncthreads();
  }
}

// ---- predict (KalmanBoxTracker.predict of both packages) + removal of the tracks whose predicted box holds a NaN (stable compaction:
// np.ma.compress_rows(np.ma.masked_invalid(trks)) + pop).  A detection of zero height gets here one frame after its birth under SORT's
// r = w / h: r = inf, s = 0, w = sqrt(0 * inf) = NaN.  NAN_COMPETES: a track dropped here competes for the export id like one that dies of
// age - SORT yes, OC-SORT no (DESIGN.md section 9 on why the two are left different).
// Entry: st.ntrk tracks in st.order, the previous step's barrier passed.  Exit, behind a barrier: every live track predicted and aged,
// sh.tbox[t] = predicted box of list position t, st.order / st.ntrk / st.used without the dropped tracks; returns the new track count.
// Bounds: only lanes < T write, to positions popcount(keep below lane) < popcount(keep) <= T <= MAXT of order[] / tbox[].
template <bool NAN_COMPETES>
__device__ __forceinline__ int predict_and_drop_nan(ClipState& st, StepShared& sh, double q44, double q66, int lane) {
  int T = st.ntrk;
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
  unsigned long long nanmask = __ballot(isnan_box);
  if (nanmask) {
    unsigned long long keep = ~nanmask & live_mask(T);
    int slot = lane < T ? st.order[lane] : 0;
    double bx[4] = {0, 0, 0, 0};
    if (lane < T)
      for (int i = 0; i < 4; i++) bx[i] = sh.tbox[lane][i];
    __syncthreads();
    retire(st, nanmask, slot, lane, NAN_COMPETES);
    if (lane < T && !isnan_box) {
      int np_ = __popcll(keep & ((1ull << lane) - 1ull));
      st.order[np_] = slot;
      for (int i = 0; i < 4; i++) sh.tbox[np_][i] = bx[i];
    }
    T = __popcll(keep);
    if (lane == 0) st.ntrk = T;
  }
  __syncthreads();
  return T;
}

// ---- gate + assignment: the detection paired with this lane's track (-1: none; lanes >= T: -1).  When every row and column of
// iou > thr holds at most one hit and there is one (a.sum(1).max() == 1 and a.sum(0).max() == 1), the hits are the pairs; else the
// linear assignment on sh.cost, rows = the shorter side.  A pair below the threshold is still returned: undoing it is the caller's.
// Entry, behind a barrier: sh.iou[d][t], sh.cost[d][t] for d < nd <= MAXD, t < T <= MAXT, and the caller's pairing arrays (d2t, ...)
// reset.  Exit: no barrier after the solver's own; the result is per lane, sh.r2c and sh.lap are scratch.  TRK_MARK(1) - the end of the
// cost matrix, per-track gate count included - sits inside, which is why the step's clock comes along.
__device__ __forceinline__ int gate_and_assign(StepShared& sh, int nd, int T, double iou_thr, int lane, TrkClock& _tp) {
  int colsum = 0;
  if (lane < T)
    for (int d = 0; d < nd; d++) colsum += sh.iou[d][lane] > iou_thr ? 1 : 0;
  TRK_MARK(1);   // cost matrix
  __syncthreads();
  const int maxcol = wave_max_i32(colsum);
  int maxrow = 0;
  for (int d = 0; d < nd; d++) {
    unsigned long long m = __ballot(lane < T && sh.iou[d][lane] > iou_thr);
    maxrow = max(maxrow, __popcll(m));
  }
  int my_det = -1;
  if (nd > 0 && T > 0) {
    if (maxrow == 1 && maxcol == 1) {
      if (lane < T)
        for (int d = 0; d < nd; d++)
          if (sh.iou[d][lane] > iou_thr) my_det = d;
    } else {
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
  return my_det;
}

// ---- births: one new track per unmatched detection, in list order, by lane 0.  TO_Z: the package's convert_bbox_to_z.  A 65th live
// track is not stored: the birth is counted in `overflow` (vbt_tracker_status, VBT_ERR_CAPACITY at the read-backs) and nothing is
// written - the slot comes from the free bits of `used`, of which there is at least one while ntrk < MAXT, and order[] is written at
// ntrk < MAXT only.  The fields only OC-SORT reads are set for both.
// Entry, behind a barrier: sh.um_d[0 .. sh.n_um_d) = the detections to start tracks from (n_um_d <= MAXD), every update of this frame
// done.  Exit, behind a barrier: the new tracks at the end of st.order, st.ntrk / st.used / st.next_id / st.overflow advanced.
template <void (*TO_Z)(const double*, double*)>
__device__ __forceinline__ void births(ClipState& st, StepShared& sh, int lane) {
  const int nud = sh.n_um_d;
  if (lane == 0) {
    for (int i = 0; i < nud; i++) {
      if (st.ntrk >= MAXT) { st.overflow += 1; continue; }
      int s = __ffsll((long long)~st.used) - 1;
      st.used |= 1ull << s;
      Trk& k = st.trk[s];
      const double* dt = sh.det[sh.um_d[i]];
      double z[4];
      TO_Z(dt, z);
      for (int j = 0; j < 7; j++) k.x[j] = j < 4 ? z[j] : 0.0;
      for (int b = 0; b < 3; b++) { k.B[b][0] = 10.0; k.B[b][1] = 0.0; k.B[b][2] = 0.0; k.B[b][3] = 10000.0; }
      k.Pr = 10.0;
      k.has_saved = 0; k.observed = 0; k.gap = 0; k.has_obs = 0; k.has_vel = 0;
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
}

// ---- emission (reverse list order) + deletion by age.  ROW_BOX: the box a track is emitted as (OC-SORT: the last observation; SORT: the
// posterior); everything behind the box is one text.  A row past rows_cap is counted in rows_overflow and not written; last_out keeps
// the first MAXD boxes of the frame.  A deleted track leaves through retire and competes for the export id.
// Entry, behind a barrier: the frame's updates and births done.  Exit, behind a barrier: rows[st.nrows ...) and st.last_out / last_n
// written, every emitted track's path length advanced, st.order / st.ntrk / st.used without the tracks older than p.max_age.
template <void (*ROW_BOX)(const Trk&, double*)>
__device__ __forceinline__ void emit_and_delete(ClipState& st, Row* rows, int rows_cap, double time, const TrackParams& p, int lane) {
  const int T = st.ntrk;
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
    int ridx = lane >= 63 ? 0 : __popcll(em >> (lane + 1));  // rows of later trackers come first
    double bx[4];
    ROW_BOX(k, bx);
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
  if (km != live_mask(T)) {
    __syncthreads();
    if (lane < T && keep) st.order[__popcll(km & ((1ull << lane) - 1ull))] = myslot;
    retire(st, ~km & live_mask(T), myslot, lane, true);
    if (lane == 0) st.ntrk = __popcll(km);
  }
  __syncthreads();
}

}  // namespace vbt
