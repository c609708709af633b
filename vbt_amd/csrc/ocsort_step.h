// One OCSort.update() for one clip by one wavefront: what is OC-SORT's own - the Kalman update with its freeze / unfreeze, the direction
// term of the first association, the unmatched lists, the second association on the last observations, update(None), the box a row is
// emitted as - and ocsort_step, which runs them between the phases it shares with sort_step (step_phases.h: predict_and_drop_nan,
// gate_and_assign, births, emit_and_delete).  Device code, included by tracker.hip.  All arithmetic is FP64 with contraction off in the
// op order of the numpy formulation (tracker.hip's header comment): nothing here may be reordered.
#pragma once
#include "step_phases.h"

namespace vbt {

// kf.update(z) with OC-SORT's freeze / unfreeze (observation-centric re-update); c = the track's filter state (registers)
__device__ inline void kf_update(Trk& k, KfCore& c, const double* z, double q44, double q66) {
  k.gap += 1;  // one more entry in history_obs since the last real observation
  if (z == nullptr) {
    if (k.observed) {  // first miss: freeze
#pragma unroll
      for (int i = 0; i < 7; i++) k.sx[i] = c.x[i];
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) k.sB[i][j] = c.B[i][j];
      k.sPr = c.Pr;
      k.has_saved = 1;
    }
    k.observed = 0;
    return;
  }
  double zl[4] = {z[0], z[1], z[2], z[3]};
  if (!k.observed && k.has_saved) {  // unfreeze: replay a linear virtual trajectory over the gap
#pragma unroll
    for (int i = 0; i < 7; i++) c.x[i] = k.sx[i];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) c.B[i][j] = k.sB[i][j];
    c.Pr = k.sPr;
    double x1 = k.last_z[0], y1 = k.last_z[1], s1 = k.last_z[2], r1 = k.last_z[3];
    double w1 = sqrt(s1 * r1), h1 = sqrt(s1 / r1);
    double x2 = z[0], y2 = z[1], s2 = z[2], r2 = z[3];
    double w2 = sqrt(s2 * r2), h2 = sqrt(s2 / r2);
    const int gap = k.gap;
    const double g = (double)gap;
    double dx = (x2 - x1) / g, dy = (y2 - y1) / g, dw = (w2 - w1) / g, dh = (h2 - h1) / g;
    for (int i = 0; i < gap; i++) {
      double f = (double)(i + 1);
      double xx = x1 + f * dx, yy = y1 + f * dy, ww = w1 + f * dw, hh = h1 + f * dh;
      double vz[4] = {xx, yy, ww * hh, ww / hh};
      kf_update_math(c, vz);
      if (i != gap - 1) kf_predict(c, q44, q66);
      else { zl[0] = vz[0]; zl[1] = vz[1]; zl[2] = vz[2]; zl[3] = vz[3]; }  // history ends with the virtual box
    }
    k.has_saved = 0;
  }
  k.observed = 1;
  kf_update_math(c, z);
  k.last_z[0] = zl[0]; k.last_z[1] = zl[1]; k.last_z[2] = zl[2]; k.last_z[3] = zl[3];
  k.gap = 0;
}

__device__ inline void bbox_to_z(const double* b, double z[4]) {
  double w = b[2] - b[0], h = b[3] - b[1];
  z[0] = b[0] + w / 2.0;
  z[1] = b[1] + h / 2.0;
  z[2] = w * h;
  z[3] = w / (h + 1e-6);
}

// `last_observation.sum() < 0` is how OC-SORT asks "no observation yet" (placeholder = five -1s); it
// also fires for a real box far enough outside the image, and that quirk is kept.
__device__ inline bool obs_sum_negative(const Trk& k) {
  double s = k.last_obs[0];
  s = s + k.last_obs[1]; s = s + k.last_obs[2]; s = s + k.last_obs[3]; s = s + k.last_obs[4];
  return s < 0.0;
}

// KalmanBoxTracker.update(bbox)   (bbox = x1,y1,x2,y2,score ; cls)
__device__ inline void trk_update(Trk& k, const double* det_in, double q44, double q66, int delta_t) {
  KfCore c;
  core_load(c, k);
  if (det_in == nullptr) { kf_update(k, c, nullptr, q44, q66); return; }     // (update(None) leaves the filter state as it is)
  const double det[6] = {det_in[0], det_in[1], det_in[2], det_in[3], det_in[4], det_in[5]};   // in registers before the first store
  k.conf = det[4];
  k.cls = det[5];
  if (!obs_sum_negative(k)) {
    const double* prev = nullptr;
    for (int i = 0; i < delta_t; i++) {
      int a = k.age - (delta_t - i);
      if (a >= 0 && k.obs_age[a & 3] == a) { prev = k.obs[a & 3]; break; }
    }
    if (!prev) prev = k.last_obs;
    const double p0 = prev[0], p1 = prev[1], p2 = prev[2], p3 = prev[3];
    double cx1 = (p0 + p2) / 2.0, cy1 = (p1 + p3) / 2.0;
    double cx2 = (det[0] + det[2]) / 2.0, cy2 = (det[1] + det[3]) / 2.0;
    double sy = cy2 - cy1, sx = cx2 - cx1;
    double norm = sqrt(sy * sy + sx * sx) + 1e-6;
    k.vel[0] = sy / norm;
    k.vel[1] = sx / norm;
    k.has_vel = 1;
  }
#pragma unroll
  for (int i = 0; i < 5; i++) { k.last_obs[i] = det[i]; k.obs[k.age & 3][i] = det[i]; }
  k.obs_age[k.age & 3] = k.age;
  k.has_obs = 1;
  k.time_since_update = 0;
  k.hits += 1;
  k.hit_streak += 1;
  double z[4];
  bbox_to_z(det, z);
  kf_update(k, c, z, q44, q66);
  core_store(k, c);
}

__device__ inline double diou_xyxy(const double* a, const double* b) {
  double iou = iou_xyxy(a, b);
  double cx1 = (a[0] + a[2]) / 2.0, cy1 = (a[1] + a[3]) / 2.0, cx2 = (b[0] + b[2]) / 2.0, cy2 = (b[1] + b[3]) / 2.0;
  double ex = cx1 - cx2, ey = cy1 - cy2;
  double inner = ex * ex + ey * ey;
  double xc1 = fmin(a[0], b[0]), yc1 = fmin(a[1], b[1]), xc2 = fmax(a[2], b[2]), yc2 = fmax(a[3], b[3]);
  double ox = xc2 - xc1, oy = yc2 - yc1;
  double outer = ox * ox + oy * oy;
  return (iou - inner / outer + 1.0) / 2.0;
}

// the box of a row: the last observation, or the filter's box while there is none
__device__ inline void ocsort_row_box(const Trk& k, double bx[4]) {
  if (obs_sum_negative(k)) x_to_bbox(k.x, bx);
  else { bx[0] = k.last_obs[0]; bx[1] = k.last_obs[1]; bx[2] = k.last_obs[2]; bx[3] = k.last_obs[3]; }
}

__device__ void ocsort_step(ClipState& st, Row* rows, int rows_cap, StepShared& sh, int nd, double time, const TrackParams& p,
                            double q44, double q66, int lane) {
  TRK_T0();
  if (lane == 0) st.frame_count += 1;
  const int T = predict_and_drop_nan<false>(st, sh, q44, q66, lane);
  const int slot = lane < T ? st.order[lane] : 0;
  TRK_MARK(0);   // predict
  // ---- first association: IoU + velocity-direction consistency ----
  // Per-tracker quantities by lane = tracker, then the (detection, tracker) cost entries dealt to the 64 lanes pair by pair:
  // every entry is the same sequence of double operations as before, but a frame with 20 detections and 3 trackers is one
  // pass of 60 lanes instead of 20 dependent passes of 3 (sqrt / acos in double dominate the step).
  if (lane < T) {
    Trk& k = st.trk[slot];
    const double* pobs = nullptr;  // k_previous_obs
    if (k.has_obs) {
      for (int i = 0; i < p.delta_t; i++) {
        int a = k.age - (p.delta_t - i);
        if (a >= 0 && k.obs_age[a & 3] == a) { pobs = k.obs[a & 3]; break; }
      }
      if (!pobs) pobs = k.last_obs;
    }
    double pcx = -1.0, pcy = -1.0, valid = 0.0;
    if (pobs) { pcx = (pobs[0] + pobs[2]) / 2.0; pcy = (pobs[1] + pobs[3]) / 2.0; valid = pobs[4] < 0.0 ? 0.0 : 1.0; }
    sh.tq[lane][0] = pcx; sh.tq[lane][1] = pcy; sh.tq[lane][2] = valid;
    sh.tq[lane][3] = k.has_vel ? k.vel[1] : 0.0;   // vx
    sh.tq[lane][4] = k.has_vel ? k.vel[0] : 0.0;   // vy
  }
  if (lane < MAXD) { sh.d2t[lane] = -1; sh.rej[lane] = 0; sh.taken[lane] = 0; }   // this frame's pairing arrays (their last readers: behind the previous step's barrier)
  __syncthreads();
  {
    const double PI = 3.141592653589793;
    const int npairs = nd * T;
    for (int p0 = 0; p0 < npairs; p0 += 64) {
      const int pr = p0 + lane;
      if (pr < npairs) {
        const int d = pr / T, t = pr - d * T;
        const double* dt = sh.det[d];
        const double pcx = sh.tq[t][0], pcy = sh.tq[t][1], valid = sh.tq[t][2], vx = sh.tq[t][3], vy = sh.tq[t][4];
        double io = iou_xyxy(dt, sh.tbox[t]);
        double dx = (dt[0] + dt[2]) / 2.0 - pcx, dy = (dt[1] + dt[3]) / 2.0 - pcy;
        double norm = sqrt(dx * dx + dy * dy) + 1e-6;
        double X = dx / norm, Y = dy / norm;
        double c = vx * X + vy * Y;
        c = fmin(fmax(c, -1.0), 1.0);
        double ang = (PI / 2.0 - fabs(acos(c))) / PI;
        double ac = ((valid * ang) * p.inertia) * dt[4];
        sh.iou[d][t] = io;
        sh.cost[d][t] = -(io + ac);
      }
    }
  }
  __syncthreads();
  int my_det = gate_and_assign(sh, nd, T, p.iou_thr, lane, _tp);   // detection matched to this lane's tracker
  TRK_MARK(2);   // assignment
  // d2t[d]: tracker position the solver paired with detection d (-1 none); rej[d]: pair rejected (IoU < thr)
  const bool was_paired = lane < T && my_det >= 0;   // the solver paired this lane's tracker with a detection (accepted or not)
  if (was_paired) {
    sh.d2t[my_det] = lane;
    if (sh.iou[my_det][lane] < p.iou_thr) { sh.rej[my_det] = 1; my_det = -1; }
  }
  __syncthreads();
  if (lane < T && my_det >= 0) trk_update(st.trk[slot], sh.det[my_det], q44, q66, p.delta_t);
  TRK_MARK(11);  // matched Kalman updates
  // unmatched lists in the reference's order (it matters: the second association sees exact ties):
  //   detections: never paired ascending, then rejected pairs in matched (= detection) order
  //   trackers  : never paired ascending, then the trackers of the rejected pairs in the same order
  // lane = detection for the detection list and the rejected pairs, lane = tracker for the never-paired trackers: positions are
  // population counts of ballots (the lists used to be walked by lane 0, one dependent LDS round trip per element)
  {
    const unsigned long long below = (1ull << lane) - 1ull;
    const int dt_ = lane < nd ? sh.d2t[lane] : 0;
    const bool un_d = lane < nd && dt_ < 0, rj_d = lane < nd && dt_ >= 0 && sh.rej[lane] != 0;
    const unsigned long long mU = __ballot(un_d), mR = __ballot(rj_d), mT = __ballot(lane < T && !was_paired);
    const int nU = __popcll(mU), nR = __popcll(mR), nT = __popcll(mT);
    if (un_d) sh.um_d[__popcll(mU & below)] = lane;
    if (rj_d) { const int q = __popcll(mR & below); sh.um_d[nU + q] = lane; sh.um_t[nT + q] = dt_; }
    if (lane < T && !was_paired) sh.um_t[__popcll(mT & below)] = lane;
    if (lane == 0) { sh.n_um_d = nU + nR; sh.n_um_t = nT + nR; }
  }
  __syncthreads();
  TRK_MARK(3);   // matched updates + unmatched lists
  // ---- observation-centric recovery (second association on the last observations) ----
  int nud = sh.n_um_d, nut = sh.n_um_t;
  bool recovered = false;
  if (nud > 0 && nut > 0) {
    double mx = -1e300;
    for (int p0 = 0; p0 < nud * nut; p0 += 64) {   // (unmatched detection, unmatched tracker) pairs dealt to the lanes
      const int pr = p0 + lane;
      if (pr < nud * nut) {
        const int i = pr / nut, j = pr - i * nut;
        const Trk& k = st.trk[st.order[sh.um_t[j]]];
        double lb[4];
        for (int q = 0; q < 4; q++) lb[q] = k.last_obs[q];
        const double* dt = sh.det[sh.um_d[i]];
        double v = p.asso == 1 ? diou_xyxy(dt, lb) : iou_xyxy(dt, lb);
        sh.iou[i][j] = v;
        sh.cost[i][j] = -v;
        mx = fmax(mx, v);
      }
    }
    mx = wave_max_f64(mx);
    __syncthreads();
    TRK_MARK(12);  // second association: cost entries
    if (mx > p.iou_thr) {
      int mine = -1;  // index into um_d matched to um_t[lane]
      if (nud <= nut) {
        lap_solve(&sh.cost[0][0], MAXT, false, nud, nut, sh.r2c, sh.lap, lane);
        if (lane < nut)
          for (int i = 0; i < nud; i++)
            if (sh.r2c[i] == lane) mine = i;
      } else {
        lap_solve(&sh.cost[0][0], MAXT, true, nut, nud, sh.r2c, sh.lap, lane);
        if (lane < nut) mine = sh.r2c[lane];
      }
      TRK_MARK(13);  // second association: assignment
      if (lane < nut && mine >= 0 && !(sh.iou[mine][lane] < p.iou_thr)) {
        int tp = sh.um_t[lane];
        trk_update(st.trk[st.order[tp]], sh.det[sh.um_d[mine]], q44, q66, p.delta_t);
        sh.taken[sh.um_d[mine]] = 1;
        sh.um_t[lane] = -1;
      }
      recovered = true;
      __syncthreads();
      TRK_MARK(14);  // second association: recovered tracks' Kalman updates (incl. the re-update over the gap)
      {  // np.setdiff1d: sorted ascending (lane = detection)
        const bool left = lane < nd && (sh.d2t[lane] < 0 || sh.rej[lane] != 0) && !sh.taken[lane];
        const unsigned long long mL = __ballot(left);
        __syncthreads();     // every lane has read the old list entries it needs (um_d is rewritten in place)
        if (left) sh.um_d[__popcll(mL & ((1ull << lane) - 1ull))] = lane;
        if (lane == 0) sh.n_um_d = __popcll(mL);
      }
      __syncthreads();
    }
  }
  (void)recovered;
  TRK_MARK(4);   // second association
  // ---- unmatched trackers: update(None) ----
  if (lane < nut && sh.um_t[lane] >= 0) trk_update(st.trk[st.order[sh.um_t[lane]]], nullptr, q44, q66, p.delta_t);
  __syncthreads();
  births<bbox_to_z>(st, sh, lane);
  TRK_MARK(5);   // update(None) + births
  emit_and_delete<ocsort_row_box>(st, rows, rows_cap, time, p, lane);
  TRK_MARK(6);   // emission + deletion
#ifdef VBT_TRK_PROF
  if (threadIdx.x == 0) { atomicAdd(&g_trk_prof[8], 1ull); atomicAdd(&g_trk_prof[9], (unsigned long long)nd); atomicAdd(&g_trk_prof[10], (unsigned long long)st.ntrk); }
#endif
}

}  // namespace vbt
