// One OCSort.update() for one clip by one wavefront: the Kalman pieces, the association costs, ocsort_step itself, the detector
// slot -> detection list loaders and the clip state's copy between global memory and LDS.  Device code, included by tracker.hip - the
// unit of the step kernels - after its TRK_T0 / TRK_MARK phase-timer macros.  All arithmetic is FP64 with contraction off in the op
// order of the numpy formulation (tracker.hip's header comment): nothing here may be reordered.
#pragma once
#include "lap.h"
#include "tracker_state.h"

namespace vbt {

// ------------------------------------------------------------------------------------------
// Kalman filter pieces (see header comment)
// ------------------------------------------------------------------------------------------
// The filter state proper as a LOCAL value: x, the three 2x2 covariance blocks and the variance of r.  predict / update work on a copy
// in registers that is loaded from the track once and stored back once: through a `Trk&` into LDS or global memory the compiler has to
// assume that every store may change what the next load reads (the detection, the observation history and the state are all plain
// double arrays), so the filter arithmetic ran as a chain of store -> wait -> load.
struct KfCore {
  double x[7];
  double B[3][4];
  double Pr;
};
__device__ __forceinline__ void core_load(KfCore& c, const Trk& k) {
#pragma unroll
  for (int i = 0; i < 7; i++) c.x[i] = k.x[i];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) c.B[i][j] = k.B[i][j];
  c.Pr = k.Pr;
}
__device__ __forceinline__ void core_store(Trk& k, const KfCore& c) {
#pragma unroll
  for (int i = 0; i < 7; i++) k.x[i] = c.x[i];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) k.B[i][j] = c.B[i][j];
  k.Pr = c.Pr;
}
__device__ __forceinline__ void kf_predict(KfCore& k, double q44, double q66) {
#pragma unroll
  for (int i = 0; i < 3; i++) k.x[i] = k.x[i] + k.x[i + 4];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    double a = k.B[i][0], b = k.B[i][1], c = k.B[i][2], d = k.B[i][3];
    double qv = i == 2 ? q66 : q44;
    k.B[i][0] = ((a + c) + (b + d)) + 1.0;
    k.B[i][1] = (b + d) + 0.0;
    k.B[i][2] = (c + d) + 0.0;
    k.B[i][3] = d + qv;
  }
  k.Pr = k.Pr + 1.0;
}

__device__ __forceinline__ void kf_update_math(KfCore& k, const double z[4]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double Rc = i == 2 ? 10.0 : 1.0;
    double a = k.B[i][0], b = k.B[i][1], c = k.B[i][2], d = k.B[i][3];
    double y = z[i] - k.x[i];
    double S = a + Rc;
    double si = 1.0 / S;
    double kp = a * si, kv = c * si;
    k.x[i] = k.x[i] + kp * y;
    k.x[i + 4] = k.x[i + 4] + kv * y;
    double omk = 1.0 - kp, nkv = 0.0 - kv;
    double M00 = omk * a, M01 = omk * b, M10 = nkv * a + c, M11 = nkv * b + d;
    double N00 = M00 * omk, N01 = M00 * nkv + M01, N10 = M10 * omk, N11 = M10 * nkv + M11;
    double KRp = kp * Rc, KRv = kv * Rc;
    k.B[i][0] = N00 + KRp * kp;
    k.B[i][1] = N01 + KRp * kv;
    k.B[i][2] = N10 + KRv * kp;
    k.B[i][3] = N11 + KRv * kv;
  }
  double y = z[3] - k.x[3];
  double S = k.Pr + 10.0;
  double si = 1.0 / S;
  double kk = k.Pr * si;
  k.x[3] = k.x[3] + kk * y;
  double omk = 1.0 - kk;
  k.Pr = (omk * k.Pr) * omk + (kk * 10.0) * kk;
}

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
__device__ inline void x_to_bbox(const double* x, double o[4]) {
  double w = sqrt(x[2] * x[3]);
  double h = x[2] / w;
  o[0] = x[0] - w / 2.0; o[1] = x[1] - h / 2.0; o[2] = x[0] + w / 2.0; o[3] = x[1] + h / 2.0;
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

__device__ inline double iou_xyxy(const double* a, const double* b) {
  double xx1 = fmax(a[0], b[0]), yy1 = fmax(a[1], b[1]), xx2 = fmin(a[2], b[2]), yy2 = fmin(a[3], b[3]);
  double w = fmax(0.0, xx2 - xx1), h = fmax(0.0, yy2 - yy1);
  double wh = w * h;
  return wh / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - wh);
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

// Linear assignment (lap_solve, lap_small and the wave reductions they use): lap.h, shared with evaluate.hip.

// ------------------------------------------------------------------------------------------
// one OCSort.update() for one clip, executed by one wavefront
// ------------------------------------------------------------------------------------------
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

__device__ void ocsort_step(ClipState& st, Row* rows, int rows_cap, StepShared& sh, int nd, double time, const TrackParams& p,
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
  unsigned long long nanmask = __ballot(isnan_box);
  if (nanmask) {  // drop trackers whose predicted box is NaN (stable compaction)
    unsigned long long keep = ~nanmask & (T >= 64 ? ~0ull : ((1ull << T) - 1ull));
    int slot = lane < T ? st.order[lane] : 0;
    double bx[4] = {0, 0, 0, 0};
    if (lane < T)
      for (int i = 0; i < 4; i++) bx[i] = sh.tbox[lane][i];
    __syncthreads();
    {  // slots of the dropped trackers go back to the pool: one lane clears their bits (no atomics: the state may sit in LDS)
      unsigned long long nm = nanmask, clr = 0ull;
      while (nm) {
        const int l = __ffsll((long long)nm) - 1;
        nm &= nm - 1;
        clr |= 1ull << __shfl(slot, l);
      }
      if (lane == 0) st.used &= ~clr;
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
  int colsum = 0;
  if (lane < T)
    for (int d = 0; d < nd; d++) colsum += sh.iou[d][lane] > p.iou_thr ? 1 : 0;
  TRK_MARK(1);   // cost matrix
  if (lane < MAXD) { sh.d2t[lane] = -1; sh.rej[lane] = 0; sh.taken[lane] = 0; }
  __syncthreads();
  const int maxcol = wave_max_i32(colsum);
  int maxrow = 0;
  for (int d = 0; d < nd; d++) {
    unsigned long long m = __ballot(lane < T && sh.iou[d][lane] > p.iou_thr);
    maxrow = max(maxrow, __popcll(m));
  }
  int my_det = -1;  // detection matched to this lane's tracker
  if (nd > 0 && T > 0) {
    if (maxrow == 1 && maxcol == 1) {
      if (lane < T)
        for (int d = 0; d < nd; d++)
          if (sh.iou[d][lane] > p.iou_thr) my_det = d;
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
  // ---- births ----
  nud = sh.n_um_d;
  if (lane == 0) {
    for (int i = 0; i < nud; i++) {
      if (st.ntrk >= MAXT) { st.overflow += 1; continue; }
      int s = __ffsll((long long)~st.used) - 1;
      st.used |= 1ull << s;
      Trk& k = st.trk[s];
      const double* dt = sh.det[sh.um_d[i]];
      double z[4];
      bbox_to_z(dt, z);
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
  TRK_MARK(5);   // update(None) + births
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
    int ridx = lane >= 63 ? 0 : __popcll(em >> (lane + 1));  // rows of later trackers come first
    double bx[4];
    if (obs_sum_negative(k)) x_to_bbox(k.x, bx);
    else { bx[0] = k.last_obs[0]; bx[1] = k.last_obs[1]; bx[2] = k.last_obs[2]; bx[3] = k.last_obs[3]; }
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
    // a finished track competes for the export id (max cumulative distance; ties -> lower id);
    // the few deaths of a frame are serialised
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

// One detector slot -> the tracker's detection list, lane i = detection i (the slot's 25 scores / boxes arrive in one
// round trip instead of 25 dependent ones by lane 0): threshold of reference odt.py:70-75 (score >= det_threshold), the
// reorder of odt.py:102-118 and OC-SORT's own gate (score > det_thresh), order kept.  Returns the number of detections
// handed to the tracker, or -1 when run_odt would have returned [] (the frame is skipped, track.py:180-181).  Uniform.
// The slot's count, this lane's score and this lane's box are requested TOGETHER (the count used to gate the score load and the score
// the box load: three dependent round trips at the head of every frame of a walk), and a walk requests frame f + 1's while it steps
// through frame f.
struct RawDet {
  int n;
  float s;
  float4 b;   // ymin,xmin,ymax,xmax
};
__device__ __forceinline__ RawDet fetch_slot_detections(const float* boxes, const float* scores, const int* counts, int slot, int lane) {
  const int l = min(lane, MAXD - 1);   // lanes past the 25 entries re-read the last one (never used)
  RawDet d;
  d.n = counts[slot];
  d.s = scores[slot * MAXD + l];
  d.b = *(const float4*)(boxes + ((size_t)slot * MAXD + l) * 4);
  return d;
}
__device__ __forceinline__ int put_slot_detections(StepShared& sh, const RawDet& d, float det_threshold, double det_thresh, int lane) {
  const int n = min(d.n, MAXD);
  const float s = lane < n ? d.s : 0.0f;
  const bool kept = lane < n && s >= det_threshold;
  const bool used = kept && (double)s > det_thresh;
  const unsigned long long mk = __ballot(kept), mu = __ballot(used);
  if (used) {
    const int m = __popcll(mu & ((1ull << lane) - 1ull));
    sh.det[m][0] = (double)d.b.y; sh.det[m][1] = (double)d.b.x; sh.det[m][2] = (double)d.b.w; sh.det[m][3] = (double)d.b.z;
    sh.det[m][4] = (double)s; sh.det[m][5] = 0.0;
  }
  return mk ? __popcll(mu) : -1;
}
__device__ inline int load_slot_detections(StepShared& sh, const float* boxes, const float* scores, const int* counts, int slot,
                                           float det_threshold, double det_thresh, int lane) {
  return put_slot_detections(sh, fetch_slot_detections(boxes, scores, counts, slot, lane), det_threshold, det_thresh, lane);
}

__device__ inline void copy_words(void* dst, const void* src, int bytes, int lane) {   // 8-byte words, one wavefront
  unsigned long long* d = (unsigned long long*)dst;
  const unsigned long long* s_ = (const unsigned long long*)src;
  for (int i = lane; i < bytes / 8; i += 64) d[i] = s_[i];
}
static_assert(sizeof(Trk) % 8 == 0 && offsetof(ClipState, trk) % 8 == 0, "8-byte copy granularity");
// The clip state between global memory and its LDS copy, by one wavefront: the header, then the LIVE tracks only.  All loads of a pass
// are in flight together (the header in one round trip, the tracks four words per lane at a time): the per-track loop it replaces
// waited for every 512 bytes - 5.8 us for ten tracks - which only a long run could amortise.  slots = 64 ints of LDS scratch.
template <bool TO_LDS>
__device__ inline void clip_state_copy(ClipState* lst, ClipState* gst, int* slots, int lane) {
  constexpr int HW = (int)(offsetof(ClipState, trk) / 8), HI = (HW + 63) / 64, TW = (int)(sizeof(Trk) / 8);
  unsigned long long* l = (unsigned long long*)lst;
  unsigned long long* g = (unsigned long long*)gst;
  {
    unsigned long long hv[HI];
#pragma unroll
    for (int k = 0; k < HI; k++) { const int i = min(lane + 64 * k, HW - 1); hv[k] = TO_LDS ? g[i] : l[i]; }
#pragma unroll
    for (int k = 0; k < HI; k++) { const int i = lane + 64 * k; if (i < HW) (TO_LDS ? l : g)[i] = hv[k]; }
  }
  __syncthreads();
  const unsigned long long used = lst->used;
  if ((used >> lane) & 1ull) slots[__popcll(used & ((1ull << lane) - 1ull))] = lane;
  __syncthreads();
  const int total = __popcll(used) * TW;
  unsigned long long* lt = (unsigned long long*)&lst->trk[0];
  unsigned long long* gt = (unsigned long long*)&gst->trk[0];
  for (int base = 0; base < total; base += 256) {
    unsigned long long v[4];
    int off[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int i = min(base + lane + 64 * k, total - 1);
      const int ord = i / TW, w = i - ord * TW;
      off[k] = slots[ord] * TW + w;
      v[k] = TO_LDS ? gt[off[k]] : lt[off[k]];
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (base + lane + 64 * k < total) (TO_LDS ? lt : gt)[off[k]] = v[k];
  }
  __syncthreads();
}

}  // namespace vbt
