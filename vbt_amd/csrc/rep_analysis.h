// Rep analysis of one track's rows: pandas' rolling / expanding means (reference plot.py:87-95) and the VelocityTracker scan
// (VelocityTracker.py:30-230).  vt_row is the ONE per-row step of the close-time scan (analyze_track, tracker_analysis.hip) and of the
// live analysis (tracker_live.hip).  Device code and plain structs.
#pragma once
#include <hip/hip_runtime.h>

#include "roll_mean.h"   // RollMean: pandas roll_mean state (Kahan add / remove)
#include "tracker_state.h"

namespace vbt {

struct VtParams {
  double plate_diameter, diff_threshold, min_distance;
  int preprocess, flush;
};

struct VtState {  // reference VelocityTracker.py:30-48
  int phase, neg, pos, nph, n, has_prev, has_max;
  double y_prev, max_y_diff;
  // the single RunningAverage(30) fed width then height (VelocityTracker.py:44-45,98-99)
  double win[30];
  int whead, wcount;
  double wtotal;
  int ver;   // bumped whenever the phase list changes (an append, or a filter that drops phases)
  int full;  // a capacity was hit: 1 = the open phase's path, 2 = the phase list (the state is not the reference's any more)
};

// The open phase's bar path (VelocityTracker.xs / ys / widths / heights / times), room for `cap` samples per column
struct VtPath {
  double *xs, *ys, *ws, *hs, *ts;
  int cap;
};

// The phase list a scan appends to: ph holds room for `cap` phases of 6 doubles; pm, when rep metrics are enabled, for their `cap`
// records of VT_METRICS doubles.  The scan's functions are templates on M, metrics formed or not: with M = false pm is never read and
// the code is the scan as it is without metrics, instruction for instruction; with M = true pm is not null.
constexpr int VT_METRICS = 8;   // = VBT_REP_METRICS; columns VBT_RM_* (include/vbt_hip.h)
struct VtPhases {
  double *ph, *pm;
  int cap;
};

__device__ inline void vt_init(VtState& s) {
  s.phase = 2; s.neg = 0; s.pos = 0; s.nph = 0; s.n = 0; s.has_prev = 0; s.has_max = 0; s.y_prev = 0; s.max_y_diff = 0;
  s.whead = 0; s.wcount = 0; s.wtotal = 0.0; s.ver = 0; s.full = 0;
}

__device__ inline double ra_update(VtState& s, double v) {  // reference RunningAverage.py:16-27
  s.win[(s.whead + s.wcount) % 30] = v;
  s.wcount += 1;
  s.wtotal += v;
  if (s.wcount >= 30) {
    double avg = s.wtotal / 30.0;
    s.wtotal -= s.win[s.whead];
    s.whead = (s.whead + 1) % 30;
    s.wcount -= 1;
    return avg;
  }
  return s.wtotal / (double)s.wcount;
}

template <bool M>
__device__ inline void vt_filter(VtState& s, const VtPhases& l) {  // VelocityTracker.py:50-67
  double *ph = l.ph, *pm = l.pm;
  double thr = s.max_y_diff / 2;
  int o = 0;
  for (int i = 0; i < s.nph; i++) {
    double yd = fabs(ph[i * 6 + 2] - ph[i * 6 + 3]);
    if (!(yd < thr)) {
      if (o != i) {
        for (int j = 0; j < 6; j++) ph[o * 6 + j] = ph[i * 6 + j];
        if (M) for (int j = 0; j < VT_METRICS; j++) pm[o * VT_METRICS + j] = pm[i * VT_METRICS + j];   // the record travels with its phase
      }
      o++;
    }
  }
  if (o != s.nph) s.ver += 1;
  s.nph = o;
}

// The rep metrics of the phase just appended ("Rep metrics"): one more pass over the steps st+1 .. en that `rom`
// was summed over, in index order, every per-step term the expression of vt_end_phase.  m[VT_METRICS].
__device__ inline void vt_phase_metrics(const VtParams& p, const VtPath& q, int st, int en, double rom, double* m) {
  const double *xs = q.xs, *ys = q.ys, *ws = q.ws, *hs = q.hs, *ts = q.ts;
  double pv = 0.0, t_pv = ts[st], rom_y = 0.0, rom_x = 0.0, pv_y = 0.0, x_dev = 0.0;
  for (int i = st + 1; i < en + 1; i++) {
    double ddx = fabs(xs[i] - xs[i - 1]) / ((ws[i] + ws[i - 1]) / 2) * p.plate_diameter;
    double ddy = fabs(ys[i] - ys[i - 1]) / ((hs[i] + hs[i - 1]) / 2) * p.plate_diameter;
    rom_x += ddx;
    rom_y += ddy;
    double dt = ts[i] - ts[i - 1];
    if (dt > 0) {   // (a tracker's log cannot hold two rows of one time stamp; rows handed to vbt_analyze_metrics can)
      double v = (ddx + ddy) / dt, vy = ddy / dt;
      if (v > pv) { pv = v; t_pv = ts[i]; }
      if (vy > pv_y) pv_y = vy;
    }
    double dev = fabs(xs[i] - xs[st]) / ((ws[i] + ws[st]) / 2) * p.plate_diameter;
    if (dev > x_dev) x_dev = dev;
  }
  double dur = ts[en] - ts[st];
  m[0] = pv; m[1] = t_pv; m[2] = rom_y; m[3] = rom_x; m[4] = pv_y;
  m[5] = dur > 0 ? rom / dur : 0.0;   // the reference's ACV (plot.py:173)
  m[6] = x_dev;
  m[7] = en > st ? (double)(en - st) : 0.0;
}

template <bool M>
__device__ inline void vt_end_phase(VtState& s, const VtParams& p, const VtPath& q, const VtPhases& l) {  // VelocityTracker.py:171-222
  double* ph = l.ph;
  const double *xs = q.xs, *ys = q.ys, *ws = q.ws, *hs = q.hs, *ts = q.ts;
  int imax = 0, imin = 0;
  for (int i = 1; i < s.n; i++) {
    if (ys[i] > ys[imax]) imax = i;
    if (ys[i] < ys[imin]) imin = i;
  }
  int st = s.phase == 0 ? imax : imin, en = s.phase == 0 ? imin : imax;
  double y_diff = fabs(ys[st] - ys[en]);
  if (!s.has_max || y_diff > s.max_y_diff) {
    s.max_y_diff = y_diff;
    s.has_max = 1;
    vt_filter<M>(s, l);
  }
  if (y_diff > s.max_y_diff * p.diff_threshold) {
    double distance = 0.0;
    for (int i = st + 1; i < en + 1; i++) {
      double ddx = fabs(xs[i] - xs[i - 1]) / ((ws[i] + ws[i - 1]) / 2) * p.plate_diameter;
      double ddy = fabs(ys[i] - ys[i - 1]) / ((hs[i] + hs[i - 1]) / 2) * p.plate_diameter;
      distance += ddx + ddy;
    }
    if (distance < p.min_distance) {
      s.neg = 0; s.pos = 0; s.phase = 2;
      return;
    }
    if (s.nph < l.cap) {
      double* o = ph + s.nph * 6;
      o[0] = ts[st]; o[1] = ts[en]; o[2] = ys[st]; o[3] = ys[en]; o[4] = distance; o[5] = (double)s.phase;
      if (M) vt_phase_metrics(p, q, st, en, distance, l.pm + s.nph * VT_METRICS);
      s.nph += 1;
      s.ver += 1;
    } else {
      s.full |= 2;
    }
    vt_filter<M>(s, l);
  }
  s.phase = 2;
  s.pos = 0; s.neg = 0;
}

__device__ inline void vt_push(VtState& s, const VtPath& q, double x, double y, double w, double h, double t) {
  if (s.n < q.cap) { q.xs[s.n] = x; q.ys[s.n] = y; q.ws[s.n] = w; q.hs[s.n] = h; q.ts[s.n] = t; s.n++; }
  else s.full |= 1;
}

// ONE row of one track - the per-row step shared by the close-time scan (analyze_track) and the live analysis
// (live_analyze_kernel), so that the two cannot drift apart.  r = time,x,y,dx,dy,h,w.  p.preprocess: plot.py:90-95 first, with
// rm = the rolling(5) x / y and expanding h / w means and (drop_x, drop_y) the raw values leaving the window (drop: row >= 5).
template <bool M>
__device__ inline void vt_row(VtState& s, RollMean* rm, const VtParams& p, const double* r, bool drop, double drop_x, double drop_y,
                              const VtPath& q, const VtPhases& l) {
  double time = r[0], x = r[1], y = r[2], h = r[5], w = r[6];
  if (p.preprocess) {  // (dx, dy columns are smoothed there too but never used downstream)
    if (drop) { rm[0].remove(drop_x); rm[1].remove(drop_y); }
    rm[0].add(x); rm[1].add(y); rm[2].add(h); rm[3].add(w);
    x = rm[0].mean(); y = rm[1].mean(); h = rm[2].mean(); w = rm[3].mean();
  }
  // VelocityTracker.process_measurements (VelocityTracker.py:92-158)
  double width = ra_update(s, w);
  double height = ra_update(s, h);
  double dy = r[4];
  if (s.has_prev) dy = y - s.y_prev;
  else if (p.preprocess) dy = r[4];  // first sample: the (smoothed == raw) incoming dy
  if (s.phase != 2) vt_push(s, q, x, y, width, height, time);
  if (s.phase == 0) {
    if (dy > 0) { s.pos += 1; s.neg = 0; if (s.pos >= 1) vt_end_phase<M>(s, p, q, l); }
    else s.pos = 0;
  }
  if (s.phase == 1) {
    if (dy < 0) { s.neg += 1; s.pos = 0; if (s.neg >= 1) vt_end_phase<M>(s, p, q, l); }
    else { s.neg = 0; s.pos += 1; }
  }
  if (dy < 0 && s.phase == 2) {
    s.neg += 1; s.pos = 0;
    if (s.neg == 1) s.n = 0;
    else vt_push(s, q, x, y, width, height, time);
    if (s.neg >= 3) { s.phase = 0; s.pos = 0; s.neg = 0; }
  }
  if (dy > 0 && s.phase == 2) {
    s.pos += 1; s.neg = 0;
    if (s.pos == 1) s.n = 0;
    else vt_push(s, q, x, y, width, height, time);
    if (s.pos >= 3) { s.phase = 1; s.pos = 0; s.neg = 0; }
  }
  s.y_prev = y; s.has_prev = 1;
}

// cols: [T][7] = time,x,y,dx,dy,h,w of ONE track.  One lane per clip does the sequential scan.
// pm: the metrics of the phases (MAXPH records); not read with M = false
template <bool M>
__device__ void analyze_track(const double* cols, int T, const VtParams& p, double* scratch /*5*T*/, double* ph, double* pm, int* nph_out) {
  const VtPath q{scratch, scratch + T, scratch + 2 * T, scratch + 3 * T, scratch + 4 * T, T};
  const VtPhases l{ph, pm, MAXPH};
  VtState s;
  vt_init(s);
  RollMean rm[4];
  for (int j = 0; j < 4; j++) rm[j].init();
  for (int i = 0; i < T; i++) {
    const bool drop = i >= 5;
    const double* old = cols + (size_t)(drop ? i - 5 : i) * 7;
    vt_row<M>(s, rm, p, cols + (size_t)i * 7, drop, old[1], old[2], q, l);
  }
  if (p.flush && s.phase != 2) vt_end_phase<M>(s, p, q, l);  // end_processing, VelocityTracker.py:224-230
  *nph_out = s.nph;
}

}  // namespace vbt
