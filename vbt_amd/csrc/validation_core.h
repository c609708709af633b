// Validation figure (include/vbt_hip.h, "Validation figure"): what validate.metric_trajectory + validate.compare compute of one
// (ground truth, tracked rows) pair, and the figure of kinovea.py:124-154 / qualysis.py:133-166 of it - layout, axes, merged points,
// records, the test of one pixel - as host + device functions of plain integers and doubles on raster_core.h.  vbt_validation_set's
// validation, the kernels of validation.hip and a host program (tests/fuzz/validation_check.cc) run these statements.  Every double is
// formed one IEEE operation per statement, without contraction.
//
// THE SUM ORDER.  Every sum of this file (the means, the MSE, the Pearson terms) over n terms is: VAL_LANES = 256 partial sums, partial
// l = 0.0 + term(l) + term(l + 256) + ... in rising order (0.0 when l >= n); then a halving tree over the 256, h = 128, 64, .. 1:
// p[l] = p[l] + p[l + h] for l < h; the sum is p[0].  A workgroup of 256 lanes forms it in parallel and val_sum below in a loop, to the
// same bits.  It is not numpy's pairwise order: parity with numpy is to a tolerance.
//
// Not taken from the reference: p-values (dropped there before printing), the LaTeX table, a display.  The axis text of the time axis
// is `Time [s]`: the reference's label is Slovak ("Cas" with a caron) and not in the 5 x 7 ASCII font.  A panel whose two series are
// constant and equal (d == 0) gets the margin 0.05 - this project's choice, matplotlib widens such a range in its own way.  The two
// curve colours are VAL_RGB_TRUTH and VAL_RGB_TRACKER below, near seaborn's two-colour `rocket` pair; palette parity is not claimed.
// fig_value_step, fig_col and fig_row are the rep figure's, unchanged; fig_value_ticks and fig_time_ticks write FigRec records with the
// rep figure's glyph indices, which lack the lower-case letters of the legend, so the ticks are written anew here on CfRec, to the same
// rule.  cf_item_range, cf_curve_mask, cf_records4 and cf_record_colour are the curve figure's, unchanged; cf_merge_series maps to the
// curve figure's fixed [0, 1.01] axes and is not used: val_point + val_merge_points are the same run merge on this figure's mapping.
#pragma once
#include "curve_figure_core.h"
#include "figure_core.h"

namespace vbt {

enum { VAL_KIND_KINOVEA = 0, VAL_KIND_QUALISYS = 1 };
enum { VAL_LANES = 256 };
// margins in cells of `scale` pixels: left (axis text, value labels, ticks), right, top (legend), between the panels, bottom
enum { VAL_CELLS_LEFT = 50, VAL_CELLS_RIGHT = 4, VAL_CELLS_TOP = 17, VAL_CELLS_MID = 6, VAL_CELLS_BOTTOM = 23, VAL_MIN_PLOT = 16 };
enum { VAL_MAX_PAIRS = 1024, VAL_MAX_ROWS = 1 << 20 };
enum { VAL_STATS = 8, VAL_HEAD = 6, VAL_GRID = 5, VAL_SERIES = 4 };            // head: t0, t1, X lo, hi, Y lo, hi
enum { VAL_S_MSE_X = 0, VAL_S_MSE_Y, VAL_S_R_X, VAL_S_R_Y, VAL_S_N, VAL_S_T_MIN, VAL_S_T_MAX, VAL_S_FLAGS };
enum { VAL_FLAG_R_X_NAN = 1, VAL_FLAG_R_Y_NAN = 2 };
// series: ground truth x, tracker x (upper panel), ground truth y, tracker y (lower panel); the tracker's over the ground truth's
enum { VAL_SER_REF_X = 0, VAL_SER_TRK_X, VAL_SER_REF_Y, VAL_SER_TRK_Y };
enum { VAL_MAX_TIME_TICKS = 140 };
enum { VAL_FIXED_RECS = 256 };   // 8 frame lines, 2 x 20 value ticks and labels, 140 time ticks with 28 labels at most, 3 texts, 5 of the legend
enum { VAL_RGB_TRUTH = 53u | 25u << 8 | 62u << 16, VAL_RGB_TRACKER = 243u | 118u << 8 | 81u << 16 };
// set's refusals of a pair's numbers
enum { VAL_OK = 0, VAL_BAD_NONFINITE, VAL_BAD_PLATE, VAL_BAD_FEW, VAL_BAD_TIME, VAL_BAD_SPAN };

// r | g << 8 | b << 16 of a colour index: the curve figure's, with the two series colours of this figure
__host__ __device__ inline uint32_t val_rgb(int c) {
  if (c == CF_C_SERIES + 0) return VAL_RGB_TRUTH;
  if (c == CF_C_SERIES + 1) return VAL_RGB_TRACKER;
  return cf_rgb(c);
}

struct ValGeom {
  int W, H, s, t;             // frame, scale, curve thickness
  int X0, Y0, Y1, PW, PH;     // the panels are [X0, X0 + PW) x [Y0, Y0 + PH) (X) and x [Y1, Y1 + PH) (Y)
};

__host__ __device__ inline ValGeom val_geom(int W, int H, int s, int t) {
  ValGeom G;
  G.W = W; G.H = H; G.s = s; G.t = t;
  G.X0 = VAL_CELLS_LEFT * s; G.Y0 = VAL_CELLS_TOP * s;
  G.PW = W - (VAL_CELLS_LEFT + VAL_CELLS_RIGHT) * s;
  const int rest = H - (VAL_CELLS_TOP + VAL_CELLS_MID + VAL_CELLS_BOTTOM) * s;
  G.PH = rest >= 0 ? rest / 2 : -1;
  G.Y1 = G.Y0 + G.PH + VAL_CELLS_MID * s;
  return G;
}

// ---- the sums ----

template <class F>
__host__ __device__ inline double val_partial(int l, int n, F term) {
  double s = 0.0;
  for (int i = l; i < n; i += VAL_LANES) {
    const double v = term(i);
    s = s + v;
  }
  return s;
}

// the whole sum, one statement after the other (a workgroup forms the partials a lane each and the tree through LDS)
template <class F>
inline double val_sum(int n, F term) {
  double p[VAL_LANES];
  for (int l = 0; l < VAL_LANES; l++) p[l] = val_partial(l, n, term);
  for (int h = VAL_LANES / 2; h >= 1; h >>= 1)
    for (int l = 0; l < h; l++) p[l] = p[l] + p[l + h];
  return p[0];
}

// ---- the numbers ----

// the window of column c (1 x, 2 y, 3 norm_plate_height, 4 norm_plate_width) as vbt_window_means takes it: > 0 rolling, 0 expanding, < 0 copy
__host__ __device__ inline int val_window(int kind, int c) {
  if (kind == VAL_KIND_KINOVEA) return c <= 2 ? 5 : 0;
  return c <= 2 ? -1 : 30;
}

// column c of rows[T][5] through its window, exactly as window_means_kernel (tracker_analysis.hip) forms it; out[i * 4 + c - 1]
__host__ __device__ inline void val_scan_column(const double* rows, int T, int c, int w, double* out) {
  RollMean r;
  r.init();
  for (int i = 0; i < T; i++) {
    double v = rows[(size_t)i * 5 + c];
    if (w >= 0) {
      if (w > 0 && i >= w) r.remove(rows[(size_t)(i - w) * 5 + c]);
      r.add(v);
      v = r.mean();
    }
    out[(size_t)i * 4 + c - 1] = v;
  }
}

// sm = the four window means of a row (x, y, height, width)
__host__ __device__ inline double val_metric_x(const double* sm, double plate) {
  const double a = sm[0] * plate;
  return a / sm[3];
}
__host__ __device__ inline double val_metric_y(const double* sm, double plate) {   // image y grows downwards
  const double a = -sm[1];
  const double b = a * plate;
  return b / sm[2];
}
__host__ __device__ inline double val_shift(double sum_ref, int n_ref, double sum_trk, int n_trk) {
  const double a = sum_ref / (double)n_ref;
  const double b = sum_trk / (double)n_trk;
  return a - b;
}

// the common span and the grid's size; times rise strictly, so the extremes are the ends
__host__ __device__ inline void val_span(const double* ref, int nref, const double* rows, int T, double rate, double* t_min, double* t_max, int* n) {
  const double r1 = ref[(size_t)(nref - 1) * 3], k1 = rows[(size_t)(T - 1) * 5];
  const double r0 = ref[0], k0 = rows[0];
  *t_max = r1 < k1 ? r1 : k1;
  *t_min = r0 > k0 ? r0 : k0;
  const double q = *t_max * rate;
  *n = q >= 2147483647.0 ? 2147483647 : (q >= 0.0 ? (int)q : 0);
}

// numpy.linspace(t_min, t_max, n)[i], n >= 2
__host__ __device__ inline double val_grid_t(int i, int n, double t_min, double t_max) {
  if (i == n - 1) return t_max;
  const double delta = t_max - t_min;
  const double step = delta / (double)(n - 1);
  const double a = (double)i * step;
  return a + t_min;
}

// validate._interp_linear at ts on the series (t[i * stride], v[i * stride]), len >= 2
__host__ __device__ inline double val_interp(const double* t, const double* v, int stride, int len, double ts) {
  int lo = 0, hi = len;
  while (lo < hi) {                                                     // searchsorted, side left
    const int mid = lo + ((hi - lo) >> 1);
    if (t[(size_t)mid * stride] < ts) lo = mid + 1; else hi = mid;
  }
  int h = lo < 1 ? 1 : lo;
  h = h > len - 1 ? len - 1 : h;
  const int l = h - 1;
  const double dv = v[(size_t)h * stride] - v[(size_t)l * stride];
  const double dt = t[(size_t)h * stride] - t[(size_t)l * stride];
  const double slope = dv / dt;
  const double d = ts - t[(size_t)l * stride];
  const double a = slope * d;
  return a + v[(size_t)l * stride];
}

__host__ __device__ inline double val_sq_diff(double a, double b) {
  const double d = a - b;
  return d * d;
}
__host__ __device__ inline double val_centred_sq(double a, double mean) {
  const double d = a - mean;
  return d * d;
}
__host__ __device__ inline double val_pearson_term(double a, double ma, double na, double b, double mb, double nb) {
  const double da = a - ma;
  const double db = b - mb;
  const double qa = da / na;
  const double qb = db / nb;
  return qa * qb;
}
// validate._pearson's clamp; *flag = 1 for NaN (a constant series: 0 / 0)
__host__ __device__ inline double val_pearson_clamp(double dot, int* flag) {
  *flag = dot != dot;
  if (dot != dot) return dot;
  const double a = dot < 1.0 ? dot : 1.0;
  return a > -1.0 ? a : -1.0;
}

// ---- what set refuses of a pair (in this order): VAL_OK or the reason, with the series (0 reference, 1 tracked rows) and the row ----
__host__ __device__ inline int val_pair_check(const double* ref, int nref, const double* rows, int T, int* series, int* row) {
  *series = 0; *row = 0;
  for (int i = 0; i < nref; i++)
    for (int k = 0; k < 3; k++)
      if (!ov_finite(ref[(size_t)i * 3 + k])) { *row = i; return VAL_BAD_NONFINITE; }
  *series = 1;
  for (int i = 0; i < T; i++)
    for (int k = 0; k < 5; k++)
      if (!ov_finite(rows[(size_t)i * 5 + k])) { *row = i; return VAL_BAD_NONFINITE; }
  for (int i = 0; i < T; i++)
    if (!(rows[(size_t)i * 5 + 3] > 0.0) || !(rows[(size_t)i * 5 + 4] > 0.0)) { *row = i; return VAL_BAD_PLATE; }
  if (nref < 2) { *series = 0; *row = nref; return VAL_BAD_FEW; }
  if (T < 2) { *row = T; return VAL_BAD_FEW; }
  *series = 0;
  for (int i = 1; i < nref; i++)
    if (!(ref[(size_t)i * 3] > ref[(size_t)(i - 1) * 3])) { *row = i; return VAL_BAD_TIME; }
  *series = 1;
  for (int i = 1; i < T; i++)
    if (!(rows[(size_t)i * 5] > rows[(size_t)(i - 1) * 5])) { *row = i; return VAL_BAD_TIME; }
  return VAL_OK;
}

// ---- the figure ----

// one panel's range from the extremes of both its series: matplotlib's default margin
__host__ __device__ inline void val_range(double m, double M, double* lo, double* hi) {
  const double d = M - m;
  double e = 0.05 * d;
  if (d == 0.0) e = 0.05;
  *lo = m - e;
  *hi = M + e;
}

// head[VAL_HEAD] from the last times and the extremes of x and y over both series, with the reference's widening rule
__host__ __device__ inline void val_head(int kind, double t_last, double mx, double Mx, double my, double My, double* head) {
  double loX, hiX, loY, hiY;
  val_range(mx, Mx, &loX, &hiX);
  val_range(my, My, &loY, &hiY);
  const double dX = hiX - loX;
  const double dY = hiY - loY;
  const double hX = dX / 2.0;
  const double hY = dY / 2.0;
  if (kind == VAL_KIND_KINOVEA ? dX < dY : !(dX > dY)) { loX = loX - hY; hiX = hiX + hY; }
  else if (kind == VAL_KIND_QUALISYS) { loY = loY - hX; hiY = hiY + hX; }
  head[0] = 0.0; head[1] = t_last; head[2] = loX; head[3] = hiX; head[4] = loY; head[5] = hiY;
}

// the (column, row) of a point of a series on the mapping of its panel: ws[0], ws[1]
__host__ __device__ inline void val_point(double t, double v, double t1, double lo, double hi, int PW, int PH, int32_t* ws) {
  ws[0] = fig_col(t, 0.0, t1, PW);
  ws[1] = fig_row(v, lo, hi, PH);
}

// The run merge of a series given as mapped points ws[n][2] (all finite, times rising, so the columns do not decrease): of every
// maximal stretch of consecutive points of one column the first, the last, the first of the lowest rows and the first of the highest
// rows.  out[CF_PT] per kept point; returns their number (at most n)
__host__ __device__ inline int val_merge_points(const int32_t* ws, int n, int32_t* out) {
  int m = 0, i = 0;
  while (i < n) {
    const int col = ws[(size_t)i * 2];
    int j = i, rlo = 0, rhi = 0, ilo = i, ihi = i;
    for (; j < n; j++) {
      if (ws[(size_t)j * 2] != col) break;
      const int r = ws[(size_t)j * 2 + 1];
      if (j == i || r < rlo) { rlo = r; ilo = j; }
      if (j == i || r > rhi) { rhi = r; ihi = j; }
    }
    for (int k = i; k < j; k++) {
      if (k != i && k != j - 1 && k != ilo && k != ihi) continue;
      out[(size_t)m * CF_PT + CF_PT_COL] = col;
      out[(size_t)m * CF_PT + CF_PT_ROW] = ws[(size_t)k * 2 + 1];
      out[(size_t)m * CF_PT + CF_PT_JOIN] = k == 0 ? 0 : 1;
      m++;
    }
    i = j;
  }
  return m;
}

__host__ __device__ inline int val_ascii(const char* s, uint8_t* out) {
  int n = 0;
  while (s[n]) { out[n] = (uint8_t)s[n]; n++; }
  return n;
}

// c hundredths (|c| <= 9999) as [-]d.dd / [-]dd.dd in ASCII
__host__ __device__ inline int val_centi_chars(int c, uint8_t* out) {
  int n = 0;
  if (c < 0) { out[n++] = '-'; c = -c; }
  const int w = c / 100;
  if (w >= 10) out[n++] = (uint8_t)('0' + w / 10 % 10);
  out[n++] = (uint8_t)('0' + w % 10);
  out[n++] = '.';
  out[n++] = (uint8_t)('0' + c / 10 % 10);
  out[n++] = (uint8_t)('0' + c % 10);
  return n;
}

// ticks and labels of the value axis of the panel at row Y: the rule of fig_value_ticks
__host__ __device__ inline void val_value_ticks(Recs& R, const ValGeom& G, int Y, double lo, double hi) {
  const int s = G.s;
  const Clip frame{0, 0, G.W - 1, G.H - 1};
  if (!(lo >= -1e9) || !(hi <= 1e9)) return;
  const int64_t step = fig_value_step(lo, hi);
  if (step == 0) return;
  const double lm = lo * 1000.0;
  const double lk = lm / (double)step;
  const int64_t k0 = (int64_t)floor(lk) - 1;
  for (int64_t k = k0; k < k0 + 10; k++) {
    const int64_t milli = k * step;
    const double v = (double)milli / 1000.0;
    if (!(v >= lo && v <= hi)) continue;
    const int row = fig_row(v, lo, hi, G.PH);
    int64_t c = milli / 10;
    c = c < -9999 ? -9999 : (c > 9999 ? 9999 : c);
    rec_box<CfRec>(R, CF_KIND_LINE, G.X0 - 3 * s, Y + row - s / 2, G.X0 - s - 1, Y + row - s / 2 + s - 1, frame, (int)c, 1);
    uint8_t ch[8];
    const int n = val_centi_chars((int)c, ch);
    rec_text<CfRec>(R, CF_KIND_TEXT, s, G.X0 - 4 * s - text_width(n, s), Y + row - 3 * s, ch, n, 0, frame, (int)c);
  }
}

// minor ticks every u seconds and major, labelled ones every 5 u under the lower panel: the rule of fig_time_ticks from t0 = 0
__host__ __device__ inline void val_time_ticks(Recs& R, const ValGeom& G, double t1) {
  const int s = G.s;
  const Clip frame{0, 0, G.W - 1, G.H - 1};
  if (!(t1 <= 1e9)) return;
  int64_t u = 1;
  while ((double)u * 128.0 < t1) u *= 10;
  const int top = G.Y1 + G.PH + s;
  for (int k = 0; k < VAL_MAX_TIME_TICKS; k++) {
    const int64_t sec = (int64_t)k * u;
    const double v = (double)sec;
    if (v > t1) break;
    const bool major = k % 5 == 0;
    const int col = fig_col(v, 0.0, t1, G.PW);
    rec_box<CfRec>(R, CF_KIND_LINE, G.X0 + col - s / 2, top, G.X0 + col - s / 2 + s - 1, top + (major ? 3 : 2) * s - 1, frame, (int)sec, 0);
    if (!major) continue;
    uint8_t g[12], ch[12];
    const int n = fig_int_chars(sec, g);
    for (int e = 0; e < n; e++) ch[e] = (uint8_t)('0' + g[e]);
    rec_text<CfRec>(R, CF_KIND_TEXT, s, G.X0 + col - text_width(n, s) / 2, top + 4 * s, ch, n, 0, frame, (int)sec);
  }
}

// All records of a figure from its head, in table order
__host__ __device__ inline int val_records(const ValGeom& G, int kind, const double* head, int32_t* rec, int cap) {
  Recs R{rec, cap, 0};
  const int s = G.s;
  const int Ys[2] = {G.Y0, G.Y1};
  const Clip frame{0, 0, G.W - 1, G.H - 1};
  uint8_t ch[20];
  // 1. per panel: the four frame lines around it (they leave every pixel of it to the curves), the value ticks, the axis text
  for (int k = 0; k < 2; k++) {
    const int Y = Ys[k];
    rec_box<CfRec>(R, CF_KIND_LINE, G.X0 - s, Y - s, G.X0 + G.PW + s - 1, Y - 1, frame, 0, 0);
    rec_box<CfRec>(R, CF_KIND_LINE, G.X0 - s, Y + G.PH, G.X0 + G.PW + s - 1, Y + G.PH + s - 1, frame, 0, 0);
    rec_box<CfRec>(R, CF_KIND_LINE, G.X0 - s, Y, G.X0 - 1, Y + G.PH - 1, frame, 0, 0);
    rec_box<CfRec>(R, CF_KIND_LINE, G.X0 + G.PW, Y, G.X0 + G.PW + s - 1, Y + G.PH - 1, frame, 0, 0);
    val_value_ticks(R, G, Y, head[2 + 2 * k], head[3 + 2 * k]);
    const int n = val_ascii(k ? "Y [m]" : "X [m]", ch);
    rec_text<CfRec>(R, CF_KIND_TEXT, s, s, Y + (G.PH - text_width(n, s)) / 2, ch, n, 1, frame, k);
  }
  // 2. the time axis
  val_time_ticks(R, G, head[1]);
  const int nt = val_ascii("Time [s]", ch);
  rec_text<CfRec>(R, CF_KIND_TEXT, s, G.X0 + (G.PW - text_width(nt, s)) / 2, G.Y1 + G.PH + 14 * s, ch, nt, 0, frame, 0);
  // 3. the legend, top right: the box, then a swatch and a text per entry, side by side
  const int n0 = kind == VAL_KIND_KINOVEA ? 7 : 8, n1 = 16;
  const int BW = 3 * s + 10 * s + text_width(n0, s) + 6 * s + 10 * s + text_width(n1, s) + 3 * s, BH = 13 * s;
  const int bx = G.X0 + G.PW + s - BW, by = 2 * s;
  rec_box<CfRec>(R, CF_KIND_LEGEND_BOX, bx, by, bx + BW - 1, by + BH - 1, frame, BW, BH);
  int x = bx + 3 * s;
  for (int k = 0; k < 2; k++) {
    const int n = val_ascii(k ? "Velocity Tracker" : (kind == VAL_KIND_KINOVEA ? "Kinovea" : "Qualisys"), ch);
    rec_box<CfRec>(R, CF_KIND_SWATCH, x, by + 5 * s, x + 8 * s - 1, by + 8 * s - 1, frame, k, k);
    rec_text<CfRec>(R, CF_KIND_LEGEND_TEXT, s, x + 10 * s, by + 3 * s, ch, n, 0, frame, k);
    x += 10 * s + text_width(n, s) + 6 * s;
  }
  return R.n;
}

// The colour indices out[e] of the frame pixels (px + e, py), e < n <= 4, all in the frame, from the whole tables: the four series'
// views over all their merged points, the records.  The statement the host program runs; the render kernel forms the same from its
// staged parts.
__host__ __device__ inline void val_pixels4(const ValGeom& G, const CfSeriesView* ser, const int32_t* recs, int nrec, int px, int py, int n, int* out) {
  int over[4], oc[4], under[4], uc[4], curve[4] = {-1, -1, -1, -1};
  cf_records4(recs, nrec, G.s, px, py, n, over, oc, under, uc);
  for (int k = 0; k < VAL_SERIES; k++) {                                 // the later series overwrites
    const int qy = py - (k >= 2 ? G.Y1 : G.Y0);
    if (qy < 0 || qy >= G.PH) continue;
    int i0, i1, k0, k1;
    cf_item_range(ser[k], 0, ser[k].m, G.t, px - G.X0, px + n - 1 - G.X0, &i0, &i1, &k0, &k1);
    if (i0 > i1) continue;
    const unsigned mask = cf_curve_mask(ser[k], G.t, G.PW, px - G.X0, n, qy, i0, i1, -65536, 65536);
    for (int e = 0; e < 4; e++)
      if (mask >> e & 1) curve[e] = CF_C_SERIES + ser[k].colour;
  }
  for (int e = 0; e < n; e++) out[e] = over[e] != CF_KIND_NONE ? oc[e] : (curve[e] >= 0 ? curve[e] : uc[e]);
}

// ---- the whole pair, one statement after the other: what the prepare kernel computes with a workgroup ----

struct ValPairOut {
  double* sm;        // [T][4] window means
  double* traj;      // [T][3] time, x, y aligned
  double* grid;      // [n][5] ts, ref x, tracker x, ref y, tracker y
  double* stats;     // [VAL_STATS]
  double* head;      // [VAL_HEAD]
  int32_t* ws[VAL_SERIES];    // [points of the series][2]: column, row before the merge
  int32_t* pts[VAL_SERIES];
  int32_t* cnt;      // [VAL_SERIES]
  int32_t* recs;
  int32_t* nrec;
  int rec_cap;
};

// a pair that val_pair_check passed and whose grid has 2 <= n points
inline void val_pair(const ValGeom& G, int kind, double plate, double rate, const double* ref, int nref, const double* rows, int T, const ValPairOut& O) {
  for (int c = 1; c <= 4; c++) val_scan_column(rows, T, c, val_window(kind, c), O.sm);
  for (int i = 0; i < T; i++) {
    O.traj[(size_t)i * 3] = rows[(size_t)i * 5];
    O.traj[(size_t)i * 3 + 1] = val_metric_x(O.sm + (size_t)i * 4, plate);
    O.traj[(size_t)i * 3 + 2] = val_metric_y(O.sm + (size_t)i * 4, plate);
  }
  for (int a = 2; a >= 1; a--) {                                         // y, then x
    const double sr = val_sum(nref, [&](int i) { return ref[(size_t)i * 3 + a]; });
    const double st = val_sum(T, [&](int i) { return O.traj[(size_t)i * 3 + a]; });
    const double d = val_shift(sr, nref, st, T);
    for (int i = 0; i < T; i++) O.traj[(size_t)i * 3 + a] = O.traj[(size_t)i * 3 + a] + d;
  }
  double t_min, t_max;
  int n;
  val_span(ref, nref, rows, T, rate, &t_min, &t_max, &n);
  for (int i = 0; i < n; i++) {
    const double ts = val_grid_t(i, n, t_min, t_max);
    double* g = O.grid + (size_t)i * VAL_GRID;
    g[0] = ts;
    g[1] = val_interp(ref, ref + 1, 3, nref, ts);
    g[2] = val_interp(O.traj, O.traj + 1, 3, T, ts);
    g[3] = val_interp(ref, ref + 2, 3, nref, ts);
    g[4] = val_interp(O.traj, O.traj + 2, 3, T, ts);
  }
  int flags = 0;
  for (int a = 0; a < 2; a++) {
    const double* ga = O.grid + 1 + 2 * a;
    const double* gb = O.grid + 2 + 2 * a;
    const double se = val_sum(n, [&](int i) { return val_sq_diff(ga[(size_t)i * VAL_GRID], gb[(size_t)i * VAL_GRID]); });
    O.stats[VAL_S_MSE_X + a] = se / (double)n;
    const double sa = val_sum(n, [&](int i) { return ga[(size_t)i * VAL_GRID]; });
    const double sb = val_sum(n, [&](int i) { return gb[(size_t)i * VAL_GRID]; });
    const double ma = sa / (double)n;
    const double mb = sb / (double)n;
    const double qa = val_sum(n, [&](int i) { return val_centred_sq(ga[(size_t)i * VAL_GRID], ma); });
    const double qb = val_sum(n, [&](int i) { return val_centred_sq(gb[(size_t)i * VAL_GRID], mb); });
    const double na = sqrt(qa);
    const double nb = sqrt(qb);
    const double dot = val_sum(n, [&](int i) { return val_pearson_term(ga[(size_t)i * VAL_GRID], ma, na, gb[(size_t)i * VAL_GRID], mb, nb); });
    int flag;
    O.stats[VAL_S_R_X + a] = val_pearson_clamp(dot, &flag);
    if (flag) flags |= a ? VAL_FLAG_R_Y_NAN : VAL_FLAG_R_X_NAN;
  }
  O.stats[VAL_S_N] = (double)n; O.stats[VAL_S_T_MIN] = t_min; O.stats[VAL_S_T_MAX] = t_max; O.stats[VAL_S_FLAGS] = (double)flags;
  // the figure
  double m[2] = {0, 0}, M[2] = {0, 0};
  for (int a = 0; a < 2; a++) {
    m[a] = ref[1 + a]; M[a] = ref[1 + a];
    for (int i = 0; i < nref; i++) { const double v = ref[(size_t)i * 3 + 1 + a]; m[a] = v < m[a] ? v : m[a]; M[a] = v > M[a] ? v : M[a]; }
    for (int i = 0; i < T; i++) { const double v = O.traj[(size_t)i * 3 + 1 + a]; m[a] = v < m[a] ? v : m[a]; M[a] = v > M[a] ? v : M[a]; }
  }
  const double r1 = ref[(size_t)(nref - 1) * 3], k1 = rows[(size_t)(T - 1) * 5];
  val_head(kind, r1 > k1 ? r1 : k1, m[0], M[0], m[1], M[1], O.head);
  for (int k = 0; k < VAL_SERIES; k++) {
    const int a = k / 2;
    const bool trk = k & 1;
    const double* src = trk ? O.traj : ref;
    const int np = trk ? T : nref;
    for (int i = 0; i < np; i++) val_point(src[(size_t)i * 3], src[(size_t)i * 3 + 1 + a], O.head[1], O.head[2 + 2 * a], O.head[3 + 2 * a], G.PW, G.PH, O.ws[k] + (size_t)i * 2);
    O.cnt[k] = val_merge_points(O.ws[k], np, O.pts[k]);
  }
  *O.nrec = val_records(G, kind, O.head, O.recs, O.rec_cap);
}

}  // namespace vbt
