// Rep figure (include/vbt_hip.h, "Rep figure"): the figure's layout, axes, records and the test of one pixel, as host + device
// functions of plain integers and doubles, on the record table, text test and segment test of raster_core.h.  vbt_figure_set's validation, the kernels of figure.hip and a host program
// (tests/fuzz/figure_check.cc) run these statements.  Every double is formed one IEEE operation per statement, without contraction.
#pragma once
#include "raster_core.h"
#include "roll_mean.h"

namespace vbt {

// margins in cells of `scale` pixels: left (value labels), right, above the upper rectangle (title), between the rectangles, below
enum { FIG_CELLS_LEFT = 40, FIG_CELLS_RIGHT = 4, FIG_CELLS_TOP = 11, FIG_CELLS_MID = 13, FIG_CELLS_BOTTOM = 14, FIG_MIN_PLOT = 16 };
enum { FIG_KEY1_CELLS = 48, FIG_KEY2_CELLS = 70, FIG_LABEL_TOP_CELLS = 2 };                // legend keys from the rectangle's left edge; rep label below its top edge
enum { FIG_MAX_FIGURES = 4096, FIG_MAX_ROWS = 1 << 20, FIG_MAX_PHASES = 65536, FIG_MAX_TIME_TICKS = 264 };
enum { FIG_HEAD = 6 };                                                                      // t0, t1, position lo, hi, velocity lo, hi
enum { FIG_PT_COL = 0, FIG_PT_X, FIG_PT_Y, FIG_PT_DX, FIG_PT_DY, FIG_PT = 5 };             // point record: column, then the row of each series
// record: 12 int32, the layout FigRec of raster_core.h
enum { FIG_R_VALUE = FigRec::VALUE, FIG_R_AUX = FigRec::AUX, FIG_REC = FigRec::REC };
enum { FIG_KIND_SPAN = 0, FIG_KIND_LINE = 1, FIG_KIND_SWATCH = 2, FIG_KIND_TEXT = 3 };
enum { FIG_TEXT_CHARS = 12, FIG_FIXED_RECS = 384 };                                         // records besides the 4 per phase: 8 + 4 + 6 + 32 + 264 + 54 at most
// colour index of a pixel
enum { FIG_C_WHITE = 0, FIG_C_CONCENTRIC, FIG_C_ECCENTRIC, FIG_C_INK, FIG_C_X, FIG_C_Y, FIG_C_DX, FIG_C_DY, FIG_COLOURS };
enum { FIG_GLYPH_MINUS = 22, FIG_GLYPH_SLASH, FIG_GLYPH_S, FIG_GLYPH_X, FIG_GLYPH_Y, FIG_GLYPH_DCAP };

// r | g << 8 | b << 16 of a colour index
__host__ __device__ inline uint32_t fig_rgb(int c) {
  switch (c) {
    case FIG_C_CONCENTRIC: return 247u | 212u << 8 | 212u << 16;
    case FIG_C_ECCENTRIC: return 255u | 229u << 8 | 207u << 16;
    case FIG_C_INK: return 0u;
    case FIG_C_X: return 53u | 25u << 8 | 62u << 16;
    case FIG_C_Y: return 226u | 75u << 8 | 64u << 16;
    case FIG_C_DX: return 112u | 31u << 8 | 87u << 16;
    case FIG_C_DY: return 243u | 118u << 8 | 81u << 16;
    default: return 0xffffffu;
  }
}

// the glyphs ov_hud_glyph lacks, in its 35-bit format (rows top to bottom, five bits each)
__host__ __device__ inline uint64_t fig_glyph(int g) {
  switch (g) {
    case FIG_GLYPH_MINUS: return 0b00000'00000'00000'11111'00000'00000'00000ull;
    case FIG_GLYPH_SLASH: return 0b00001'00001'00010'00100'01000'10000'10000ull;
    case FIG_GLYPH_S:     return 0b01111'10000'10000'01110'00001'00001'11110ull;
    case FIG_GLYPH_X:     return 0b10001'10001'01010'00100'01010'10001'10001ull;
    case FIG_GLYPH_Y:     return 0b10001'10001'01010'00100'00100'00100'00100ull;
    case FIG_GLYPH_DCAP:  return 0b11110'10001'10001'10001'10001'10001'11110ull;
    default: return ov_hud_glyph(g);
  }
}

struct FigGeom {
  int W, H, s, t;             // frame, scale, curve thickness
  int X0, Y0, Y1, PW, PH;     // the rectangles are [X0, X0 + PW) x [Y0, Y0 + PH) and x [Y1, Y1 + PH)
};

__host__ __device__ inline FigGeom fig_geom(int W, int H, int s, int t) {
  FigGeom G;
  G.W = W; G.H = H; G.s = s; G.t = t;
  G.X0 = FIG_CELLS_LEFT * s; G.Y0 = FIG_CELLS_TOP * s;
  G.PW = W - (FIG_CELLS_LEFT + FIG_CELLS_RIGHT) * s;
  const int rest = H - (FIG_CELLS_TOP + FIG_CELLS_MID + FIG_CELLS_BOTTOM) * s;
  G.PH = rest >= 0 ? rest / 2 : -1;
  G.Y1 = G.Y0 + G.PH + FIG_CELLS_MID * s;
  return G;
}

__host__ __device__ inline int32_t fig_col(double time, double t0, double t1, int PW) {
  if (!(t1 > t0)) return 0;
  const double d = time - t0;
  const double w = t1 - t0;
  const double q = d / w;
  const double v = q * (double)(PW - 1);
  return fig_clamp_round(v);
}

__host__ __device__ inline int32_t fig_row(double value, double lo, double hi, int PH) {
  const double d = hi - value;
  const double w = hi - lo;
  const double q = d / w;
  const double v = q * (double)(PH - 1);
  return fig_clamp_round(v);
}

// plot.py:145 on the data's own min and max (matplotlib's autoscale margin is not taken)
__host__ __device__ inline void fig_position_range(double m, double M, double* lo, double* hi) {
  const double a = m - 0.2, b = M + 0.2;
  *lo = a > 0.0 ? a : 0.0;
  *hi = b < 1.0 ? b : 1.0;
  if (*hi <= *lo) { *lo = a; *hi = b; }
}

__host__ __device__ inline void fig_velocity_range(double m, double M, double* lo, double* hi) {
  const double d = M - m;
  double pad = d * 0.05;
  if (pad == 0.0) pad = 0.5;
  *lo = m - pad;
  *hi = M + pad;
}

// head[FIG_HEAD] from the extremes of the smoothed series (T > 0) or the empty figure's
__host__ __device__ inline void fig_head(int T, double t0, double t1, double pm, double pM, double vm, double vM, double* head) {
  if (T <= 0) { head[0] = 0; head[1] = 0; head[2] = 0; head[3] = 1; head[4] = 0; head[5] = 1; return; }
  head[0] = t0; head[1] = t1;
  fig_position_range(pm, pM, head + 2, head + 3);
  fig_velocity_range(vm, vM, head + 4, head + 5);
}

// the step of a value axis in thousandths; 0: none qualifies
__host__ __device__ inline int64_t fig_value_step(double lo, double hi) {
  const double span = hi - lo;
  const double milli = span * 1000.0;
  int64_t decade = 10;
  for (int k = 0; k < 7; k++, decade *= 10) {
    for (int j = 0; j < 3; j++) {
      const int64_t step = decade * (j == 0 ? 1 : (j == 1 ? 2 : 5));
      if (step > 10000000) return 0;
      const double n = milli / (double)step;
      if (n <= 6.0) return step;
    }
  }
  return 0;
}

// c hundredths (|c| <= 9999) as [-]d.dd / [-]dd.dd; returns the number of characters
__host__ __device__ inline int fig_centi_chars(int c, uint8_t* out) {
  int n = 0;
  if (c < 0) { out[n++] = FIG_GLYPH_MINUS; c = -c; }
  const int w = c / 100;
  if (w >= 10) out[n++] = (uint8_t)(w / 10 % 10);
  out[n++] = (uint8_t)(w % 10);
  out[n++] = OV_GLYPH_DOT;
  out[n++] = (uint8_t)(c / 10 % 10);
  out[n++] = (uint8_t)(c % 10);
  return n;
}

// an integer of at most 10 digits with its sign
__host__ __device__ inline int fig_int_chars(int64_t v, uint8_t* out) {
  uint8_t dig[12];
  int n = 0, nd = 0;
  if (v < 0) { out[n++] = FIG_GLYPH_MINUS; v = -v; }
  do { dig[nd++] = (uint8_t)(v % 10); v /= 10; } while (v && nd < 10);
  for (int k = 0; k < nd; k++) out[n++] = dig[nd - 1 - k];
  return n;
}

// ticks and labels of the value axis of the rectangle at row Y
__host__ __device__ inline void fig_value_ticks(Recs& R, const FigGeom& G, int Y, double lo, double hi) {
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
    rec_box<FigRec>(R, FIG_KIND_LINE, G.X0 - 3 * s, Y + row - s / 2, G.X0 - s - 1, Y + row - s / 2 + s - 1, frame, (int)c, 0);
    uint8_t ch[FIG_TEXT_CHARS];
    const int n = fig_centi_chars((int)c, ch);
    rec_text<FigRec>(R, FIG_KIND_TEXT, s, G.X0 - 4 * s - text_width(n, s), Y + row - 3 * s, ch, n, 0, frame, (int)c);
  }
}

// minor ticks every u seconds and major ones every 5 u, u the smallest power of ten that gives at most 256 steps between t0 and t1 (1 for
// every set shorter than 256 s: plot.py:208-215), under the lower rectangle
__host__ __device__ inline void fig_time_ticks(Recs& R, const FigGeom& G, double t0, double t1) {
  const int s = G.s;
  const Clip frame{0, 0, G.W - 1, G.H - 1};
  if (!(t0 >= -1e9) || !(t1 <= 1e9)) return;
  const double w = t1 - t0;
  int64_t u = 1;
  while ((double)u * 256.0 < w) u *= 10;
  const int64_t i0 = (int64_t)floor(t0), m = 5 * u;
  const int64_t base = i0 - ((i0 % m) + m) % m;                         // Python's x_min - x_min % 5
  const int top = G.Y1 + G.PH + s;
  for (int k = 0; k < FIG_MAX_TIME_TICKS; k++) {
    const int64_t sec = base + (int64_t)k * u;
    const double v = (double)sec;
    if (v > t1) break;
    if (v < t0) continue;
    const bool major = (sec - base) % m == 0;
    const int col = fig_col(v, t0, t1, G.PW);
    rec_box<FigRec>(R, FIG_KIND_LINE, G.X0 + col - s / 2, top, G.X0 + col - s / 2 + s - 1, top + (major ? 3 : 2) * s - 1, frame, (int)sec, major);
    if (!major) continue;
    uint8_t ch[FIG_TEXT_CHARS];
    const int n = fig_int_chars(sec, ch);
    rec_text<FigRec>(R, FIG_KIND_TEXT, s, G.X0 + col - text_width(n, s) / 2, top + 4 * s, ch, n, 0, frame, (int)sec);
  }
}

// All records of a figure from its head and its phases (each passed ov_hud_phase_check), in the order of the contract: the phase
// records first - two spans per concentric or eccentric phase, then two labels per concentric one, in phase order - then the fixed ones
__host__ __device__ inline int fig_records(const FigGeom& G, const double* head, const double* ph, int P, int32_t* rec, int cap) {
  Recs R{rec, cap, 0};
  const int s = G.s;
  const double t0 = head[0], t1 = head[1];
  const int Ys[2] = {G.Y0, G.Y1};
  const Clip frame{0, 0, G.W - 1, G.H - 1}, plot[2] = {{G.X0, G.Y0, G.X0 + G.PW - 1, G.Y0 + G.PH - 1}, {G.X0, G.Y1, G.X0 + G.PW - 1, G.Y1 + G.PH - 1}};
  for (int i = 0; i < P; i++) {
    const double* p = ph + (size_t)i * 6;
    const int type = (int)p[5];
    if (type == 2) continue;
    const int c0 = fig_col(p[0], t0, t1, G.PW), c1 = fig_col(p[1], t0, t1, G.PW);
    for (int k = 0; k < 2; k++) rec_box<FigRec>(R, FIG_KIND_SPAN, G.X0 + c0, Ys[k], G.X0 + c1, Ys[k] + G.PH - 1, plot[k], i, type);
  }
  for (int i = 0; i < P; i++) {
    const double* p = ph + (size_t)i * 6;
    if ((int)p[5] != 0) continue;
    const double dur = p[1] - p[0];
    const double sum = p[0] + p[1];
    const double mid = sum / 2.0;
    const int cc = fig_col(mid, t0, t1, G.PW);
    const int v[2] = {ov_centi(p[4]), dur > 0 ? ov_centi(p[4] / dur) : 0};
    for (int k = 0; k < 2; k++) {
      uint8_t ch[FIG_TEXT_CHARS];
      const int n = fig_centi_chars(v[k], ch);
      rec_text<FigRec>(R, FIG_KIND_TEXT, s, G.X0 + cc - 3 * s, Ys[k] + FIG_LABEL_TOP_CELLS * s, ch, n, 1, plot[k], v[k]);
    }
  }
  const uint8_t title[2][7] = {{OV_GLYPH_R, OV_GLYPH_O, OV_GLYPH_M, OV_GLYPH_SPACE, OV_GLYPH_M, 0, 0},
                               {OV_GLYPH_A, OV_GLYPH_C, OV_GLYPH_V, OV_GLYPH_SPACE, OV_GLYPH_M, FIG_GLYPH_SLASH, FIG_GLYPH_S}};
  const uint8_t keys[4][2] = {{FIG_GLYPH_X, 0}, {FIG_GLYPH_Y, 0}, {FIG_GLYPH_DCAP, FIG_GLYPH_X}, {FIG_GLYPH_DCAP, FIG_GLYPH_Y}};
  for (int k = 0; k < 2; k++) {
    const int Y = Ys[k];
    // the frame lines lie around the rectangle, s wide, and leave every pixel of it to the curves and spans
    rec_box<FigRec>(R, FIG_KIND_LINE, G.X0 - s, Y - s, G.X0 + G.PW + s - 1, Y - 1, frame, 0, 0);
    rec_box<FigRec>(R, FIG_KIND_LINE, G.X0 - s, Y + G.PH, G.X0 + G.PW + s - 1, Y + G.PH + s - 1, frame, 0, 0);
    rec_box<FigRec>(R, FIG_KIND_LINE, G.X0 - s, Y, G.X0 - 1, Y + G.PH - 1, frame, 0, 0);
    rec_box<FigRec>(R, FIG_KIND_LINE, G.X0 + G.PW, Y, G.X0 + G.PW + s - 1, Y + G.PH - 1, frame, 0, 0);
    rec_text<FigRec>(R, FIG_KIND_TEXT, s, G.X0, Y - 9 * s, title[k], k ? 7 : 5, 0, frame, 0);
    for (int j = 0; j < 2; j++) {
      const int kx = G.X0 + (j ? FIG_KEY2_CELLS : FIG_KEY1_CELLS) * s;
      rec_box<FigRec>(R, FIG_KIND_SWATCH, kx, Y - 7 * s, kx + 6 * s - 1, Y - 4 * s - 1, frame, 0, FIG_C_X + 2 * k + j);
      rec_text<FigRec>(R, FIG_KIND_TEXT, s, kx + 7 * s, Y - 9 * s, keys[2 * k + j], k ? 2 : 1, 0, frame, 0);
    }
    fig_value_ticks(R, G, Y, head[2 + 2 * k], head[3 + 2 * k]);
  }
  fig_time_ticks(R, G, t0, t1);
  return R.n;
}

// ---- one pixel ----

// What a pixel is tested against: the point table (point i at pts[(i - pt_base) * FIG_PT], for the i the segments passed to fig_pixels4
// touch) and a set of records that contains every record whose visible box holds the pixel
struct FigView {
  const int32_t* pts;
  int pt_base, T;
  const int32_t* recs;
  int nrec;
  int rlo[FIG_PT], rhi[FIG_PT];   // per series (FIG_PT_X ..): bounds that hold the rows of every point the passed segments touch
};
__host__ __device__ inline void fig_view_unbounded(FigView& V) {
  for (int k = 0; k < FIG_PT; k++) { V.rlo[k] = -65536; V.rhi[k] = 65536; }
}

// The segments that can cover a pixel of columns [pa, pb] (rectangle coordinates): segment i joins points i and min(i + 1, T - 1),
// i < max(T - 1, 1); those with col_{i+1} >= pa - h and col_i <= pb + h, h = (t + 1) / 2.  Empty: *seg0 > *seg1.  [lo, hi) is a range
// of points known to hold both bounds ([0, T), or the bounds *k0, *k1 of columns that contain [pa, pb]).
__host__ __device__ inline void fig_seg_range(const FigView& V, int lo, int hi, int t, int pa, int pb, int* seg0, int* seg1, int* k0_out, int* k1_out) {
  if (V.T <= 0) { *seg0 = 0; *seg1 = -1; *k0_out = 0; *k1_out = 0; return; }
  const int h = (t + 1) / 2, nseg = V.T > 1 ? V.T - 1 : 1;
  const int k0 = col_lower_bound(V.pts, FIG_PT, V.pt_base, lo, hi, pa - h), k1 = col_lower_bound(V.pts, FIG_PT, V.pt_base, lo, hi, pb + h + 1);
  *seg0 = k0 > 0 ? k0 - 1 : 0;
  *seg1 = k1 - 1 < nseg - 1 ? k1 - 1 : nseg - 1;
  *k0_out = k0; *k1_out = k1;
}

// which of the pixels (qx0 + e, qy), e < n <= 4 (rectangle coordinates, columns outside [0, PW) never), series `which` (FIG_PT_X ..) covers
// by one of the segments [seg0, seg1]: rule 2 of the overlay.  Bit e of the result.
__host__ __device__ inline unsigned fig_curve_mask(const FigView& V, int t, int PW, int which, int qx0, int n, int qy, int seg0, int seg1) {
  const int h = (t + 1) / 2;
  // (selects, not an index: the view stays in registers)
  const int lo = which == FIG_PT_X ? V.rlo[FIG_PT_X] : (which == FIG_PT_Y ? V.rlo[FIG_PT_Y] : (which == FIG_PT_DX ? V.rlo[FIG_PT_DX] : V.rlo[FIG_PT_DY]));
  const int hi = which == FIG_PT_X ? V.rhi[FIG_PT_X] : (which == FIG_PT_Y ? V.rhi[FIG_PT_Y] : (which == FIG_PT_DX ? V.rhi[FIG_PT_DX] : V.rhi[FIG_PT_DY]));
  if (qy < lo - h || qy > hi + h) return 0;
  const unsigned all = (1u << n) - 1u;
  unsigned m = 0;
  for (int i = seg0; i <= seg1; i++) {
    const int j = i + 1 < V.T ? i + 1 : V.T - 1;
    const int32_t *a = V.pts + (size_t)(i - V.pt_base) * FIG_PT, *b = V.pts + (size_t)(j - V.pt_base) * FIG_PT;
    m |= quad_segment_mask(qx0, n, qy, PW, a[0], a[which], b[0], b[which], t);
    if (m == all) break;
  }
  return m;
}

// The colour indices out[e] of the frame pixels (px + e, py), e < n <= 4, all in the frame: for each the first of text, second
// curve, first curve, lines, span, white that covers it.  [seg0, seg1] contains the segments fig_seg_range gives for their columns.
__host__ __device__ inline void fig_pixels4(const FigGeom& G, const FigView& V, int px, int py, int n, int seg0, int seg1, int* out) {
  int line[4] = {-1, -1, -1, -1}, span[4] = {-1, -1, -1, -1}, span_type[4] = {0, 0, 0, 0};
  unsigned text = 0, second = 0, first = 0;
  for (int k = 0; k < V.nrec; k++) {
    const int32_t* r = V.recs + (size_t)k * FIG_REC;
    const int x0 = r[REC_X0], x1 = r[REC_X1];
    if (px + n - 1 < x0 || px > x1 || py < r[REC_Y0] || py > r[REC_Y1]) continue;
    const int kind = r[REC_KIND], value = r[FIG_R_VALUE], aux = r[FIG_R_AUX];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int e = 0; e < 4; e++) {
      if (e >= n || px + e < x0 || px + e > x1) continue;
      if (kind == FIG_KIND_TEXT) { if (text_covers<FigRec, fig_glyph>(r, G.s, px + e, py)) text |= 1u << e; }
      else if (kind == FIG_KIND_SPAN) { if (value >= span[e]) { span[e] = value; span_type[e] = aux; } }   // the later phase wins
      else line[e] = kind == FIG_KIND_SWATCH ? aux : FIG_C_INK;
    }
  }
  const int panel = py >= G.Y1 ? 1 : 0, qy = py - (panel ? G.Y1 : G.Y0);
  if (qy >= 0 && qy < G.PH && seg0 <= seg1) {
    second = fig_curve_mask(V, G.t, G.PW, FIG_PT_Y + 2 * panel, px - G.X0, n, qy, seg0, seg1);
    first = fig_curve_mask(V, G.t, G.PW, FIG_PT_X + 2 * panel, px - G.X0, n, qy, seg0, seg1);
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int e = 0; e < 4; e++) {
    if (e >= n) continue;
    int c = FIG_C_WHITE;
    if (text >> e & 1) c = FIG_C_INK;
    else if (second >> e & 1) c = FIG_C_Y + 2 * panel;
    else if (first >> e & 1) c = FIG_C_X + 2 * panel;
    else if (line[e] >= 0) c = line[e];
    else if (span[e] >= 0) c = span_type[e] == 0 ? FIG_C_CONCENTRIC : FIG_C_ECCENTRIC;
    out[e] = c;
  }
}

// ---- the whole figure, one statement after the other: what the prepare kernel computes with a workgroup ----

// sm[4][T]: the rolling(5, min_periods=1) means of x, y, dx, dy
__host__ __device__ inline void fig_smooth_series(const double* rows7, int T, int series, double* out) {
  RollMean rm;
  rm.init();
  for (int i = 0; i < T; i++) {
    if (i >= 5) rm.remove(rows7[(size_t)(i - 5) * 7 + 1 + series]);
    rm.add(rows7[(size_t)i * 7 + 1 + series]);
    out[i] = rm.mean();
  }
}

__host__ __device__ inline void fig_point(const FigGeom& G, const double* head, double time, const double* sm4, int32_t* pt) {
  pt[FIG_PT_COL] = fig_col(time, head[0], head[1], G.PW);
  pt[FIG_PT_X] = fig_row(sm4[0], head[2], head[3], G.PH);
  pt[FIG_PT_Y] = fig_row(sm4[1], head[2], head[3], G.PH);
  pt[FIG_PT_DX] = fig_row(sm4[2], head[4], head[5], G.PH);
  pt[FIG_PT_DY] = fig_row(sm4[3], head[4], head[5], G.PH);
}

// What vbt_figure_set refuses a row for on its doubles: 0 ok, 1 a non-finite value, 2 a time below the previous row's
__host__ __device__ inline int fig_row_check(const double* r, const double* prev) {
  for (int k = 0; k < 7; k++)
    if (!ov_finite(r[k])) return 1;
  if (prev && r[0] < prev[0]) return 2;
  return 0;
}

}  // namespace vbt
