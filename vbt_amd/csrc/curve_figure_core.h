// Curve figure (include/vbt_hip.h, "Curve figure"): layout, axes, records, the run merge and the test of one pixel, as host + device
// functions of plain integers and doubles, on the record table, text test and segment test of raster_core.h (and on nothing of the rep
// figure's).  vbt_curve_figure_set's validation, the kernels of curve_figure.hip and a host program
// (tests/fuzz/curve_figure_check.cc) run these statements.  Every double is formed one IEEE operation per statement, without contraction.
#pragma once
#include "curve_font.h"
#include "raster_core.h"

namespace vbt {

// margins in cells of `scale` pixels: left (axis title, value labels, ticks), right, top, bottom (ticks, labels, axis title)
enum { CF_CELLS_LEFT = 30, CF_CELLS_RIGHT = 4, CF_CELLS_TOP = 4, CF_CELLS_BOTTOM = 22, CF_MIN_PLOT = 16 };
enum { CF_MAX_FIGURES = 1024, CF_MAX_SERIES = 16, CF_MAX_POINTS = 1 << 22, CF_MAX_MARKS = 64, CF_PALETTE = 10 };
enum { CF_TEXT_MAX = 63, CF_MARK_TEXT_MAX = 15, CF_TITLE_MAX = 31, CF_MINOR_MIN = 20, CF_MINOR_MAX = 1000 };
enum { CF_PT_COL = 0, CF_PT_ROW, CF_PT_JOIN, CF_PT = 3 };      // merged point: column, row, 1 when a segment joins it to the point before
// record: 28 int32, the layout CfRec of raster_core.h
enum { CF_R_VALUE = CfRec::VALUE, CF_R_AUX = CfRec::AUX, CF_REC = CfRec::REC };
// the kinds are the priorities of "one writer per pixel": the smallest kind that covers a pixel decides it; 6 is the curves' place
enum { CF_KIND_LEGEND_TEXT = 0, CF_KIND_SWATCH, CF_KIND_LEGEND_BOX, CF_KIND_MARK_TEXT, CF_KIND_MARKER, CF_KIND_LEADER, CF_KIND_CURVES,
       CF_KIND_LINE, CF_KIND_TEXT, CF_KIND_GRID_MAJOR, CF_KIND_GRID_MINOR, CF_KIND_NONE };
enum { CF_FIXED_RECS = 144 };                                  // 2 spines, 12 ticks, 12 labels, 2 titles, 12 major and at most 2 x 48 minor grid lines
enum { CF_C_WHITE = 0, CF_C_INK, CF_C_GRID_MAJOR, CF_C_GRID_MINOR, CF_C_BORDER, CF_C_SERIES };    // CF_C_SERIES + palette index
enum { CF_LEGEND_LOWER_LEFT = 0, CF_LEGEND_LOWER_RIGHT = 1 };
enum { CF_CHECK_OK = 0, CF_CHECK_NOT_MONOTONE = 1 };

// r | g << 8 | b << 16 of a colour index
__host__ __device__ inline uint32_t cf_rgb(int c) {
  switch (c) {
    case CF_C_INK: return 0u;
    case CF_C_GRID_MAJOR: return 176u | 176u << 8 | 176u << 16;
    case CF_C_GRID_MINOR: return 204u | 204u << 8 | 204u << 16;
    case CF_C_BORDER: return 128u | 128u << 8 | 128u << 16;
    case CF_C_SERIES + 0: return 31u | 119u << 8 | 180u << 16;
    case CF_C_SERIES + 1: return 255u | 127u << 8 | 14u << 16;
    case CF_C_SERIES + 2: return 44u | 160u << 8 | 44u << 16;
    case CF_C_SERIES + 3: return 214u | 39u << 8 | 40u << 16;
    case CF_C_SERIES + 4: return 148u | 103u << 8 | 189u << 16;
    case CF_C_SERIES + 5: return 140u | 86u << 8 | 75u << 16;
    case CF_C_SERIES + 6: return 227u | 119u << 8 | 194u << 16;
    case CF_C_SERIES + 7: return 127u | 127u << 8 | 127u << 16;
    case CF_C_SERIES + 8: return 188u | 189u << 8 | 34u << 16;
    case CF_C_SERIES + 9: return 23u | 190u << 8 | 207u << 16;
    default: return 0xffffffu;
  }
}

struct CfGeom {
  int W, H, s, t;        // frame, scale, curve thickness
  int X0, Y0, PW, PH;    // the plot rectangle is [X0, X0 + PW) x [Y0, Y0 + PH)
};

__host__ __device__ inline CfGeom cf_geom(int W, int H, int s, int t) {
  CfGeom G;
  G.W = W; G.H = H; G.s = s; G.t = t;
  G.X0 = CF_CELLS_LEFT * s; G.Y0 = CF_CELLS_TOP * s;
  G.PW = W - (CF_CELLS_LEFT + CF_CELLS_RIGHT) * s;
  G.PH = H - (CF_CELLS_TOP + CF_CELLS_BOTTOM) * s;
  return G;
}

// both axes are [0, 1.01]
__host__ __device__ inline int32_t cf_col(double x, int PW) {
  const double q = x / 1.01;
  const double v = q * (double)(PW - 1);
  return fig_clamp_round(v);
}
__host__ __device__ inline int32_t cf_row(double y, int PH) {
  const double d = 1.01 - y;
  const double q = d / 1.01;
  const double v = q * (double)(PH - 1);
  return fig_clamp_round(v);
}
__host__ __device__ inline bool cf_point_finite(const double* xy) { return ov_finite(xy[0]) && ov_finite(xy[1]); }

// x over the finite points of a series must not decrease or must not increase.  *rev = 1 for a series that decreases somewhere (it is
// taken in reversed order); *bad = the index of the first point that turns back.
__host__ __device__ inline int cf_series_check(const double* xy, int n, int* rev, int* bad) {
  int dir = 0;
  bool have = false;
  double prev = 0;
  *rev = 0; *bad = -1;
  for (int i = 0; i < n; i++) {
    if (!cf_point_finite(xy + (size_t)2 * i)) continue;
    const double x = xy[(size_t)2 * i];
    if (have && x != prev) {
      const int d = x > prev ? 1 : -1;
      if (dir == 0) dir = d;
      else if (d != dir) { *bad = i; return CF_CHECK_NOT_MONOTONE; }
    }
    prev = x; have = true;
  }
  *rev = dir < 0;
  return CF_CHECK_OK;
}

// ---- the run merge: one statement after the other (the prepare kernel computes the same with a workgroup) ----
// Point i of a series in drawing order (reversed when rev) is kept when it is finite and the first, the last, the first of the lowest
// rows or the first of the highest rows of its RUN: a maximal stretch of consecutive finite points of one column.  out[CF_PT] per kept
// point; returns their number (at most n).
__host__ __device__ inline int cf_merge_series(const double* xy, int n, int rev, int PW, int PH, int32_t* out) {
  int m = 0, i = 0;
  bool prev_finite = false;
  while (i < n) {
    const double* p = xy + (size_t)2 * (rev ? n - 1 - i : i);
    if (!cf_point_finite(p)) { prev_finite = false; i++; continue; }
    const int col = cf_col(p[0], PW);
    int j = i, lo = 0, hi = 0, ilo = i, ihi = i;
    for (; j < n; j++) {
      const double* q = xy + (size_t)2 * (rev ? n - 1 - j : j);
      if (!cf_point_finite(q) || cf_col(q[0], PW) != col) break;
      const int r = cf_row(q[1], PH);
      if (j == i || r < lo) { lo = r; ilo = j; }
      if (j == i || r > hi) { hi = r; ihi = j; }
    }
    for (int k = i; k < j; k++) {
      if (k != i && k != j - 1 && k != ilo && k != ihi) continue;
      const double* q = xy + (size_t)2 * (rev ? n - 1 - k : k);
      out[(size_t)m * CF_PT + CF_PT_COL] = col;
      out[(size_t)m * CF_PT + CF_PT_ROW] = cf_row(q[1], PH);
      out[(size_t)m * CF_PT + CF_PT_JOIN] = k == i ? (prev_finite ? 1 : 0) : 1;
      m++;
    }
    prev_finite = true;
    i = j;
  }
  return m;
}

// ---- records ----

__host__ __device__ inline int cf_strlen(const uint8_t* s, int cap) {
  int n = 0;
  while (n < cap && s[n]) n++;
  return n;
}

// What a figure is besides its points (the device copies of the caller's structs, with the places of its series, marks and points)
struct CfFigure {
  int32_t n_series, n_marks, series0, marks0, point0, corner, minor_x, minor_y;
  uint8_t x_title[32], y_title[32];
};
struct CfSeries {
  int32_t n, colour, off, rev;      // off: first point of the series among the figure's
  uint8_t text[64];
};
struct CfMark {
  int32_t series, point;
  uint8_t text[16];
};

// All records of a figure in table order.  xy: the figure's points (series k at xy + 2 off_k).
__host__ __device__ inline int cf_records(const CfGeom& G, const CfFigure& F, const CfSeries* ser, const CfMark* marks, const double* xy, int32_t* rec, int cap) {
  Recs R{rec, cap, 0};
  const int s = G.s, W = G.W, H = G.H, X0 = G.X0, Y0 = G.Y0, PW = G.PW, PH = G.PH, b = (s + 1) / 2;
  const Clip frame{0, 0, W - 1, H - 1}, plot{X0, Y0, X0 + PW - 1, Y0 + PH - 1};
  // 1. spines: left, bottom
  rec_box<CfRec>(R, CF_KIND_LINE, X0 - s, Y0, X0 - 1, Y0 + PH + s - 1, frame, 0, 0);
  rec_box<CfRec>(R, CF_KIND_LINE, X0, Y0 + PH, X0 + PW - 1, Y0 + PH + s - 1, frame, 0, 0);
  // 2. major ticks with their labels and grid lines: x axis, then y axis, 0.0 .. 1.0
  for (int axis = 0; axis < 2; axis++)
    for (int k = 0; k <= 5; k++) {
      const int milli = 200 * k;
      const double v = (double)milli / 1000.0;
      const uint8_t ch[3] = {(uint8_t)('0' + k / 5), '.', (uint8_t)('0' + 2 * k % 10)};
      if (axis == 0) {
        const int x = X0 + cf_col(v, PW);
        rec_box<CfRec>(R, CF_KIND_LINE, x - s / 2, Y0 + PH + s, x - s / 2 + s - 1, Y0 + PH + 4 * s - 1, frame, milli, 0);
        rec_text<CfRec>(R, CF_KIND_TEXT, s, x - (17 * s) / 2, Y0 + PH + 5 * s, ch, 3, 0, frame, milli);
        rec_box<CfRec>(R, CF_KIND_GRID_MAJOR, x, Y0, x + b - 1, Y0 + PH - 1, plot, milli, 0);
      } else {
        const int y = Y0 + cf_row(v, PH);
        rec_box<CfRec>(R, CF_KIND_LINE, X0 - 4 * s, y - s / 2, X0 - s - 1, y - s / 2 + s - 1, frame, milli, 1);
        rec_text<CfRec>(R, CF_KIND_TEXT, s, X0 - 22 * s, y - 3 * s, ch, 3, 0, frame, milli);
        rec_box<CfRec>(R, CF_KIND_GRID_MAJOR, X0, y, X0 + PW - 1, y + b - 1, plot, milli, 1);
      }
    }
  // 3. minor grid lines: the multiples of the step up to 1000 that are no major tick
  for (int axis = 0; axis < 2; axis++) {
    const int step = axis ? F.minor_y : F.minor_x;
    if (step <= 0) continue;
    for (int milli = step; milli <= 1000; milli += step) {
      if (milli % 200 == 0) continue;
      const double v = (double)milli / 1000.0;
      if (axis == 0) { const int x = X0 + cf_col(v, PW); rec_box<CfRec>(R, CF_KIND_GRID_MINOR, x, Y0, x + b - 1, Y0 + PH - 1, plot, milli, 0); }
      else { const int y = Y0 + cf_row(v, PH); rec_box<CfRec>(R, CF_KIND_GRID_MINOR, X0, y, X0 + PW - 1, y + b - 1, plot, milli, 1); }
    }
  }
  // 4. axis titles
  const int nx = cf_strlen(F.x_title, CF_TITLE_MAX), ny = cf_strlen(F.y_title, CF_TITLE_MAX);
  if (nx) rec_text<CfRec>(R, CF_KIND_TEXT, s, X0 + (PW - text_width(nx, s)) / 2, Y0 + PH + 14 * s, F.x_title, nx, 0, frame, 0);
  if (ny) rec_text<CfRec>(R, CF_KIND_TEXT, s, s, Y0 + (PH - text_width(ny, s)) / 2, F.y_title, ny, 1, frame, 0);
  // 5. legend: the box, then a swatch and a text per series
  const int K = F.n_series;
  if (K > 0) {
    int L = 0;
    for (int k = 0; k < K; k++) { const int n = cf_strlen(ser[k].text, CF_TEXT_MAX); L = n > L ? n : L; }
    const int BW = (L ? text_width(L, s) : 0) + 16 * s, BH = 9 * s * K + 4 * s;
    const int bx = F.corner == CF_LEGEND_LOWER_RIGHT ? X0 + PW - 3 * s - BW : X0 + 3 * s, by = Y0 + PH - 3 * s - BH;
    rec_box<CfRec>(R, CF_KIND_LEGEND_BOX, bx, by, bx + BW - 1, by + BH - 1, frame, BW, BH);
    for (int k = 0; k < K; k++) {
      const int ty = by + 3 * s + 9 * s * k;
      rec_box<CfRec>(R, CF_KIND_SWATCH, bx + 3 * s, ty + 2 * s, bx + 11 * s - 1, ty + 5 * s - 1, frame, k, ser[k].colour);
      rec_text<CfRec>(R, CF_KIND_LEGEND_TEXT, s, bx + 13 * s, ty, ser[k].text, cf_strlen(ser[k].text, CF_TEXT_MAX), 0, frame, k);
    }
  }
  // 6. marks: text, marker, leader each
  const int M = F.n_marks;
  for (int i = 0; i < M; i++) {
    const CfMark& mk = marks[i];
    const CfSeries& S = ser[mk.series];
    const double* p = xy + (size_t)2 * ((size_t)S.off + (size_t)mk.point);
    const int n = cf_strlen(mk.text, CF_MARK_TEXT_MAX);
    if (!cf_point_finite(p)) {                                          // nothing of it can be seen
      const Clip none{0, 0, -1, -1};
      rec_text<CfRec>(R, CF_KIND_MARK_TEXT, s, 0, 0, mk.text, n, 0, none, i);
      rec_box<CfRec>(R, CF_KIND_MARKER, 0, 0, -1, -1, none, 0, 0);
      rec_box<CfRec>(R, CF_KIND_LEADER, 0, 0, -1, -1, none, 0, 0);
      continue;
    }
    const int px = X0 + cf_col(p[0], PW), py = Y0 + cf_row(p[1], PH), wu = text_width(n, s), rad = 2 * s;
    int ax, ay, ox;
    if (F.corner == CF_LEGEND_LOWER_RIGHT) { ax = px + (M - i) * 6 * s; ay = py + (i + 1) * 10 * s; ox = ax; }
    else { ax = px - 8 * s; ay = py + ((i < 3 ? i : 3) + 1) * 10 * s; ox = ax - wu + 1; }
    rec_text<CfRec>(R, CF_KIND_MARK_TEXT, s, ox, ay, mk.text, n, 0, frame, i);
    rec_box<CfRec>(R, CF_KIND_MARKER, px - rad, py - rad, px + rad, py + rad, frame, px, py);
    // the leader from the text's corner (ox, oy of the record) to the point (value, aux): the box around both, a pixel wider
    int32_t* r = rec_box<CfRec>(R, CF_KIND_LEADER, (ax < px ? ax : px) - 1, (ay < py ? ay : py) - 1, (ax < px ? px : ax) + 1, (ay < py ? py : ay) + 1, frame, px, py);
    if (r) { r[REC_OX] = ax; r[REC_OY] = ay; }
  }
  return R.n;
}

// ---- one pixel ----

// the colour index record r gives pixel (px, py) of its visible box, -1 when it does not cover it
__host__ __device__ inline int cf_record_colour(const int32_t* r, int s, int px, int py) {
  const int b = (s + 1) / 2;
  switch (r[REC_KIND]) {
    case CF_KIND_LEGEND_TEXT: case CF_KIND_MARK_TEXT: case CF_KIND_TEXT: return text_covers<CfRec, cf_glyph>(r, s, px, py) ? CF_C_INK : -1;
    case CF_KIND_SWATCH: return CF_C_SERIES + r[CF_R_AUX];
    case CF_KIND_LEGEND_BOX: {
      const int rx = px - r[REC_OX], ry = py - r[REC_OY];
      return rx < b || ry < b || rx >= r[CF_R_VALUE] - b || ry >= r[CF_R_AUX] - b ? CF_C_BORDER : CF_C_WHITE;
    }
    case CF_KIND_MARKER: {
      const int64_t dx = px - r[CF_R_VALUE], dy = py - r[CF_R_AUX], rad = r[CF_R_VALUE] - r[REC_OX];
      return dx * dx + dy * dy <= rad * rad ? CF_C_INK : -1;
    }
    case CF_KIND_LEADER: return ov_segment_covers(px, py, r[REC_OX], r[REC_OY], r[CF_R_VALUE], r[CF_R_AUX], 1) ? CF_C_INK : -1;
    case CF_KIND_LINE: return CF_C_INK;
    case CF_KIND_GRID_MAJOR: return CF_C_GRID_MAJOR;
    case CF_KIND_GRID_MINOR: {                                          // dotted: one block of b pixels in three along the line
      const int along = r[CF_R_AUX] ? px - r[REC_OX] : py - r[REC_OY];
      return (along / b) % 3 == 0 ? CF_C_GRID_MINOR : -1;
    }
    default: return -1;
  }
}

// Over the records: for each of the pixels (px + e, py), e < n <= 4, the smallest kind above the curves that covers it (over[e], colour
// oc[e]) and the smallest below them (under[e], uc[e]); CF_KIND_NONE when there is none
__host__ __device__ inline void cf_records4(const int32_t* recs, int nrec, int s, int px, int py, int n, int* over, int* oc, int* under, int* uc) {
  for (int e = 0; e < 4; e++) { over[e] = CF_KIND_NONE; under[e] = CF_KIND_NONE; oc[e] = CF_C_WHITE; uc[e] = CF_C_WHITE; }
  for (int k = 0; k < nrec; k++) {
    const int32_t* r = recs + (size_t)k * CF_REC;
    const int x0 = r[REC_X0], x1 = r[REC_X1];
    if (px + n - 1 < x0 || px > x1 || py < r[REC_Y0] || py > r[REC_Y1]) continue;
    const int kind = r[REC_KIND];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int e = 0; e < 4; e++) {
      if (e >= n || px + e < x0 || px + e > x1) continue;
      if (kind < CF_KIND_CURVES ? kind >= over[e] : kind >= under[e]) continue;   // (no two records of one kind give a pixel different colours)
      const int c = cf_record_colour(r, s, px + e, py);
      if (c < 0) continue;
      if (kind < CF_KIND_CURVES) { over[e] = kind; oc[e] = c; } else { under[e] = kind; uc[e] = c; }
    }
  }
}

// A series as the pixels see it: merged point i at pts[(i - base) * CF_PT], for the i the passed items touch
struct CfSeriesView {
  const int32_t* pts;
  int base, m, colour;
};

// Item i of a series is the segment from point i - 1 to point i when point i is joined, else the dot of point i.  The items that can
// cover a pixel of columns [pa, pb] (rectangle coordinates) are [*i0, *i1]: col_i >= pa - h and col_{i-1} <= pb + h, h = (t + 1) / 2.
// Empty: *i0 > *i1.  [lo, hi) is a range of points known to hold both bounds ([0, m), or bounds *k0, *k1 found for columns that contain
// [pa, pb]).  The points the items touch are max(*i0 - 1, 0) .. *i1.
__host__ __device__ inline void cf_item_range(const CfSeriesView& V, int lo, int hi, int t, int pa, int pb, int* i0, int* i1, int* k0_out, int* k1_out) {
  if (V.m <= 0) { *i0 = 0; *i1 = -1; *k0_out = 0; *k1_out = 0; return; }
  const int h = (t + 1) / 2;
  const int k0 = col_lower_bound(V.pts, CF_PT, V.base, lo, hi, pa - h), k1 = col_lower_bound(V.pts, CF_PT, V.base, lo, hi, pb + h + 1);
  *i0 = k0;
  *i1 = k1 < V.m ? k1 : V.m - 1;
  *k0_out = k0; *k1_out = k1;
}

// which of the pixels (qx0 + e, qy), e < n <= 4 (rectangle coordinates; columns outside [0, PW) never) the items [i0, i1] cover: rule 2
// of the overlay.  [rlo, rhi] holds the rows of every point the items touch.  Bit e of the result.
__host__ __device__ inline unsigned cf_curve_mask(const CfSeriesView& V, int t, int PW, int qx0, int n, int qy, int i0, int i1, int rlo, int rhi) {
  const int h = (t + 1) / 2;
  if (qy < rlo - h || qy > rhi + h) return 0;
  const unsigned all = (1u << n) - 1u;
  unsigned m = 0;
  for (int i = i0; i <= i1; i++) {
    const int32_t* b = V.pts + (size_t)(i - V.base) * CF_PT;
    const int32_t* a = b[CF_PT_JOIN] ? b - CF_PT : b;
    m |= quad_segment_mask(qx0, n, qy, PW, a[CF_PT_COL], a[CF_PT_ROW], b[CF_PT_COL], b[CF_PT_ROW], t);
    if (m == all) break;
  }
  return m;
}

// The colour indices out[e] of the frame pixels (px + e, py), e < n <= 4, all in the frame, from the whole tables: K series views over
// all their points, the records.  The statement the host program runs; the render kernel forms the same from its staged parts.
__host__ __device__ inline void cf_pixels4(const CfGeom& G, const CfSeriesView* ser, int K, const int32_t* recs, int nrec, int px, int py, int n, int* out) {
  int over[4], oc[4], under[4], uc[4], curve[4] = {-1, -1, -1, -1};
  cf_records4(recs, nrec, G.s, px, py, n, over, oc, under, uc);
  const int qy = py - G.Y0;
  if (qy >= 0 && qy < G.PH)
    for (int k = 0; k < K; k++) {                                       // the later series overwrites
      int i0, i1, k0, k1;
      cf_item_range(ser[k], 0, ser[k].m, G.t, px - G.X0, px + n - 1 - G.X0, &i0, &i1, &k0, &k1);
      if (i0 > i1) continue;
      const unsigned mask = cf_curve_mask(ser[k], G.t, G.PW, px - G.X0, n, qy, i0, i1, -65536, 65536);
      for (int e = 0; e < 4; e++)
        if (mask >> e & 1) curve[e] = CF_C_SERIES + ser[k].colour;
    }
  for (int e = 0; e < n; e++) out[e] = over[e] != CF_KIND_NONE ? oc[e] : (curve[e] >= 0 ? curve[e] : uc[e]);
}

}  // namespace vbt
