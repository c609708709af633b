// Curve figure on the device (gfx950): eval.py's precision-recall and ROC figures of N sets of curves rendered into N RGB24 frames
// that stay in device memory (include/vbt_hip.h, "Curve figure"; reference eval.py:218-468).  Two kernels:
//   curve_figure_prepare_kernel, once per vbt_curve_figure_set: a workgroup per figure.  Per series the whole workgroup maps the
//     points to (column, row), finds the runs of one column - every lane scans a contiguous share of the points, the shares are joined
//     through LDS - reduces each run's lowest and highest row with 64-bit atomic minima keyed (row, index), and compacts the kept
//     points (first, lowest, highest, last of a run) by a workgroup prefix sum.  One lane then writes the figure's records.
//   curve_figure_render_kernel, once per vbt_curve_figure_render: grid (tile of the frame, figure).  A gather with one writer per
//     pixel: a lane per series finds the merged points the tile's columns can meet, the workgroup stages them and the records that
//     touch the tile in LDS (or reads global memory when they do not fit), and every lane decides four adjacent pixels of two rows
//     by the contract's test (curve_figure_core.h) and stores them once.  Nothing is read from the frames.
// Shared with figure.hip: the tile's rectangle, the record staging and the RGB24 store (raster_tile.h), the handle's host side (figure_host.h).
// Compiled without FMA contraction (-ffp-contract=off, as every unit here: build.py), so the doubles of the contract are the ones a
// host compiler forms from curve_figure_core.h.
#include <algorithm>
#include <climits>

#include "curve_figure_core.h"
#include "figure_host.h"
#include "raster_tile.h"

namespace vbt {

constexpr int CF_THREADS = RASTER_THREADS;
constexpr int CF_TILE_H = 8;                            // two rows per lane (profiles/curve_figure.md)
constexpr int CF_ROWS_PER_LANE = CF_TILE_H / 4;
constexpr int32_t CF_NO_ROW = INT32_MIN;                // the row of a non-finite point in the workspace

static_assert(sizeof(CfFigure) == sizeof(vbt_curve_figure_desc) && sizeof(CfFigure) == 96, "figure layout");
static_assert(sizeof(CfSeries) == 80 && sizeof(vbt_curve_series) == 72, "series layout");
static_assert(sizeof(CfMark) == sizeof(vbt_curve_mark) && sizeof(CfMark) == 24, "mark layout");

struct CfPrepArgs {
  const CfFigure* figs;
  const CfSeries* series;
  const CfMark* marks;
  const double* xy;                 // the points of all figures
  int32_t *ws_col, *ws_row;         // [max_figures][max_points]
  unsigned long long *ws_lo, *ws_hi;   // [max_figures][max_points]: at a run's first point, (row key << 32 | index) of its lowest / highest row
  int32_t* pts;                     // [max_figures][max_points][CF_PT]: series k's merged points from its input offset
  int32_t* cnt;                     // [max_figures][CF_MAX_SERIES]
  int32_t* recs;                    // [max_figures][rec_cap][CF_REC]
  int32_t* nrec;                    // [max_figures]
  CfGeom G;
  int max_points, rec_cap;
};

struct CfRenderArgs {
  const CfFigure* figs;
  const CfSeries* series;
  const int32_t* pts;
  const int32_t* cnt;
  const int32_t* recs;
  const int32_t* nrec;
  uint8_t* frames;                  // frame of figure fig0 + blockIdx.y at frames + blockIdx.y * frame_bytes
  size_t frame_bytes;
  CfGeom G;
  int max_points, rec_cap, fig0, tiles_x;
  int words;                        // W % 4 == 0 and a 4-aligned base: four pixels go out as three 32-bit stores
};

__device__ __forceinline__ unsigned long long cf_load_key(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // (written by atomics of other lanes of the workgroup)
}

__global__ __launch_bounds__(CF_THREADS) void curve_figure_prepare_kernel(CfPrepArgs A) {
  __shared__ int s_last[CF_THREADS], s_cnt[CF_THREADS];
  const int fig = blockIdx.x, tid = threadIdx.x;
  const CfFigure& F = A.figs[fig];
  const CfSeries* ser = A.series + F.series0;
  const double* fxy = A.xy + (size_t)2 * F.point0;
  for (int k = 0; k < F.n_series; k++) {
    const int n = ser[k].n, rev = ser[k].rev;
    const size_t at = (size_t)fig * A.max_points + (size_t)ser[k].off;
    const double* xy = fxy + (size_t)2 * ser[k].off;
    int32_t *col = A.ws_col + at, *row = A.ws_row + at, *out = A.pts + at * CF_PT;
    unsigned long long *lo = A.ws_lo + at, *hi = A.ws_hi + at;
    for (int i = tid; i < n; i += CF_THREADS) {
      const double* p = xy + (size_t)2 * (rev ? n - 1 - i : i);
      const bool fin = cf_point_finite(p);
      col[i] = fin ? cf_col(p[0], A.G.PW) : 0;
      row[i] = fin ? cf_row(p[1], A.G.PH) : CF_NO_ROW;
      lo[i] = ~0ull; hi[i] = ~0ull;
    }
    __syncthreads();
    // a lane's share: points [a, b)
    const int per = (n + CF_THREADS - 1) / CF_THREADS;
    const int a = min(tid * per, n), b = min(a + per, n);
    auto starts = [&](int i) { return row[i] != CF_NO_ROW && (i == 0 || row[i - 1] == CF_NO_ROW || col[i - 1] != col[i]); };
    auto ends = [&](int i) { return i == n - 1 || row[i + 1] == CF_NO_ROW || col[i + 1] != col[i]; };
    int last = -1;
    for (int i = a; i < b; i++)
      if (starts(i)) last = i;
    s_last[tid] = last;
    __syncthreads();
    int carry = -1;                                                    // the first point of the run that reaches into this share
    for (int j = tid - 1; j >= 0 && carry < 0; j--) carry = s_last[j];
    int rs = carry;
    for (int i = a; i < b; i++) {
      if (row[i] == CF_NO_ROW) continue;
      if (starts(i)) rs = i;
      atomicMin(lo + rs, (unsigned long long)(uint32_t)(row[i] + 32768) << 32 | (uint32_t)i);
      atomicMin(hi + rs, (unsigned long long)(uint32_t)(32768 - row[i]) << 32 | (uint32_t)i);
    }
    __threadfence();
    __syncthreads();
    auto kept = [&](int i, int run) {
      return starts(i) || ends(i) || (uint32_t)cf_load_key(lo + run) == (uint32_t)i || (uint32_t)cf_load_key(hi + run) == (uint32_t)i;
    };
    int c = 0;
    rs = carry;
    for (int i = a; i < b; i++) {
      if (row[i] == CF_NO_ROW) continue;
      if (starts(i)) rs = i;
      c += kept(i, rs) ? 1 : 0;
    }
    s_cnt[tid] = c;
    __syncthreads();
    int base = 0;
    for (int j = 0; j < tid; j++) base += s_cnt[j];
    if (tid == CF_THREADS - 1) A.cnt[(size_t)fig * CF_MAX_SERIES + k] = base + c;
    rs = carry;                                                        // (out is an array of its own: no lane reads what another writes here)
    for (int i = a; i < b; i++) {
      if (row[i] == CF_NO_ROW) continue;
      const bool st = starts(i);
      if (st) rs = i;
      if (!kept(i, rs)) continue;
      out[(size_t)base * CF_PT + CF_PT_COL] = col[i];
      out[(size_t)base * CF_PT + CF_PT_ROW] = row[i];
      out[(size_t)base * CF_PT + CF_PT_JOIN] = st ? (i > 0 && row[i - 1] != CF_NO_ROW ? 1 : 0) : 1;
      base++;
    }
    __syncthreads();                                                   // s_last and s_cnt are the next series'
  }
  if (tid == 0)
    A.nrec[fig] = cf_records(A.G, F, ser, A.marks + F.marks0, fxy, A.recs + (size_t)fig * A.rec_cap * CF_REC, A.rec_cap);
}

// what the workgroup knows of its series: LDS, read as broadcasts
struct CfTileSeries {
  int k0[CF_MAX_SERIES], k1[CF_MAX_SERIES];       // the bounds cf_item_range found for the tile's columns
  int first[CF_MAX_SERIES], np[CF_MAX_SERIES];    // the points the tile's items touch: first .. first + np - 1
  int m[CF_MAX_SERIES], colour[CF_MAX_SERIES], off[CF_MAX_SERIES];
};

// the tile's pixels from pointers the compiler knows the address space of.  staged: pts holds, series after series, the np points of
// each from its `first`; else pts is the figure's whole table.
__device__ __forceinline__ void curve_figure_render_tile(const CfRenderArgs& A, const CfTileSeries& S, int K, const int32_t* pts, bool staged,
                                                         const int32_t* recs, int nrec, int x_lo, int y_lo, uint8_t* frame) {
  const CfGeom& G = A.G;
  const int px = x_lo + (int)(threadIdx.x & 63) * 4;
  if (px >= G.W) return;
  const int last = px + 3 < G.W ? px + 3 : G.W - 1, n = last - px + 1;
  const int wave = (int)(threadIdx.x >> 6);
  // the curves first, series after series, the later one over the earlier: a colour index per pixel, 0xff where no curve is
  uint32_t cur[CF_ROWS_PER_LANE];
#pragma unroll
  for (int j = 0; j < CF_ROWS_PER_LANE; j++) cur[j] = 0xffffffffu;
  int at = 0;
  for (int k = 0; k < K; k++) {
    const CfSeriesView V{staged ? pts + (size_t)at * CF_PT : pts + (size_t)S.off[k] * CF_PT, staged ? S.first[k] : 0, S.m[k], S.colour[k]};
    at += S.np[k];
    if (S.np[k] == 0) continue;
    int i0, i1, q0, q1;
    cf_item_range(V, S.k0[k], S.k1[k], G.t, px - G.X0, last - G.X0, &i0, &i1, &q0, &q1);
    if (i0 > i1) continue;
    // the rows the lane's own items reach, once for all its pixel rows
    int rlo = 65536, rhi = -65536;
    for (int i = i0 > 0 ? i0 - 1 : 0; i <= i1; i++) {
      const int v = V.pts[(size_t)(i - V.base) * CF_PT + CF_PT_ROW];
      rlo = v < rlo ? v : rlo; rhi = v > rhi ? v : rhi;
    }
    const uint32_t c = (uint32_t)(CF_C_SERIES + V.colour);
#pragma unroll
    for (int j = 0; j < CF_ROWS_PER_LANE; j++) {
      const int qy = y_lo + wave + 4 * j - G.Y0;
      if (qy < 0 || qy >= G.PH) continue;
      const unsigned mask = cf_curve_mask(V, G.t, G.PW, px - G.X0, n, qy, i0, i1, rlo, rhi);
#pragma unroll
      for (int e = 0; e < 4; e++)
        if (mask >> e & 1) cur[j] = (cur[j] & ~(0xffu << (8 * e))) | c << (8 * e);
    }
  }
#pragma unroll
  for (int j = 0; j < CF_ROWS_PER_LANE; j++) {                      // wavefront w takes rows w, w + 4, ...
    const int py = y_lo + wave + 4 * j;
    if (py >= G.H) return;
    uint8_t* p = frame + ((size_t)py * G.W + px) * 3;
    int over[4], oc[4], under[4], uc[4];
    cf_records4(recs, nrec, G.s, px, py, n, over, oc, under, uc);
    uint32_t rgb[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int cc = (int)(cur[j] >> (8 * e) & 0xffu);
      rgb[e] = cf_rgb(over[e] != CF_KIND_NONE ? oc[e] : (cc != 0xff ? cc : uc[e]));
    }
    store_rgb24x4(p, rgb, n, A.words);                              // W % 4 == 0: px + 3 < W, and p is 4-aligned
  }
}

__global__ __launch_bounds__(CF_THREADS, 4) void curve_figure_render_kernel(CfRenderArgs A) {
  __shared__ int32_t s_pts[VBT_CURVE_FIGURE_STAGE_POINTS * CF_PT];
  __shared__ int32_t s_recs[VBT_CURVE_FIGURE_STAGE_RECORDS * CF_REC];
  __shared__ CfTileSeries S;
  __shared__ int s_found;
  const CfGeom& G = A.G;
  const int fig = A.fig0 + (int)blockIdx.y, tid = threadIdx.x;
  const int K = A.figs[fig].n_series, series0 = A.figs[fig].series0, nrec = A.nrec[fig];
  const int32_t* gp = A.pts + (size_t)fig * A.max_points * CF_PT;
  const int32_t* gr = A.recs + (size_t)fig * A.rec_cap * CF_REC;
  const TileBox box = tile_box<CF_TILE_H>(A.tiles_x, G.W, G.H);
  if (tid == 0) s_found = 0;
  // the points of the tile's columns: a lane per series, on the whole table
  if (tid < K) {
    const CfSeries& sr = A.series[series0 + tid];
    const int m = A.cnt[(size_t)fig * CF_MAX_SERIES + tid];
    const CfSeriesView V{gp + (size_t)sr.off * CF_PT, 0, m, sr.colour};
    int i0, i1, k0, k1;
    cf_item_range(V, 0, m, G.t, box.x_lo - G.X0, box.x_hi - G.X0, &i0, &i1, &k0, &k1);
    const int first = i0 <= i1 ? (i0 > 0 ? i0 - 1 : 0) : 0;
    S.k0[tid] = k0; S.k1[tid] = k1; S.first[tid] = first; S.np[tid] = i0 <= i1 ? i1 - first + 1 : 0;
    S.m[tid] = m; S.colour[tid] = sr.colour; S.off[tid] = sr.off;
  }
  __syncthreads();
  int total = 0;
  for (int k = 0; k < K; k++) total += S.np[k];
  const bool pts_staged = total <= VBT_CURVE_FIGURE_STAGE_POINTS;
  if (pts_staged) {
    int at = 0;
    for (int k = 0; k < K; k++) {
      const int32_t* src = gp + ((size_t)S.off[k] + (size_t)S.first[k]) * CF_PT;
      for (int i = tid; i < S.np[k] * CF_PT; i += CF_THREADS) s_pts[at * CF_PT + i] = src[i];
      at += S.np[k];
    }
  }
  stage_tile_records<CF_REC>(gr, nrec, box, s_recs, VBT_CURVE_FIGURE_STAGE_RECORDS, &s_found);
  __syncthreads();
  const int found = s_found;
  uint8_t* frame = A.frames + (size_t)blockIdx.y * A.frame_bytes;
  if (pts_staged && found <= VBT_CURVE_FIGURE_STAGE_RECORDS)
    curve_figure_render_tile(A, S, K, s_pts, true, s_recs, found, box.x_lo, box.y_lo, frame);
  else                                                              // long curves or a crowded tile: the same statements on global memory
    curve_figure_render_tile(A, S, K, gp, false, gr, nrec, box.x_lo, box.y_lo, frame);
}

}  // namespace vbt

using namespace vbt;

struct vbt_curve_figure : FigureHandle {   // blob: upload (figures | series | marks | points) | workspace | pts | recs | nrec | cnt
  vbt_curve_figure_params prm{};
  CfGeom G{};
  int32_t *d_col = nullptr, *d_row = nullptr, *d_pts = nullptr, *d_cnt = nullptr;
  unsigned long long *d_lo = nullptr, *d_hi = nullptr;
  const CfFigure* d_figs = nullptr;    // inside the upload of the last set
  const CfSeries* d_series = nullptr;
  std::vector<CfFigure> figs;          // the host's copies
  std::vector<CfSeries> series;
};

namespace {

int check_curve_figure_params(const vbt_curve_figure_params& p) {
  const char* who = "vbt_curve_figure_create";
  if (int rc = check_canvas(who, p.width, p.height, p.scale, p.thickness)) return rc;
  if (p.max_figures < 1 || p.max_figures > CF_MAX_FIGURES) { set_error("%s: max_figures %d outside 1..%d", who, p.max_figures, (int)CF_MAX_FIGURES); return VBT_ERR_ARG; }
  if (p.max_series < 1 || p.max_series > CF_MAX_SERIES) { set_error("%s: max_series %d outside 1..%d", who, p.max_series, (int)CF_MAX_SERIES); return VBT_ERR_ARG; }
  if (p.max_points < 1 || p.max_points > CF_MAX_POINTS) { set_error("%s: max_points %d outside 1..%d", who, p.max_points, (int)CF_MAX_POINTS); return VBT_ERR_ARG; }
  if (p.max_marks < 0 || p.max_marks > CF_MAX_MARKS) { set_error("%s: max_marks %d outside 0..%d", who, p.max_marks, (int)CF_MAX_MARKS); return VBT_ERR_ARG; }
  if ((long)p.max_figures * p.max_points > (1l << 26)) {
    set_error("%s: %d figures of %d points: above 2^26 points in all", who, p.max_figures, p.max_points);
    return VBT_ERR_ARG;
  }
  return check_plot_rect(who, cf_geom(p.width, p.height, p.scale, p.thickness), CF_MIN_PLOT);
}

// 0: n < cap bytes of 0x20..0x7E and a NUL; 1: no NUL; 2: a byte outside (at *at)
int check_text(const char* s, int cap, int* at) {
  for (int i = 0; i < cap; i++) {
    const unsigned char c = (unsigned char)s[i];
    if (c == 0) return 0;
    if (c < CF_FONT_FIRST || c > CF_FONT_LAST) { *at = i; return 2; }
  }
  return 1;
}

struct CurveTotals { size_t series = 0, marks = 0, points = 0; };

// the refusals of vbt_curve_figure_set that need no handle and no device; the totals and each series' direction (rev) on VBT_OK
int check_curve_figure_set(int n, const vbt_curve_figure_desc* figs, const vbt_curve_series* series, const double* xy, const vbt_curve_mark* marks,
                           CurveTotals* tot, std::vector<int>* revs) {
  const char* who = "vbt_curve_figure_set";
  if (n < 0 || (n > 0 && !figs)) { set_error("%s: bad argument (n %d, figs %p)", who, n, (const void*)figs); return VBT_ERR_ARG; }
  if (n > CF_MAX_FIGURES) { set_error("%s: %d figures, above %d", who, n, (int)CF_MAX_FIGURES); return VBT_ERR_CAPACITY; }
  CurveTotals T;
  for (int f = 0; f < n; f++) {
    const vbt_curve_figure_desc& d = figs[f];
    if (d.n_series < 0 || d.n_marks < 0) { set_error("%s: figure %d has a negative count (%d series, %d marks)", who, f, d.n_series, d.n_marks); return VBT_ERR_ARG; }
    if (d.legend_corner != CF_LEGEND_LOWER_LEFT && d.legend_corner != CF_LEGEND_LOWER_RIGHT) { set_error("%s: figure %d: legend_corner %d is neither 0 nor 1", who, f, d.legend_corner); return VBT_ERR_ARG; }
    for (int a = 0; a < 2; a++) {
      const int step = a ? d.minor_y : d.minor_x;
      if (step != 0 && (step < CF_MINOR_MIN || step > CF_MINOR_MAX)) { set_error("%s: figure %d: minor_%c %d is neither 0 nor in %d..%d", who, f, a ? 'y' : 'x', step, (int)CF_MINOR_MIN, (int)CF_MINOR_MAX); return VBT_ERR_ARG; }
    }
    if (d.n_series > CF_MAX_SERIES) { set_error("%s: figure %d has %d series, above %d", who, f, d.n_series, (int)CF_MAX_SERIES); return VBT_ERR_CAPACITY; }
    if (d.n_marks > CF_MAX_MARKS) { set_error("%s: figure %d has %d marks, above %d", who, f, d.n_marks, (int)CF_MAX_MARKS); return VBT_ERR_CAPACITY; }
    T.series += (size_t)d.n_series; T.marks += (size_t)d.n_marks;
  }
  if ((T.series > 0 && !series) || (T.marks > 0 && !marks)) { set_error("%s: NULL series or marks", who); return VBT_ERR_ARG; }
  for (size_t k = 0; k < T.series; k++)
    if (series[k].n_points > 0 && !xy) { set_error("%s: NULL xy", who); return VBT_ERR_ARG; }
  revs->assign(T.series, 0);
  const vbt_curve_series* sr = series;
  const vbt_curve_mark* mk = marks;
  const double* p = xy;
  size_t sk = 0;
  for (int f = 0; f < n; f++) {
    const vbt_curve_figure_desc& d = figs[f];
    int at = 0;
    for (int a = 0; a < 2; a++)
      switch (check_text(a ? d.y_title : d.x_title, 32, &at)) {
        case 1: set_error("%s: figure %d: %c_title has no NUL within 32 bytes", who, f, a ? 'y' : 'x'); return VBT_ERR_ARG;
        case 2: set_error("%s: figure %d: %c_title holds byte 0x%02x at %d, outside 0x20..0x7E", who, f, a ? 'y' : 'x', (unsigned)(unsigned char)(a ? d.y_title : d.x_title)[at], at); return VBT_ERR_ARG;
        default: break;
      }
    size_t fig_points = 0;
    for (int k = 0; k < d.n_series; k++) {
      const vbt_curve_series& s = sr[k];
      if (s.n_points < 0) { set_error("%s: figure %d, series %d has a negative count (%d points)", who, f, k, s.n_points); return VBT_ERR_ARG; }
      fig_points += (size_t)s.n_points;
      if (fig_points > CF_MAX_POINTS) { set_error("%s: figure %d has more than %d points", who, f, (int)CF_MAX_POINTS); return VBT_ERR_CAPACITY; }
      if (s.colour < 0 || s.colour >= CF_PALETTE) { set_error("%s: figure %d, series %d: colour %d outside 0..%d", who, f, k, s.colour, (int)CF_PALETTE - 1); return VBT_ERR_ARG; }
      switch (check_text(s.text, 64, &at)) {
        case 1: set_error("%s: figure %d, series %d: text has no NUL within 64 bytes", who, f, k); return VBT_ERR_ARG;
        case 2: set_error("%s: figure %d, series %d: text holds byte 0x%02x at %d, outside 0x20..0x7E", who, f, k, (unsigned)(unsigned char)s.text[at], at); return VBT_ERR_ARG;
        default: break;
      }
      int rev = 0, bad = -1;
      if (cf_series_check(p, s.n_points, &rev, &bad) != CF_CHECK_OK) {
        set_error("%s: figure %d, series %d, point %d: x is not monotone (it neither never decreases nor never increases)", who, f, k, bad);
        return VBT_ERR_ARG;
      }
      (*revs)[sk + (size_t)k] = rev;
      p += (size_t)2 * s.n_points;
    }
    for (int i = 0; i < d.n_marks; i++) {
      const vbt_curve_mark& m = mk[i];
      if (m.series < 0 || m.series >= d.n_series) { set_error("%s: figure %d, mark %d names series %d of %d", who, f, i, m.series, d.n_series); return VBT_ERR_ARG; }
      if (m.point < 0 || m.point >= sr[m.series].n_points) { set_error("%s: figure %d, mark %d names point %d of series %d, which has %d", who, f, i, m.point, m.series, sr[m.series].n_points); return VBT_ERR_ARG; }
      switch (check_text(m.text, 16, &at)) {
        case 1: set_error("%s: figure %d, mark %d: text has no NUL within 16 bytes", who, f, i); return VBT_ERR_ARG;
        case 2: set_error("%s: figure %d, mark %d: text holds byte 0x%02x at %d, outside 0x20..0x7E", who, f, i, (unsigned)(unsigned char)m.text[at], at); return VBT_ERR_ARG;
        default: break;
      }
    }
    T.points += fig_points;
    sr += d.n_series; mk += d.n_marks; sk += (size_t)d.n_series;
  }
  *tot = T;
  return VBT_OK;
}

}  // namespace

extern "C" {

void vbt_curve_figure_default_params(vbt_curve_figure_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->width = 1120; p->height = 640; p->scale = 2; p->thickness = 2; p->max_figures = 16; p->max_series = 8; p->max_points = 131072; p->max_marks = 8;
}

int vbt_curve_figure_create(int device, const vbt_curve_figure_params* params, vbt_curve_figure** out) {
  if (!out) { set_error("vbt_curve_figure_create: out is NULL"); return VBT_ERR_ARG; }
  *out = nullptr;
  vbt_curve_figure_params p;
  vbt_curve_figure_default_params(&p);
  if (params) p = *params;
  if (int rc = check_curve_figure_params(p)) return rc;
  if (int rc = use_device("vbt_curve_figure_create", device, /*set_current=*/true)) return rc;
  std::unique_ptr<vbt_curve_figure> f(new vbt_curve_figure());
  f->device = device; f->prm = p; f->G = cf_geom(p.width, p.height, p.scale, p.thickness);
  f->rec_cap = CF_FIXED_RECS + 1 + 2 * p.max_series + 3 * p.max_marks;
  const size_t F = (size_t)p.max_figures, P = (size_t)p.max_points;
  FigCarver C;                                                          // the largest upload, at the blob's head
  C.add<uint8_t>(align64(F * sizeof(CfFigure)) + align64(F * p.max_series * sizeof(CfSeries)) + align64(F * p.max_marks * sizeof(CfMark)) + F * P * 16);
  const auto lo = C.add<unsigned long long>(F * P), hi = C.add<unsigned long long>(F * P);
  const auto col = C.add<int32_t>(F * P), row = C.add<int32_t>(F * P), pts = C.add<int32_t>(F * P * CF_PT);
  const auto recs = C.add<int32_t>(F * (size_t)f->rec_cap * CF_REC), nrec = C.add<int32_t>(F), cnt = C.add<int32_t>(F * CF_MAX_SERIES);
  if (f->blob.alloc(C.bytes()) != hipSuccess) {
    (void)hipGetLastError();
    set_error("vbt_curve_figure_create: the device cannot give %zu bytes for %d figures of %d points, %d series and %d marks", C.bytes(), p.max_figures,
              p.max_points, p.max_series, p.max_marks);
    return VBT_ERR_HIP;
  }
  f->d_lo = C.ptr(f->blob.get(), lo); f->d_hi = C.ptr(f->blob.get(), hi); f->d_col = C.ptr(f->blob.get(), col); f->d_row = C.ptr(f->blob.get(), row);
  f->d_pts = C.ptr(f->blob.get(), pts); f->d_recs = C.ptr(f->blob.get(), recs); f->d_nrec = C.ptr(f->blob.get(), nrec); f->d_cnt = C.ptr(f->blob.get(), cnt);
  *out = f.release();
  return VBT_OK;
}

void vbt_curve_figure_destroy(vbt_curve_figure* f) { delete f; }

int vbt_curve_figure_set(vbt_curve_figure* f, int n, const vbt_curve_figure_desc* figs, const vbt_curve_series* series, const double* xy,
                         const vbt_curve_mark* marks, void* stream) {
  CurveTotals T;
  std::vector<int> revs;
  if (int rc = check_curve_figure_set(n, figs, series, xy, marks, &T, &revs)) return rc;
  const char* who = "vbt_curve_figure_set";
  if (!f) { set_error("%s: handle is NULL", who); return VBT_ERR_ARG; }
  if (n > f->prm.max_figures) { set_error("%s: %d figures, the handle holds %d", who, n, f->prm.max_figures); return VBT_ERR_CAPACITY; }
  {
    const vbt_curve_series* sr = series;
    for (int i = 0; i < n; i++) {
      if (figs[i].n_series > f->prm.max_series) { set_error("%s: figure %d has %d series, the handle holds %d", who, i, figs[i].n_series, f->prm.max_series); return VBT_ERR_CAPACITY; }
      if (figs[i].n_marks > f->prm.max_marks) { set_error("%s: figure %d has %d marks, the handle holds %d", who, i, figs[i].n_marks, f->prm.max_marks); return VBT_ERR_CAPACITY; }
      size_t pts = 0;
      for (int k = 0; k < figs[i].n_series; k++) pts += (size_t)sr[k].n_points;
      if (pts > (size_t)f->prm.max_points) { set_error("%s: figure %d has %zu points, the handle holds %d", who, i, pts, f->prm.max_points); return VBT_ERR_CAPACITY; }
      sr += figs[i].n_series;
    }
  }
  VBT_HIP_CHECK(hipSetDevice(f->device));
  f->n = 0;
  if (n == 0) return VBT_OK;
  const size_t figs_b = align64((size_t)n * sizeof(CfFigure)), ser_b = align64(T.series * sizeof(CfSeries)), mk_b = align64(T.marks * sizeof(CfMark));
  std::vector<uint8_t> up(figs_b + ser_b + mk_b + T.points * 16, 0);
  CfFigure* hf = (CfFigure*)up.data();
  CfSeries* hs = (CfSeries*)(up.data() + figs_b);
  size_t s0 = 0, m0 = 0, p0 = 0;
  for (int i = 0; i < n; i++) {
    const vbt_curve_figure_desc& d = figs[i];
    CfFigure& o = hf[i];
    o.n_series = d.n_series; o.n_marks = d.n_marks; o.series0 = (int32_t)s0; o.marks0 = (int32_t)m0; o.point0 = (int32_t)p0;
    o.corner = d.legend_corner; o.minor_x = d.minor_x; o.minor_y = d.minor_y;
    memcpy(o.x_title, d.x_title, 32); memcpy(o.y_title, d.y_title, 32);
    size_t off = 0;
    for (int k = 0; k < d.n_series; k++) {
      const vbt_curve_series& s = series[s0 + (size_t)k];
      CfSeries& q = hs[s0 + (size_t)k];
      q.n = s.n_points; q.colour = s.colour; q.off = (int32_t)off; q.rev = revs[s0 + (size_t)k];
      memcpy(q.text, s.text, 64);
      off += (size_t)s.n_points;
    }
    s0 += (size_t)d.n_series; m0 += (size_t)d.n_marks; p0 += off;
  }
  if (T.marks) memcpy(up.data() + figs_b + ser_b, marks, T.marks * sizeof(CfMark));
  if (T.points) memcpy(up.data() + figs_b + ser_b + mk_b, xy, T.points * 16);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(f->blob.get(), up.data(), up.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    CfPrepArgs A{};
    A.figs = (const CfFigure*)f->blob.get(); A.series = (const CfSeries*)(f->blob.get() + figs_b); A.marks = (const CfMark*)(f->blob.get() + figs_b + ser_b);
    A.xy = (const double*)(f->blob.get() + figs_b + ser_b + mk_b);
    A.ws_col = f->d_col; A.ws_row = f->d_row; A.ws_lo = f->d_lo; A.ws_hi = f->d_hi;
    A.pts = f->d_pts; A.cnt = f->d_cnt; A.recs = f->d_recs; A.nrec = f->d_nrec;
    A.G = f->G; A.max_points = f->prm.max_points; A.rec_cap = f->rec_cap;
    curve_figure_prepare_kernel<<<dim3((unsigned)n), CF_THREADS, 0, st>>>(A);
    e = hipGetLastError();
  }
  if (int rc = f->finish_set(who, st, e)) return rc;                   // (`up` leaves scope: the copy must have read it)
  f->figs.assign(hf, hf + n);
  f->series.assign(hs, hs + T.series);
  f->d_figs = (const CfFigure*)f->blob.get(); f->d_series = (const CfSeries*)(f->blob.get() + figs_b);
  f->n = n;
  return VBT_OK;
}

int vbt_curve_figure_render(vbt_curve_figure* f, uint8_t* frames_dev, int fig0, int n, void* stream) {
  if (int rc = check_render_args("vbt_curve_figure_render", "vbt_curve_figure_set", f, frames_dev, fig0, n)) return rc;
  if (n == 0) return VBT_OK;
  VBT_HIP_CHECK(hipSetDevice(f->device));
  CfRenderArgs A{};
  A.figs = f->d_figs; A.series = f->d_series; A.pts = f->d_pts; A.cnt = f->d_cnt; A.recs = f->d_recs; A.nrec = f->d_nrec;
  A.frames = frames_dev; A.frame_bytes = (size_t)f->G.W * f->G.H * 3;
  A.G = f->G; A.max_points = f->prm.max_points; A.rec_cap = f->rec_cap; A.fig0 = fig0;
  A.tiles_x = (f->G.W + RASTER_TILE_W - 1) / RASTER_TILE_W;
  A.words = f->G.W % 4 == 0 && ((uintptr_t)frames_dev & 3) == 0;
  const int tiles_y = (f->G.H + CF_TILE_H - 1) / CF_TILE_H;
  curve_figure_render_kernel<<<dim3((unsigned)(A.tiles_x * tiles_y), (unsigned)n), CF_THREADS, 0, (hipStream_t)stream>>>(A);
  VBT_HIP_CHECK(hipGetLastError());
  f->last = (hipStream_t)stream;
  return VBT_OK;
}

int vbt_curve_figure_table(vbt_curve_figure* f, int fig, int32_t* counts, int cap_series, int* n_series, int32_t* points, int cap_points,
                           int* n_points, int32_t* records, int cap_records, int* n_records) {
  if (!f || !n_series || !n_points || !n_records || cap_series < 0 || cap_points < 0 || cap_records < 0 || (cap_series > 0 && !counts) ||
      (cap_points > 0 && !points) || (cap_records > 0 && !records)) {
    set_error("vbt_curve_figure_table: bad argument");
    return VBT_ERR_ARG;
  }
  int32_t nrec = 0, cnt[CF_MAX_SERIES] = {};
  if (int rc = table_begin("vbt_curve_figure_table", "vbt_curve_figure_set", f, fig, &nrec)) return rc;
  const CfFigure& F = f->figs[(size_t)fig];
  VBT_HIP_CHECK(hipMemcpy(cnt, f->d_cnt + (size_t)fig * CF_MAX_SERIES, sizeof(cnt), hipMemcpyDeviceToHost));
  long total = 0;
  for (int k = 0; k < F.n_series; k++) total += cnt[k];
  *n_series = F.n_series; *n_points = (int)total; *n_records = nrec;
  if (cap_series < F.n_series || cap_points < total || cap_records < nrec) {
    set_error("vbt_curve_figure_table: %d series, %ld points and %d records, room for %d, %d and %d", F.n_series, total, nrec, cap_series, cap_points, cap_records);
    return VBT_ERR_CAPACITY;
  }
  int32_t* out = points;
  for (int k = 0; k < F.n_series; k++) {
    counts[k] = cnt[k];
    const size_t at = (size_t)fig * f->prm.max_points + (size_t)f->series[(size_t)F.series0 + (size_t)k].off;
    if (cnt[k] > 0) VBT_HIP_CHECK(hipMemcpy(out, f->d_pts + at * CF_PT, (size_t)cnt[k] * CF_PT * 4, hipMemcpyDeviceToHost));
    out += (size_t)cnt[k] * CF_PT;
  }
  if (nrec > 0) VBT_HIP_CHECK(hipMemcpy(records, f->d_recs + (size_t)fig * f->rec_cap * CF_REC, (size_t)nrec * CF_REC * 4, hipMemcpyDeviceToHost));
  return VBT_OK;
}

}  // extern "C"
