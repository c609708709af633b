// Validation figure on the device (gfx950): the accuracy study of kinovea.py / qualysis.py for N (ground truth, tracked rows) pairs -
// the numbers of validate.metric_trajectory + validate.compare and N figures rendered into RGB24 frames that stay in device memory
// (include/vbt_hip.h, "Validation figure").  The aligned trajectories never leave the device between the comparison and the figure.
//   validation_prepare_kernel, once per vbt_validation_set: a workgroup of 256 lanes per pair.  Four lanes run the four window scans
//     (Kahan state, serial by nature); then the whole workgroup converts the rows to metres, forms the means, the grid, the
//     interpolation, the MSE and the Pearson terms - every sum as 256 lane partials and a halving tree through LDS, the order
//     validation_core.h states -, the extremes of the panels and every point's column and row; then four lanes merge the four series'
//     mapped points, one each, and a lane of another wavefront writes the records.  The launch is latency-bound (37 pairs of a few thousand rows): the serial parts are
//     left serial until measured (profiles/validation.md).
//   validation_render_kernel, once per vbt_validation_render: grid (tile of the frame, pair), as curve_figure_render_kernel - a lane
//     per series finds the merged points the tile's columns can meet, the workgroup stages them and the records that touch the tile in
//     LDS (or reads global memory when they do not fit), every lane decides four adjacent pixels of two rows and stores them once.
// Compiled without FMA contraction (-ffp-contract=off, as every unit here: build.py).
#include <algorithm>
#include <climits>
#include <cmath>

#include "figure_host.h"
#include "raster_tile.h"
#include "validation_core.h"

namespace vbt {

constexpr int VAL_THREADS = RASTER_THREADS;
constexpr int VAL_TILE_H = 8;
constexpr int VAL_ROWS_PER_LANE = VAL_TILE_H / 4;
static_assert(VAL_THREADS == VAL_LANES, "the sum order is the workgroup's");

struct ValPairIn { int32_t nref, T, ref0, row0, kind, pad[3]; };     // counts; first reference row and first tracked row among the set's

struct ValTables {                  // per pair, at index pair * its capacity
  double *sm, *traj, *grid, *stats, *head;
  int32_t *ws, *pts, *cnt, *recs, *nrec;     // ws: [pts_cap()][2] mapped points before the merge, at the offsets of pts
  int max_rows, max_ref, max_grid, rec_cap;
  __host__ __device__ size_t pts_cap() const { return 2 * ((size_t)max_rows + (size_t)max_ref); }
  // series k's merged points within a pair's: ref x, tracker x, ref y, tracker y
  __host__ __device__ size_t pts_off(int k) const { return (size_t)(k / 2) * ((size_t)max_rows + (size_t)max_ref) + (k & 1 ? (size_t)max_ref : 0); }
};

struct ValPrepArgs {
  const ValPairIn* pairs;
  const double *ref, *rows;
  ValTables D;
  ValGeom G;
  double plate, rate;
};

struct ValRenderArgs {
  ValTables D;
  uint8_t* frames;                  // frame of pair pair0 + blockIdx.y at frames + blockIdx.y * frame_bytes
  size_t frame_bytes;
  ValGeom G;
  int pair0, tiles_x;
  int words;                        // W % 4 == 0 and a 4-aligned base: four pixels go out as three 32-bit stores
};

// the sum of validation_core.h by the workgroup: every lane gets it
template <class F>
__device__ __forceinline__ double block_sum(double* s_red, int n, F term) {
  const int l = threadIdx.x;
  __syncthreads();                                                       // s_red is free, and what other lanes wrote can be read
  s_red[l] = val_partial(l, n, term);
  __syncthreads();
  for (int h = VAL_LANES / 2; h >= 1; h >>= 1) {
    if (l < h) s_red[l] = s_red[l] + s_red[l + h];
    __syncthreads();
  }
  return s_red[0];
}

// the smallest, or the largest, of a value per lane: every lane gets it
__device__ __forceinline__ double block_min(double* s_red, double v, bool largest) {
  const int l = threadIdx.x;
  __syncthreads();
  s_red[l] = v;
  __syncthreads();
  for (int h = VAL_LANES / 2; h >= 1; h >>= 1) {
    if (l < h) { const double a = s_red[l], b = s_red[l + h]; s_red[l] = largest ? (b > a ? b : a) : (b < a ? b : a); }
    __syncthreads();
  }
  return s_red[0];
}

__global__ __launch_bounds__(VAL_THREADS) void validation_prepare_kernel(ValPrepArgs A) {
  __shared__ double s_red[VAL_LANES];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const ValPairIn P = A.pairs[pair];
  const ValTables& D = A.D;
  const int nref = P.nref, T = P.T, kind = P.kind;
  const double* ref = A.ref + (size_t)P.ref0 * 3;
  const double* rows = A.rows + (size_t)P.row0 * 5;
  double* sm = D.sm + (size_t)pair * D.max_rows * 4;
  double* traj = D.traj + (size_t)pair * D.max_rows * 3;
  double* grid = D.grid + (size_t)pair * D.max_grid * VAL_GRID;
  double* stats = D.stats + (size_t)pair * VAL_STATS;
  double* head = D.head + (size_t)pair * VAL_HEAD;
  if (tid < 4) val_scan_column(rows, T, tid + 1, val_window(kind, tid + 1), sm);
  __syncthreads();
  for (int i = tid; i < T; i += VAL_THREADS) {
    traj[(size_t)i * 3] = rows[(size_t)i * 5];
    traj[(size_t)i * 3 + 1] = val_metric_x(sm + (size_t)i * 4, A.plate);
    traj[(size_t)i * 3 + 2] = val_metric_y(sm + (size_t)i * 4, A.plate);
  }
  for (int a = 2; a >= 1; a--) {                                         // y, then x
    const double sr = block_sum(s_red, nref, [&](int i) { return ref[(size_t)i * 3 + a]; });
    const double st = block_sum(s_red, T, [&](int i) { return traj[(size_t)i * 3 + a]; });
    const double d = val_shift(sr, nref, st, T);
    for (int i = tid; i < T; i += VAL_THREADS) traj[(size_t)i * 3 + a] = traj[(size_t)i * 3 + a] + d;   // (a lane's own elements)
  }
  __syncthreads();
  double t_min, t_max;
  int n;
  val_span(ref, nref, rows, T, A.rate, &t_min, &t_max, &n);
  n = n < D.max_grid ? n : D.max_grid;                                   // (never: set refused a larger grid)
  for (int i = tid; i < n; i += VAL_THREADS) {
    const double ts = val_grid_t(i, n, t_min, t_max);
    double* g = grid + (size_t)i * VAL_GRID;
    g[0] = ts;
    g[1] = val_interp(ref, ref + 1, 3, nref, ts);
    g[2] = val_interp(traj, traj + 1, 3, T, ts);
    g[3] = val_interp(ref, ref + 2, 3, nref, ts);
    g[4] = val_interp(traj, traj + 2, 3, T, ts);
  }
  int flags = 0;
  for (int a = 0; a < 2; a++) {
    const double* ga = grid + 1 + 2 * a;
    const double* gb = grid + 2 + 2 * a;
    const double se = block_sum(s_red, n, [&](int i) { return val_sq_diff(ga[(size_t)i * VAL_GRID], gb[(size_t)i * VAL_GRID]); });
    const double mse = se / (double)n;
    const double sa = block_sum(s_red, n, [&](int i) { return ga[(size_t)i * VAL_GRID]; });
    const double sb = block_sum(s_red, n, [&](int i) { return gb[(size_t)i * VAL_GRID]; });
    const double ma = sa / (double)n;
    const double mb = sb / (double)n;
    const double qa = block_sum(s_red, n, [&](int i) { return val_centred_sq(ga[(size_t)i * VAL_GRID], ma); });
    const double qb = block_sum(s_red, n, [&](int i) { return val_centred_sq(gb[(size_t)i * VAL_GRID], mb); });
    const double na = sqrt(qa);
    const double nb = sqrt(qb);
    const double dot = block_sum(s_red, n, [&](int i) { return val_pearson_term(ga[(size_t)i * VAL_GRID], ma, na, gb[(size_t)i * VAL_GRID], mb, nb); });
    int flag;
    const double r = val_pearson_clamp(dot, &flag);
    if (flag) flags |= a ? VAL_FLAG_R_Y_NAN : VAL_FLAG_R_X_NAN;
    if (tid == 0) { stats[VAL_S_MSE_X + a] = mse; stats[VAL_S_R_X + a] = r; }
  }
  if (tid == 0) { stats[VAL_S_N] = (double)n; stats[VAL_S_T_MIN] = t_min; stats[VAL_S_T_MAX] = t_max; stats[VAL_S_FLAGS] = (double)flags; }
  // the figure: the extremes of each panel over both its series
  double m[2], M[2];
  for (int a = 0; a < 2; a++) {
    double lo = ref[1 + a], hi = ref[1 + a];
    for (int i = tid; i < nref; i += VAL_THREADS) { const double v = ref[(size_t)i * 3 + 1 + a]; lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    for (int i = tid; i < T; i += VAL_THREADS) { const double v = traj[(size_t)i * 3 + 1 + a]; lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    m[a] = block_min(s_red, lo, false);
    M[a] = block_min(s_red, hi, true);
  }
  const double r1 = ref[(size_t)(nref - 1) * 3], k1 = rows[(size_t)(T - 1) * 5];
  double hd[VAL_HEAD];
  val_head(kind, r1 > k1 ? r1 : k1, m[0], M[0], m[1], M[1], hd);
  for (int k = 0; k < VAL_SERIES; k++) {                                 // every point to its column and row, the whole workgroup
    const int a = k / 2;
    const bool trk = k & 1;
    const double* src = trk ? traj : ref;
    int32_t* ws = D.ws + ((size_t)pair * D.pts_cap() + D.pts_off(k)) * 2;
    for (int i = tid; i < (trk ? T : nref); i += VAL_THREADS) val_point(src[(size_t)i * 3], src[(size_t)i * 3 + 1 + a], hd[1], hd[2 + 2 * a], hd[3 + 2 * a], A.G.PW, A.G.PH, ws + (size_t)i * 2);
  }
  __syncthreads();
  if (tid < VAL_SERIES) {                                                // the run merge: serial in a series, a lane each
    const size_t at = (size_t)pair * D.pts_cap() + D.pts_off(tid);
    D.cnt[(size_t)pair * VAL_SERIES + tid] = val_merge_points(D.ws + at * 2, tid & 1 ? T : nref, D.pts + at * CF_PT);
  }
  if (tid == 64) {
    for (int k = 0; k < VAL_HEAD; k++) head[k] = hd[k];
    D.nrec[pair] = val_records(A.G, kind, hd, D.recs + (size_t)pair * D.rec_cap * CF_REC, D.rec_cap);
  }
}

// what the workgroup knows of its series: LDS, read as broadcasts
struct ValTileSeries {
  int k0[VAL_SERIES], k1[VAL_SERIES];       // the bounds cf_item_range found for the tile's columns
  int first[VAL_SERIES], np[VAL_SERIES];    // the points the tile's items touch: first .. first + np - 1
  int m[VAL_SERIES];
};

// the tile's pixels from pointers the compiler knows the address space of.  staged: pts holds, series after series, the np points of
// each from its `first`; else pts is the pair's whole table.
__device__ __forceinline__ void validation_render_tile(const ValRenderArgs& A, const ValTileSeries& S, const int32_t* pts, bool staged, const int32_t* recs,
                                                       int nrec, int x_lo, int y_lo, uint8_t* frame) {
  const ValGeom& G = A.G;
  const int px = x_lo + (int)(threadIdx.x & 63) * 4;
  if (px >= G.W) return;
  const int last = px + 3 < G.W ? px + 3 : G.W - 1, n = last - px + 1;
  const int wave = (int)(threadIdx.x >> 6);
  uint32_t cur[VAL_ROWS_PER_LANE];                                    // a colour index per pixel, 0xff where no curve is
#pragma unroll
  for (int j = 0; j < VAL_ROWS_PER_LANE; j++) cur[j] = 0xffffffffu;
  int at = 0;
  for (int k = 0; k < VAL_SERIES; k++) {
    const CfSeriesView V{staged ? pts + (size_t)at * CF_PT : pts + A.D.pts_off(k) * CF_PT, staged ? S.first[k] : 0, S.m[k], k & 1};
    at += S.np[k];
    if (S.np[k] == 0) continue;
    const int PY = k >= 2 ? G.Y1 : G.Y0;
    if (y_lo + VAL_TILE_H <= PY || y_lo >= PY + G.PH) continue;        // the tile has no row of the series' panel
    int i0, i1, q0, q1;
    cf_item_range(V, S.k0[k], S.k1[k], G.t, px - G.X0, last - G.X0, &i0, &i1, &q0, &q1);
    if (i0 > i1) continue;
    int rlo = 65536, rhi = -65536;                                    // the rows the lane's own items reach
    for (int i = i0 > 0 ? i0 - 1 : 0; i <= i1; i++) {
      const int v = V.pts[(size_t)(i - V.base) * CF_PT + CF_PT_ROW];
      rlo = v < rlo ? v : rlo; rhi = v > rhi ? v : rhi;
    }
    const uint32_t c = (uint32_t)(CF_C_SERIES + V.colour);
#pragma unroll
    for (int j = 0; j < VAL_ROWS_PER_LANE; j++) {
      const int qy = y_lo + wave + 4 * j - PY;
      if (qy < 0 || qy >= G.PH) continue;
      const unsigned mask = cf_curve_mask(V, G.t, G.PW, px - G.X0, n, qy, i0, i1, rlo, rhi);
#pragma unroll
      for (int e = 0; e < 4; e++)
        if (mask >> e & 1) cur[j] = (cur[j] & ~(0xffu << (8 * e))) | c << (8 * e);
    }
  }
#pragma unroll
  for (int j = 0; j < VAL_ROWS_PER_LANE; j++) {                        // wavefront w takes rows w, w + 4, ...
    const int py = y_lo + wave + 4 * j;
    if (py >= G.H) return;
    uint8_t* p = frame + ((size_t)py * G.W + px) * 3;
    int over[4], oc[4], under[4], uc[4];
    cf_records4(recs, nrec, G.s, px, py, n, over, oc, under, uc);
    uint32_t rgb[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int cc = (int)(cur[j] >> (8 * e) & 0xffu);
      rgb[e] = val_rgb(over[e] != CF_KIND_NONE ? oc[e] : (cc != 0xff ? cc : uc[e]));
    }
    store_rgb24x4(p, rgb, n, A.words);                                // W % 4 == 0: px + 3 < W, and p is 4-aligned
  }
}

__global__ __launch_bounds__(VAL_THREADS, 4) void validation_render_kernel(ValRenderArgs A) {
  __shared__ int32_t s_pts[VBT_VALIDATION_STAGE_POINTS * CF_PT];
  __shared__ int32_t s_recs[VBT_VALIDATION_STAGE_RECORDS * CF_REC];
  __shared__ ValTileSeries S;
  __shared__ int s_found;
  const ValGeom& G = A.G;
  const ValTables& D = A.D;
  const int pair = A.pair0 + (int)blockIdx.y, tid = threadIdx.x;
  const int nrec = D.nrec[pair];
  const int32_t* gp = D.pts + (size_t)pair * D.pts_cap() * CF_PT;
  const int32_t* gr = D.recs + (size_t)pair * D.rec_cap * CF_REC;
  const TileBox box = tile_box<VAL_TILE_H>(A.tiles_x, G.W, G.H);
  if (tid == 0) s_found = 0;
  if (tid < VAL_SERIES) {                                               // the points of the tile's columns: a lane per series, on the whole table
    const int m = D.cnt[(size_t)pair * VAL_SERIES + tid];
    const CfSeriesView V{gp + D.pts_off(tid) * CF_PT, 0, m, tid & 1};
    int i0, i1, k0, k1;
    cf_item_range(V, 0, m, G.t, box.x_lo - G.X0, box.x_hi - G.X0, &i0, &i1, &k0, &k1);
    const int first = i0 <= i1 ? (i0 > 0 ? i0 - 1 : 0) : 0;
    S.k0[tid] = k0; S.k1[tid] = k1; S.first[tid] = first; S.np[tid] = i0 <= i1 ? i1 - first + 1 : 0;
    S.m[tid] = m;
  }
  __syncthreads();
  int total = 0;
  for (int k = 0; k < VAL_SERIES; k++) total += S.np[k];
  const bool pts_staged = total <= VBT_VALIDATION_STAGE_POINTS;
  if (pts_staged) {
    int at = 0;
    for (int k = 0; k < VAL_SERIES; k++) {
      const int32_t* src = gp + (D.pts_off(k) + (size_t)S.first[k]) * CF_PT;
      for (int i = tid; i < S.np[k] * CF_PT; i += VAL_THREADS) s_pts[at * CF_PT + i] = src[i];
      at += S.np[k];
    }
  }
  stage_tile_records<CF_REC>(gr, nrec, box, s_recs, VBT_VALIDATION_STAGE_RECORDS, &s_found);
  __syncthreads();
  const int found = s_found;
  uint8_t* frame = A.frames + (size_t)blockIdx.y * A.frame_bytes;
  if (pts_staged && found <= VBT_VALIDATION_STAGE_RECORDS)
    validation_render_tile(A, S, s_pts, true, s_recs, found, box.x_lo, box.y_lo, frame);
  else                                                                  // long series or a crowded tile: the same statements on global memory
    validation_render_tile(A, S, gp, false, gr, nrec, box.x_lo, box.y_lo, frame);
}

}  // namespace vbt

using namespace vbt;

struct vbt_validation : FigureHandle {   // blob: upload (pairs | reference rows | tracked rows) | sm | traj | grid | stats | head | ws | pts | cnt | recs | nrec
  vbt_validation_params prm{};
  ValGeom G{};
  ValTables D{};
  std::vector<ValPairIn> pairs;          // the host's copy, with each pair's grid size
  std::vector<int> grid_n;
};

namespace {

int check_validation_params(const vbt_validation_params& p) {
  const char* who = "vbt_validation_create";
  if (int rc = check_canvas(who, p.width, p.height, p.scale, p.thickness)) return rc;
  if (p.max_pairs < 1 || p.max_pairs > VAL_MAX_PAIRS) { set_error("%s: max_pairs %d outside 1..%d", who, p.max_pairs, (int)VAL_MAX_PAIRS); return VBT_ERR_ARG; }
  if (p.max_rows < 2 || p.max_rows > VAL_MAX_ROWS) { set_error("%s: max_rows %d outside 2..%d", who, p.max_rows, (int)VAL_MAX_ROWS); return VBT_ERR_ARG; }
  if (p.max_ref_rows < 2 || p.max_ref_rows > VAL_MAX_ROWS) { set_error("%s: max_ref_rows %d outside 2..%d", who, p.max_ref_rows, (int)VAL_MAX_ROWS); return VBT_ERR_ARG; }
  if (p.max_grid < 2 || p.max_grid > VAL_MAX_ROWS) { set_error("%s: max_grid %d outside 2..%d", who, p.max_grid, (int)VAL_MAX_ROWS); return VBT_ERR_ARG; }
  if ((long)p.max_pairs * ((long)p.max_rows + p.max_ref_rows + p.max_grid) > (1l << 26)) {
    set_error("%s: %d pairs of %d + %d rows and %d grid points: above 2^26 in all", who, p.max_pairs, p.max_rows, p.max_ref_rows, p.max_grid);
    return VBT_ERR_ARG;
  }
  return check_plot_rect(who, val_geom(p.width, p.height, p.scale, p.thickness), VAL_MIN_PLOT);
}

struct ValTotals { size_t ref = 0, rows = 0; };

// the refusals of vbt_validation_set that need no handle and no device, in the header's order; each pair's grid size on VBT_OK
int check_validation_set(int n, const int32_t* kinds, double plate, double rate, const double* ref, const int32_t* ref_counts, const double* rows,
                         const int32_t* row_counts, ValTotals* tot, std::vector<int>* grid_n) {
  const char* who = "vbt_validation_set";
  if (n < 0 || (n > 0 && (!kinds || !ref || !ref_counts || !rows || !row_counts))) {
    set_error("%s: bad argument (n %d, kinds %p, ref %p, ref_counts %p, rows %p, row_counts %p)", who, n, (const void*)kinds, (const void*)ref, (const void*)ref_counts, (const void*)rows,
              (const void*)row_counts);
    return VBT_ERR_ARG;
  }
  if (n > VAL_MAX_PAIRS) { set_error("%s: %d pairs, above %d", who, n, (int)VAL_MAX_PAIRS); return VBT_ERR_CAPACITY; }
  for (int i = 0; i < n; i++)
    if (kinds[i] != VAL_KIND_KINOVEA && kinds[i] != VAL_KIND_QUALISYS) { set_error("%s: pair %d: kind %d is neither 0 (kinovea) nor 1 (qualisys)", who, i, kinds[i]); return VBT_ERR_ARG; }
  if (!(ov_finite(plate) && plate > 0.0)) { set_error("%s: plate_diameter %g is not finite and above 0", who, plate); return VBT_ERR_ARG; }
  if (!(ov_finite(rate) && rate > 0.0)) { set_error("%s: rate %g is not finite and above 0", who, rate); return VBT_ERR_ARG; }
  for (int i = 0; i < n; i++)
    if (ref_counts[i] < 0 || row_counts[i] < 0) { set_error("%s: pair %d has a negative count (%d reference rows, %d tracked rows)", who, i, ref_counts[i], row_counts[i]); return VBT_ERR_ARG; }
  grid_n->assign((size_t)n, 0);
  ValTotals T;
  static const char* const series_name[2] = {"reference", "tracked"};
  for (int i = 0; i < n; i++) {
    const double* r = ref + T.ref * 3;
    const double* k = rows + T.rows * 5;
    const int nref = ref_counts[i], nt = row_counts[i];
    int series = 0, row = 0;
    switch (val_pair_check(r, nref, k, nt, &series, &row)) {
      case VAL_BAD_NONFINITE: set_error("%s: pair %d, %s row %d: a value is not finite", who, i, series_name[series], row); return VBT_ERR_ARG;
      case VAL_BAD_PLATE: set_error("%s: pair %d, tracked row %d: a plate size of 0 or below", who, i, row); return VBT_ERR_ARG;
      case VAL_BAD_FEW: set_error("%s: pair %d: %d %s rows, fewer than 2", who, i, row, series_name[series]); return VBT_ERR_ARG;
      case VAL_BAD_TIME: set_error("%s: pair %d, %s row %d: time does not rise strictly", who, i, series_name[series], row); return VBT_ERR_ARG;
      default: break;
    }
    double t_min, t_max;
    int g;
    val_span(r, nref, k, nt, rate, &t_min, &t_max, &g);
    if (!(t_max > t_min)) { set_error("%s: pair %d: no common time span (%g .. %g)", who, i, t_min, t_max); return VBT_ERR_ARG; }
    if (g < 2) { set_error("%s: pair %d: a grid of n = %d points, fewer than 2", who, i, g); return VBT_ERR_ARG; }
    (*grid_n)[(size_t)i] = g;
    T.ref += (size_t)nref; T.rows += (size_t)nt;
  }
  *tot = T;
  return VBT_OK;
}

}  // namespace

extern "C" {

void vbt_validation_default_params(vbt_validation_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->width = 1280; p->height = 640; p->scale = 2; p->thickness = 2; p->max_pairs = 64; p->max_rows = 4096; p->max_ref_rows = 4096; p->max_grid = 4096;
}

int vbt_validation_create(int device, const vbt_validation_params* params, vbt_validation** out) {
  if (!out) { set_error("vbt_validation_create: out is NULL"); return VBT_ERR_ARG; }
  *out = nullptr;
  vbt_validation_params p;
  vbt_validation_default_params(&p);
  if (params) p = *params;
  if (int rc = check_validation_params(p)) return rc;
  if (int rc = use_device("vbt_validation_create", device, /*set_current=*/true)) return rc;
  std::unique_ptr<vbt_validation> f(new vbt_validation());
  f->device = device; f->prm = p; f->G = val_geom(p.width, p.height, p.scale, p.thickness);
  f->rec_cap = VAL_FIXED_RECS;
  ValTables& D = f->D;
  D.max_rows = p.max_rows; D.max_ref = p.max_ref_rows; D.max_grid = p.max_grid; D.rec_cap = f->rec_cap;
  const size_t N = (size_t)p.max_pairs, T = (size_t)p.max_rows, R = (size_t)p.max_ref_rows, Gn = (size_t)p.max_grid;
  FigCarver C;                                                          // the largest upload, at the blob's head
  C.add<uint8_t>(align64(N * sizeof(ValPairIn)) + N * (R * 24 + T * 40));
  const auto sm = C.add<double>(N * T * 4), traj = C.add<double>(N * T * 3), grid = C.add<double>(N * Gn * VAL_GRID);
  const auto stats = C.add<double>(N * VAL_STATS), head = C.add<double>(N * VAL_HEAD);
  const auto ws = C.add<int32_t>(N * D.pts_cap() * 2), pts = C.add<int32_t>(N * D.pts_cap() * CF_PT), cnt = C.add<int32_t>(N * VAL_SERIES);
  const auto recs = C.add<int32_t>(N * (size_t)f->rec_cap * CF_REC), nrec = C.add<int32_t>(N);
  if (f->blob.alloc(C.bytes()) != hipSuccess) {
    (void)hipGetLastError();
    set_error("vbt_validation_create: the device cannot give %zu bytes for %d pairs of %d + %d rows and %d grid points", C.bytes(), p.max_pairs, p.max_rows,
              p.max_ref_rows, p.max_grid);
    return VBT_ERR_HIP;
  }
  D.sm = C.ptr(f->blob.get(), sm); D.traj = C.ptr(f->blob.get(), traj); D.grid = C.ptr(f->blob.get(), grid); D.stats = C.ptr(f->blob.get(), stats); D.head = C.ptr(f->blob.get(), head);
  D.ws = C.ptr(f->blob.get(), ws); D.pts = C.ptr(f->blob.get(), pts); D.cnt = C.ptr(f->blob.get(), cnt); D.recs = C.ptr(f->blob.get(), recs); D.nrec = C.ptr(f->blob.get(), nrec);
  f->d_recs = D.recs; f->d_nrec = D.nrec;
  *out = f.release();
  return VBT_OK;
}

void vbt_validation_destroy(vbt_validation* f) { delete f; }

int vbt_validation_set(vbt_validation* f, int n, const int32_t* kinds, double plate_diameter, double rate, const double* ref, const int32_t* ref_counts,
                       const double* rows, const int32_t* row_counts, void* stream) {
  ValTotals T;
  std::vector<int> grid_n;
  if (int rc = check_validation_set(n, kinds, plate_diameter, rate, ref, ref_counts, rows, row_counts, &T, &grid_n)) return rc;
  const char* who = "vbt_validation_set";
  if (!f) { set_error("%s: handle is NULL", who); return VBT_ERR_ARG; }
  if (n > f->prm.max_pairs) { set_error("%s: %d pairs, the handle holds %d", who, n, f->prm.max_pairs); return VBT_ERR_CAPACITY; }
  for (int i = 0; i < n; i++) {
    if (ref_counts[i] > f->prm.max_ref_rows) { set_error("%s: pair %d has %d reference rows, the handle holds %d", who, i, ref_counts[i], f->prm.max_ref_rows); return VBT_ERR_CAPACITY; }
    if (row_counts[i] > f->prm.max_rows) { set_error("%s: pair %d has %d tracked rows, the handle holds %d", who, i, row_counts[i], f->prm.max_rows); return VBT_ERR_CAPACITY; }
    if (grid_n[(size_t)i] > f->prm.max_grid) { set_error("%s: pair %d has a grid of n = %d points, the handle holds %d", who, i, grid_n[(size_t)i], f->prm.max_grid); return VBT_ERR_CAPACITY; }
  }
  VBT_HIP_CHECK(hipSetDevice(f->device));
  f->n = 0;
  if (n == 0) return VBT_OK;
  const size_t pairs_b = align64((size_t)n * sizeof(ValPairIn));
  std::vector<uint8_t> up(pairs_b + T.ref * 24 + T.rows * 40, 0);
  ValPairIn* hp = (ValPairIn*)up.data();
  size_t r0 = 0, k0 = 0;
  for (int i = 0; i < n; i++) {
    hp[i] = ValPairIn{ref_counts[i], row_counts[i], (int32_t)r0, (int32_t)k0, kinds[i], {0, 0, 0}};
    r0 += (size_t)ref_counts[i]; k0 += (size_t)row_counts[i];
  }
  memcpy(up.data() + pairs_b, ref, T.ref * 24);
  memcpy(up.data() + pairs_b + T.ref * 24, rows, T.rows * 40);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(f->blob.get(), up.data(), up.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    ValPrepArgs A{};
    A.pairs = (const ValPairIn*)f->blob.get(); A.ref = (const double*)(f->blob.get() + pairs_b); A.rows = (const double*)(f->blob.get() + pairs_b + T.ref * 24);
    A.D = f->D; A.G = f->G; A.plate = plate_diameter; A.rate = rate;
    validation_prepare_kernel<<<dim3((unsigned)n), VAL_THREADS, 0, st>>>(A);
    e = hipGetLastError();
  }
  if (int rc = f->finish_set(who, st, e)) return rc;                   // (`up` leaves scope: the copy must have read it)
  f->pairs.assign(hp, hp + n);
  f->grid_n = grid_n;
  f->n = n;
  return VBT_OK;
}

int vbt_validation_stats(vbt_validation* f, double* out, int cap) {
  const char* who = "vbt_validation_stats";
  if (!f || !out || cap < 0) { set_error("%s: bad argument (handle %p, out %p, cap %d)", who, (const void*)f, (const void*)out, cap); return VBT_ERR_ARG; }
  if (f->n == 0) { set_error("%s: no pairs are set (vbt_validation_set)", who); return VBT_ERR_STATE; }
  if (cap < f->n) { set_error("%s: %d pairs are set, room for %d", who, f->n, cap); return VBT_ERR_CAPACITY; }
  VBT_HIP_CHECK(hipSetDevice(f->device));
  VBT_HIP_CHECK(hipStreamSynchronize(f->last));
  VBT_HIP_CHECK(hipMemcpy(out, f->D.stats, (size_t)f->n * VAL_STATS * 8, hipMemcpyDeviceToHost));
  return VBT_OK;
}

int vbt_validation_render(vbt_validation* f, uint8_t* frames_dev, int pair0, int n, void* stream) {
  if (int rc = check_render_args("vbt_validation_render", "vbt_validation_set", f, frames_dev, pair0, n)) return rc;
  if (n == 0) return VBT_OK;
  VBT_HIP_CHECK(hipSetDevice(f->device));
  ValRenderArgs A{};
  A.D = f->D; A.frames = frames_dev; A.frame_bytes = (size_t)f->G.W * f->G.H * 3;
  A.G = f->G; A.pair0 = pair0;
  A.tiles_x = (f->G.W + RASTER_TILE_W - 1) / RASTER_TILE_W;
  A.words = f->G.W % 4 == 0 && ((uintptr_t)frames_dev & 3) == 0;
  const int tiles_y = (f->G.H + VAL_TILE_H - 1) / VAL_TILE_H;
  validation_render_kernel<<<dim3((unsigned)(A.tiles_x * tiles_y), (unsigned)n), VAL_THREADS, 0, (hipStream_t)stream>>>(A);
  VBT_HIP_CHECK(hipGetLastError());
  f->last = (hipStream_t)stream;
  return VBT_OK;
}

int vbt_validation_table(vbt_validation* f, int pair, double* head, double* traj, int cap_rows, int* n_rows, double* grid, int cap_grid, int* n_grid,
                         int32_t* counts, int32_t* points, int cap_points, int* n_points, int32_t* records, int cap_records, int* n_records) {
  const char* who = "vbt_validation_table";
  if (!f || !head || !counts || !n_rows || !n_grid || !n_points || !n_records || cap_rows < 0 || cap_grid < 0 || cap_points < 0 || cap_records < 0 ||
      (cap_rows > 0 && !traj) || (cap_grid > 0 && !grid) || (cap_points > 0 && !points) || (cap_records > 0 && !records)) {
    set_error("%s: bad argument", who);
    return VBT_ERR_ARG;
  }
  int32_t nrec = 0, cnt[VAL_SERIES] = {};
  if (int rc = table_begin(who, "vbt_validation_set", f, pair, &nrec)) return rc;
  const ValTables& D = f->D;
  const int T = f->pairs[(size_t)pair].T, g = f->grid_n[(size_t)pair];
  VBT_HIP_CHECK(hipMemcpy(cnt, D.cnt + (size_t)pair * VAL_SERIES, sizeof(cnt), hipMemcpyDeviceToHost));
  VBT_HIP_CHECK(hipMemcpy(head, D.head + (size_t)pair * VAL_HEAD, VAL_HEAD * 8, hipMemcpyDeviceToHost));
  long total = 0;
  for (int k = 0; k < VAL_SERIES; k++) { counts[k] = cnt[k]; total += cnt[k]; }
  *n_rows = T; *n_grid = g; *n_points = (int)total; *n_records = nrec;
  if (cap_rows < T || cap_grid < g || cap_points < total || cap_records < nrec) {
    set_error("%s: %d rows, %d grid points, %ld points and %d records, room for %d, %d, %d and %d", who, T, g, total, nrec, cap_rows, cap_grid, cap_points, cap_records);
    return VBT_ERR_CAPACITY;
  }
  VBT_HIP_CHECK(hipMemcpy(traj, D.traj + (size_t)pair * D.max_rows * 3, (size_t)T * 24, hipMemcpyDeviceToHost));
  VBT_HIP_CHECK(hipMemcpy(grid, D.grid + (size_t)pair * D.max_grid * VAL_GRID, (size_t)g * VAL_GRID * 8, hipMemcpyDeviceToHost));
  int32_t* out = points;
  for (int k = 0; k < VAL_SERIES; k++) {
    if (cnt[k] > 0) VBT_HIP_CHECK(hipMemcpy(out, D.pts + ((size_t)pair * D.pts_cap() + D.pts_off(k)) * CF_PT, (size_t)cnt[k] * CF_PT * 4, hipMemcpyDeviceToHost));
    out += (size_t)cnt[k] * CF_PT;
  }
  if (nrec > 0) VBT_HIP_CHECK(hipMemcpy(records, D.recs + (size_t)pair * D.rec_cap * CF_REC, (size_t)nrec * CF_REC * 4, hipMemcpyDeviceToHost));
  return VBT_OK;
}

}  // extern "C"
