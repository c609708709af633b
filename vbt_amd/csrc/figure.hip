// Rep figure on the device (gfx950): plot.py's position / velocity figure of N tracks rendered into N RGB24 frames that stay in
// device memory (include/vbt_hip.h, "Rep figure"; reference plot.py:87-232).  Two kernels:
//   figure_prepare_kernel, once per vbt_figure_set: a workgroup per figure.  Four lanes scan the rolling means (sequential per
//     series), the workgroup reduces their extremes, forms the ranges, maps every row to its point (column, four pixel rows), and one
//     lane walks the phases and ticks into the figure's records.
//   figure_render_kernel, once per vbt_figure_render: grid (tile of the frame, figure).  A gather with one writer per pixel: the
//     workgroup finds the points its columns can meet by two binary searches on the column table, stages them and the records that
//     touch the tile in LDS (or reads global memory when they do not fit), and every lane decides four adjacent pixels by the
//     contract's test (figure_core.h) and stores them once.  Nothing is read from the frames.
// Shared with curve_figure.hip: the tile's rectangle, the record staging and the RGB24 store (raster_tile.h), the handle's host side (figure_host.h).
// This translation unit is compiled without FMA contraction (-ffp-contract=off, as every unit here: build.py), so the doubles of the
// contract are the ones a host compiler forms from figure_core.h.
#include <algorithm>

#include "figure_core.h"
#include "figure_host.h"
#include "raster_tile.h"

namespace vbt {

constexpr int FIG_THREADS = RASTER_THREADS;
constexpr int FIG_TILE_H = 32;
constexpr int FIG_META = 8;                           // per figure: rows, phases, first row, first phase of the upload

struct FigPrepArgs {
  const int32_t* meta;     // [n][FIG_META]
  const double* rows;      // the rows of all figures, 7 doubles each
  const double* phases;    // the phases of all figures, 6 doubles each
  double* smooth;          // [max_figures][4][max_rows]
  double* head;            // [max_figures][FIG_HEAD]
  int32_t* pts;            // [max_figures][max_rows][FIG_PT]
  int32_t* recs;           // [max_figures][rec_cap][FIG_REC]
  int32_t* nrec;           // [max_figures]
  FigGeom G;
  int max_rows, rec_cap;
};

struct FigRenderArgs {
  const int32_t* meta;
  const int32_t* pts;
  const int32_t* recs;
  const int32_t* nrec;
  uint8_t* frames;         // frame of figure fig0 + blockIdx.y at frames + blockIdx.y * frame_bytes
  size_t frame_bytes;
  FigGeom G;
  int max_rows, rec_cap, fig0, tiles_x;
  int words;               // W % 4 == 0 and a 4-aligned base: four pixels go out as three 32-bit stores
};

__global__ __launch_bounds__(FIG_THREADS) void figure_prepare_kernel(FigPrepArgs A) {
  __shared__ double s_lo[2][FIG_THREADS], s_hi[2][FIG_THREADS];
  __shared__ double s_head[FIG_HEAD];
  const int fig = blockIdx.x, tid = threadIdx.x;
  const int32_t* m = A.meta + (size_t)fig * FIG_META;
  const int T = m[0], P = m[1];
  const double* rows = A.rows + (size_t)m[2] * 7;
  const double* ph = A.phases + (size_t)m[3] * 6;
  double* sm = A.smooth + (size_t)fig * 4 * A.max_rows;
  if (tid < 4) fig_smooth_series(rows, T, tid, sm + (size_t)tid * A.max_rows);
  __syncthreads();
  double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
  for (int i = tid; i < T; i += FIG_THREADS)
    for (int k = 0; k < 4; k++) {
      const double v = sm[(size_t)k * A.max_rows + i];
      lo[k >> 1] = v < lo[k >> 1] ? v : lo[k >> 1];
      hi[k >> 1] = v > hi[k >> 1] ? v : hi[k >> 1];
    }
  for (int q = 0; q < 2; q++) { s_lo[q][tid] = lo[q]; s_hi[q][tid] = hi[q]; }
  __syncthreads();
  for (int step = FIG_THREADS / 2; step > 0; step >>= 1) {
    if (tid < step)
      for (int q = 0; q < 2; q++) {
        s_lo[q][tid] = s_lo[q][tid + step] < s_lo[q][tid] ? s_lo[q][tid + step] : s_lo[q][tid];
        s_hi[q][tid] = s_hi[q][tid + step] > s_hi[q][tid] ? s_hi[q][tid + step] : s_hi[q][tid];
      }
    __syncthreads();
  }
  if (tid == 0) {
    fig_head(T, T > 0 ? rows[0] : 0.0, T > 0 ? rows[(size_t)(T - 1) * 7] : 0.0, s_lo[0][0], s_hi[0][0], s_lo[1][0], s_hi[1][0], s_head);
    for (int k = 0; k < FIG_HEAD; k++) A.head[(size_t)fig * FIG_HEAD + k] = s_head[k];
  }
  __syncthreads();
  double head[FIG_HEAD];
  for (int k = 0; k < FIG_HEAD; k++) head[k] = s_head[k];
  int32_t* pts = A.pts + (size_t)fig * A.max_rows * FIG_PT;
  for (int i = tid; i < T; i += FIG_THREADS) {
    double sm4[4];
    for (int k = 0; k < 4; k++) sm4[k] = sm[(size_t)k * A.max_rows + i];
    int32_t pt[FIG_PT];
    fig_point(A.G, head, rows[(size_t)i * 7], sm4, pt);
    for (int k = 0; k < FIG_PT; k++) pts[(size_t)i * FIG_PT + k] = pt[k];
  }
  if (tid == 0) A.nrec[fig] = fig_records(A.G, head, ph, P, A.recs + (size_t)fig * A.rec_cap * FIG_REC, A.rec_cap);
}

// the tile's pixels from a view whose pointers the compiler knows the address space of
__device__ __forceinline__ void figure_render_tile(const FigRenderArgs& A, const FigView& T, int k0, int k1, int x_lo, int y_lo, uint8_t* frame) {
  const FigGeom& G = A.G;
  const int px = x_lo + (int)(threadIdx.x & 63) * 4;
  if (px >= G.W) return;
  int seg0, seg1, q0, q1;
  const int last = px + 3 < G.W ? px + 3 : G.W - 1;
  fig_seg_range(T, k0, k1, G.t, px - G.X0, last - G.X0, &seg0, &seg1, &q0, &q1);
  // the rows the lane's own segments reach, once for all its pixel rows: a curve crosses its four columns in a few rows, and every
  // other row skips the segments without loading a point
  FigView V = T;
#pragma unroll
  for (int k = 1; k < FIG_PT; k++) { V.rlo[k] = 65536; V.rhi[k] = -65536; }
  if (seg0 <= seg1) {
    const int pe = seg1 + 1 < T.T ? seg1 + 1 : T.T - 1;
    for (int i = seg0; i <= pe; i++) {
      const int32_t* q = T.pts + (size_t)(i - T.pt_base) * FIG_PT;
#pragma unroll
      for (int k = 1; k < FIG_PT; k++) { const int v = q[k]; V.rlo[k] = v < V.rlo[k] ? v : V.rlo[k]; V.rhi[k] = v > V.rhi[k] ? v : V.rhi[k]; }
    }
  }
  for (int j = 0; j < FIG_TILE_H / 4; j++) {                        // wavefront w takes rows w, w + 4, ...
    const int py = y_lo + (int)(threadIdx.x >> 6) + 4 * j;
    if (py >= G.H) return;
    uint8_t* p = frame + ((size_t)py * G.W + px) * 3;
    int ci[4] = {0, 0, 0, 0};
    fig_pixels4(G, V, px, py, last - px + 1, seg0, seg1, ci);
    const uint32_t rgb[4] = {fig_rgb(ci[0]), fig_rgb(ci[1]), fig_rgb(ci[2]), fig_rgb(ci[3])};
    store_rgb24x4(p, rgb, last - px + 1, A.words);                  // W % 4 == 0: px + 3 < W, and p is 4-aligned
  }
}

__global__ __launch_bounds__(FIG_THREADS, 4) void figure_render_kernel(FigRenderArgs A) {
  __shared__ int32_t s_pts[VBT_FIGURE_STAGE_POINTS * FIG_PT];
  __shared__ int32_t s_recs[VBT_FIGURE_STAGE_RECORDS * FIG_REC];
  __shared__ int s_found;
  const FigGeom& G = A.G;
  const int fig = A.fig0 + (int)blockIdx.y, tid = threadIdx.x;
  const int T = A.meta[(size_t)fig * FIG_META], nrec = A.nrec[fig];
  const int32_t* gp = A.pts + (size_t)fig * A.max_rows * FIG_PT;
  const int32_t* gr = A.recs + (size_t)fig * A.rec_cap * FIG_REC;
  const TileBox box = tile_box<FIG_TILE_H>(A.tiles_x, G.W, G.H);
  if (tid == 0) s_found = 0;
  __syncthreads();
  // the points of the tile's columns: once per workgroup, on the whole table
  FigView V{gp, 0, T, gr, nrec, {}, {}};
  int seg0, seg1, k0, k1;
  fig_seg_range(V, 0, T, G.t, box.x_lo - G.X0, box.x_hi - G.X0, &seg0, &seg1, &k0, &k1);
  const int p0 = seg0, np = seg0 <= seg1 ? (seg1 + 1 < T ? seg1 + 1 : T - 1) - p0 + 1 : 0;
  const bool pts_staged = np <= VBT_FIGURE_STAGE_POINTS;
  if (pts_staged)
    for (int i = tid; i < np * FIG_PT; i += FIG_THREADS) s_pts[i] = gp[(size_t)p0 * FIG_PT + i];
  stage_tile_records<FIG_REC>(gr, nrec, box, s_recs, VBT_FIGURE_STAGE_RECORDS, &s_found);
  __syncthreads();
  const int found = s_found;
  const bool recs_staged = found <= VBT_FIGURE_STAGE_RECORDS;
  uint8_t* frame = A.frames + (size_t)blockIdx.y * A.frame_bytes;
  if (pts_staged && recs_staged) {
    FigView S{s_pts, p0, T, s_recs, found, {}, {}};
    fig_view_unbounded(S);
    figure_render_tile(A, S, k0, k1, box.x_lo, box.y_lo, frame);
  } else {                                                          // a dense series or a crowded tile: the same statements on global memory
    FigView S{pts_staged ? s_pts : gp, pts_staged ? p0 : 0, T, recs_staged ? s_recs : gr, recs_staged ? found : nrec, {}, {}};
    fig_view_unbounded(S);
    figure_render_tile(A, S, k0, k1, box.x_lo, box.y_lo, frame);
  }
}

}  // namespace vbt

using namespace vbt;

struct vbt_figure : FigureHandle {     // blob: upload (meta | rows | phases) | head | pts | recs | nrec | smooth
  vbt_figure_params prm{};
  FigGeom G{};
  double *d_smooth = nullptr, *d_head = nullptr;
  int32_t* d_pts = nullptr;
  std::vector<int32_t> meta;           // the host's copy
};

namespace {

int check_figure_params(const vbt_figure_params& p) {
  const char* who = "vbt_figure_create";
  if (int rc = check_canvas(who, p.width, p.height, p.scale, p.thickness)) return rc;
  if (p.max_figures < 1 || p.max_figures > FIG_MAX_FIGURES) { set_error("%s: max_figures %d outside 1..%d", who, p.max_figures, (int)FIG_MAX_FIGURES); return VBT_ERR_ARG; }
  if (p.max_rows < 1 || p.max_rows > FIG_MAX_ROWS) { set_error("%s: max_rows %d outside 1..%d", who, p.max_rows, (int)FIG_MAX_ROWS); return VBT_ERR_ARG; }
  if (p.max_phases < 0 || p.max_phases > FIG_MAX_PHASES) { set_error("%s: max_phases %d outside 0..%d", who, p.max_phases, (int)FIG_MAX_PHASES); return VBT_ERR_ARG; }
  if ((long)p.max_figures * p.max_rows > (1l << 26) || (long)p.max_figures * p.max_phases > (1l << 22)) {
    set_error("%s: %d figures of %d rows and %d phases: above 2^26 rows or 2^22 phases in all", who, p.max_figures, p.max_rows, p.max_phases);
    return VBT_ERR_ARG;
  }
  return check_plot_rect(who, fig_geom(p.width, p.height, p.scale, p.thickness), FIG_MIN_PLOT);
}

// the refusals of vbt_figure_set that need no handle and no device; the totals on VBT_OK
int check_figure_set(int n, const double* rows, const int32_t* row_counts, const double* phases, const int32_t* phase_counts, size_t* rows_total,
                     size_t* phases_total) {
  const char* who = "vbt_figure_set";
  if (n < 0 || (n > 0 && (!row_counts || !phase_counts))) { set_error("%s: bad argument (n %d, row counts %p, phase counts %p)", who, n, (const void*)row_counts, (const void*)phase_counts); return VBT_ERR_ARG; }
  if (n > FIG_MAX_FIGURES) { set_error("%s: %d figures, above %d", who, n, (int)FIG_MAX_FIGURES); return VBT_ERR_CAPACITY; }
  size_t nr = 0, np = 0;
  for (int f = 0; f < n; f++) {
    if (row_counts[f] < 0 || phase_counts[f] < 0) { set_error("%s: figure %d has a negative count (%d rows, %d phases)", who, f, row_counts[f], phase_counts[f]); return VBT_ERR_ARG; }
    if (row_counts[f] > FIG_MAX_ROWS) { set_error("%s: figure %d has %d rows, above %d", who, f, row_counts[f], (int)FIG_MAX_ROWS); return VBT_ERR_CAPACITY; }
    if (phase_counts[f] > FIG_MAX_PHASES) { set_error("%s: figure %d has %d phases, above %d", who, f, phase_counts[f], (int)FIG_MAX_PHASES); return VBT_ERR_CAPACITY; }
    nr += (size_t)row_counts[f]; np += (size_t)phase_counts[f];
  }
  if ((nr > 0 && !rows) || (np > 0 && !phases)) { set_error("%s: NULL rows or phases", who); return VBT_ERR_ARG; }
  const double *r = rows, *p = phases;
  for (int f = 0; f < n; f++) {
    for (int i = 0; i < row_counts[f]; i++, r += 7) {
      switch (fig_row_check(r, i > 0 ? r - 7 : nullptr)) {
        case 1: set_error("%s: figure %d, row %d holds a non-finite value", who, f, i); return VBT_ERR_ARG;
        case 2: set_error("%s: figure %d, row %d: time decreases", who, f, i); return VBT_ERR_ARG;
        default: break;
      }
    }
    for (int i = 0; i < phase_counts[f]; i++, p += 6) {
      switch (ov_hud_phase_check(p, i > 0 ? p - 6 : nullptr)) {
        case OV_HUD_PHASE_NONFINITE: set_error("%s: figure %d, phase %d holds a non-finite value", who, f, i); return VBT_ERR_ARG;
        case OV_HUD_PHASE_TYPE: set_error("%s: figure %d, phase %d has type %g, not 0, 1 or 2", who, f, i, p[5]); return VBT_ERR_ARG;
        case OV_HUD_PHASE_ENDS_BEFORE: set_error("%s: figure %d, phase %d ends before it starts (time_end < time_start)", who, f, i); return VBT_ERR_ARG;
        case OV_HUD_PHASE_ORDER: set_error("%s: figure %d: phases are not ordered in time at phase %d", who, f, i); return VBT_ERR_ARG;
        default: break;
      }
    }
  }
  *rows_total = nr; *phases_total = np;
  return VBT_OK;
}

}  // namespace

extern "C" {

void vbt_figure_default_params(vbt_figure_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->width = 1280; p->height = 800; p->scale = 2; p->thickness = 2; p->max_figures = 64; p->max_rows = 16384; p->max_phases = 512;
}

int vbt_figure_create(int device, const vbt_figure_params* params, vbt_figure** out) {
  if (!out) { set_error("vbt_figure_create: out is NULL"); return VBT_ERR_ARG; }
  *out = nullptr;
  vbt_figure_params p;
  vbt_figure_default_params(&p);
  if (params) p = *params;
  if (int rc = check_figure_params(p)) return rc;
  if (int rc = use_device("vbt_figure_create", device, /*set_current=*/true)) return rc;
  std::unique_ptr<vbt_figure> f(new vbt_figure());
  f->device = device; f->prm = p; f->G = fig_geom(p.width, p.height, p.scale, p.thickness);
  f->rec_cap = FIG_FIXED_RECS + 4 * p.max_phases;
  const size_t F = (size_t)p.max_figures, R = (size_t)p.max_rows;
  FigCarver C;
  C.add<uint8_t>(align64(F * FIG_META * 4) + F * R * 7 * 8 + F * (size_t)p.max_phases * 6 * 8);      // the largest upload, at the blob's head
  const auto head = C.add<double>(F * FIG_HEAD);
  const auto pts = C.add<int32_t>(F * R * FIG_PT);
  const auto recs = C.add<int32_t>(F * (size_t)f->rec_cap * FIG_REC);
  const auto nrec = C.add<int32_t>(F);
  const auto smooth = C.add<double>(F * 4 * R);
  if (f->blob.alloc(C.bytes()) != hipSuccess) {
    (void)hipGetLastError();
    set_error("vbt_figure_create: the device cannot give %zu bytes for %d figures of %d rows and %d phases", C.bytes(), p.max_figures, p.max_rows, p.max_phases);
    return VBT_ERR_HIP;
  }
  f->d_head = C.ptr(f->blob.get(), head); f->d_pts = C.ptr(f->blob.get(), pts); f->d_recs = C.ptr(f->blob.get(), recs);
  f->d_nrec = C.ptr(f->blob.get(), nrec); f->d_smooth = C.ptr(f->blob.get(), smooth);
  *out = f.release();
  return VBT_OK;
}

void vbt_figure_destroy(vbt_figure* f) { delete f; }

int vbt_figure_set(vbt_figure* f, int n, const double* rows7_host, const int32_t* row_counts, const double* phases6_host, const int32_t* phase_counts,
                   void* stream) {
  size_t nr = 0, np = 0;
  if (int rc = check_figure_set(n, rows7_host, row_counts, phases6_host, phase_counts, &nr, &np)) return rc;
  if (!f) { set_error("vbt_figure_set: handle is NULL"); return VBT_ERR_ARG; }
  if (n > f->prm.max_figures) { set_error("vbt_figure_set: %d figures, the handle holds %d", n, f->prm.max_figures); return VBT_ERR_CAPACITY; }
  for (int i = 0; i < n; i++) {
    if (row_counts[i] > f->prm.max_rows) { set_error("vbt_figure_set: figure %d has %d rows, the handle holds %d", i, row_counts[i], f->prm.max_rows); return VBT_ERR_CAPACITY; }
    if (phase_counts[i] > f->prm.max_phases) { set_error("vbt_figure_set: figure %d has %d phases, the handle holds %d", i, phase_counts[i], f->prm.max_phases); return VBT_ERR_CAPACITY; }
  }
  VBT_HIP_CHECK(hipSetDevice(f->device));
  f->n = 0;
  if (n == 0) return VBT_OK;
  const size_t meta_b = align64((size_t)n * FIG_META * 4), rows_b = nr * 7 * 8, ph_b = np * 6 * 8;
  std::vector<uint8_t> up(meta_b + rows_b + ph_b, 0);
  int32_t* meta = (int32_t*)up.data();
  size_t r0 = 0, p0 = 0;
  for (int i = 0; i < n; i++) {
    int32_t* m = meta + (size_t)i * FIG_META;
    m[0] = row_counts[i]; m[1] = phase_counts[i]; m[2] = (int32_t)r0; m[3] = (int32_t)p0;
    r0 += (size_t)row_counts[i]; p0 += (size_t)phase_counts[i];
  }
  if (rows_b) memcpy(up.data() + meta_b, rows7_host, rows_b);
  if (ph_b) memcpy(up.data() + meta_b + rows_b, phases6_host, ph_b);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(f->blob.get(), up.data(), up.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    FigPrepArgs A{};
    A.meta = (const int32_t*)f->blob.get(); A.rows = (const double*)(f->blob.get() + meta_b); A.phases = (const double*)(f->blob.get() + meta_b + rows_b);
    A.smooth = f->d_smooth; A.head = f->d_head; A.pts = f->d_pts; A.recs = f->d_recs; A.nrec = f->d_nrec;
    A.G = f->G; A.max_rows = f->prm.max_rows; A.rec_cap = f->rec_cap;
    figure_prepare_kernel<<<dim3((unsigned)n), FIG_THREADS, 0, st>>>(A);
    e = hipGetLastError();
  }
  if (int rc = f->finish_set("vbt_figure_set", st, e)) return rc;      // (`up` leaves scope: the copy must have read it)
  f->meta.assign(meta, meta + (size_t)n * FIG_META);
  f->n = n;
  return VBT_OK;
}

int vbt_figure_render(vbt_figure* f, uint8_t* frames_dev, int fig0, int n, void* stream) {
  if (int rc = check_render_args("vbt_figure_render", "vbt_figure_set", f, frames_dev, fig0, n)) return rc;
  if (n == 0) return VBT_OK;
  VBT_HIP_CHECK(hipSetDevice(f->device));
  FigRenderArgs A{};
  A.meta = (const int32_t*)f->blob.get(); A.pts = f->d_pts; A.recs = f->d_recs; A.nrec = f->d_nrec;
  A.frames = frames_dev; A.frame_bytes = (size_t)f->G.W * f->G.H * 3;
  A.G = f->G; A.max_rows = f->prm.max_rows; A.rec_cap = f->rec_cap; A.fig0 = fig0;
  A.tiles_x = (f->G.W + RASTER_TILE_W - 1) / RASTER_TILE_W;
  A.words = f->G.W % 4 == 0 && ((uintptr_t)frames_dev & 3) == 0;
  const int tiles_y = (f->G.H + FIG_TILE_H - 1) / FIG_TILE_H;
  figure_render_kernel<<<dim3((unsigned)(A.tiles_x * tiles_y), (unsigned)n), FIG_THREADS, 0, (hipStream_t)stream>>>(A);
  VBT_HIP_CHECK(hipGetLastError());
  f->last = (hipStream_t)stream;
  return VBT_OK;
}

int vbt_figure_table(vbt_figure* f, int fig, double* head6, int32_t* points, int cap_points, int* n_points, int32_t* records, int cap_records,
                     int* n_records) {
  if (!f || !head6 || !n_points || !n_records || cap_points < 0 || cap_records < 0 || (cap_points > 0 && !points) || (cap_records > 0 && !records)) {
    set_error("vbt_figure_table: bad argument");
    return VBT_ERR_ARG;
  }
  int32_t nrec = 0;
  if (int rc = table_begin("vbt_figure_table", "vbt_figure_set", f, fig, &nrec)) return rc;
  VBT_HIP_CHECK(hipMemcpy(head6, f->d_head + (size_t)fig * FIG_HEAD, FIG_HEAD * 8, hipMemcpyDeviceToHost));
  const int T = f->meta[(size_t)fig * FIG_META];
  *n_points = T; *n_records = nrec;
  if (cap_points < T || cap_records < nrec) { set_error("vbt_figure_table: %d points and %d records, room for %d and %d", T, nrec, cap_points, cap_records); return VBT_ERR_CAPACITY; }
  if (T > 0) VBT_HIP_CHECK(hipMemcpy(points, f->d_pts + (size_t)fig * f->prm.max_rows * FIG_PT, (size_t)T * FIG_PT * 4, hipMemcpyDeviceToHost));
  if (nrec > 0) VBT_HIP_CHECK(hipMemcpy(records, f->d_recs + (size_t)fig * f->rec_cap * FIG_REC, (size_t)nrec * FIG_REC * 4, hipMemcpyDeviceToHost));
  return VBT_OK;
}

}  // extern "C"
