// Tracking overlay on the device (gfx950): box, id label, marker and bar path of the tracked plates drawn into frames that are
// already in device memory (include/vbt_hip.h, "tracking overlay"; reference track.py:28-62,201-224).  Two kernels:
//   overlay_prepare_kernel, once per vbt_overlay_set_rows: one thread per row - frame number, the six pixel coordinates, trail length;
//   overlay_draw_kernel, once per vbt_overlay_draw: grid (row slot x chunk, frame of the batch).  A frame's rows come from the dense
//     index frame number -> rows (the host builds it while it validates the rows; it sizes the grid from it).  Chunk 0 of a row is its
//     box outline (a few thousand pixels), chunk 1 its marker and label, chunk 2 + j the 16 trail segments 16 j .. 16 j + 15, one per
//     16-lane group: a segment is a few dozen candidate pixels, so a wavefront takes four of them and a workgroup sixteen.
// Nothing reads a pixel and nothing passes over a frame: a workgroup walks its primitive clipped to the frame (overlay_core.h).
#include <algorithm>

#include "common.h"
#include "overlay_core.h"

namespace vbt {

constexpr int OV_THREADS = 256;
constexpr int OV_SEG_LANES = 16;                                  // lanes per trail segment
constexpr int OV_SEGS_PER_BLOCK = OV_THREADS / OV_SEG_LANES;
constexpr int OV_MAX_FRAME = 1 << 24;                             // the frame index is dense: 64 MB at most

struct OverlayDrawArgs {
  const int32_t* geom;     // [n][OV_GEOM]
  const int64_t* ids;      // row i's id at ids[8 i] (the rows as uploaded)
  const int32_t* fstart;   // [fmax + 2]: rows of frame f are frow[fstart[f] .. fstart[f + 1])
  const int32_t* frow;     // [n] row numbers ordered by frame
  uint8_t* frames;
  size_t frame_bytes;
  int frame0, frame_step, fmax, chunks;
  int H, W, fmt, t, R, s, label, box;
  uint8_t c0, c1, c2;
};

__global__ __launch_bounds__(OV_THREADS) void overlay_prepare_kernel(const OverlayRow* __restrict__ rows, int n, double fps, int H, int W, int trail,
                                                                       int32_t* __restrict__ geom) {
  const int i = blockIdx.x * OV_THREADS + threadIdx.x;
  if (i >= n) return;
  int32_t g[OV_GEOM];
  ov_row_geometry(rows[i], fps, H, W, g);
  // rows are sorted by (id, time): the rows of the same id before row i are a contiguous slice ending at i
  const int64_t id = rows[i].id;
  int lo = 0, hi = trail - 1 < i ? trail - 1 : i;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[i - mid].id == id) lo = mid; else hi = mid - 1;
  }
  g[OV_TRAIL] = lo + 1;
#pragma unroll
  for (int k = 0; k < OV_GEOM; k++) geom[(size_t)i * OV_GEOM + k] = g[k];
}

__global__ __launch_bounds__(OV_THREADS) void overlay_draw_kernel(OverlayDrawArgs A) {
  const long f = (long)A.frame0 + (long)blockIdx.y * A.frame_step;
  if (f < 1 || f > A.fmax) return;
  const int slot = blockIdx.x / A.chunks, chunk = blockIdx.x % A.chunks;
  const int r0 = A.fstart[f], r1 = A.fstart[f + 1];
  if (slot >= r1 - r0) return;
  const int row = A.frow[r0 + slot];
  const int32_t* g = A.geom + (size_t)row * OV_GEOM;
  Painter P{A.frames + (size_t)blockIdx.y * A.frame_bytes, A.H, A.W, A.fmt, A.c0, A.c1, A.c2};
  const int lane = threadIdx.x;
  if (chunk == 0) {
    if (A.box) ov_draw_box(P, g, A.t, lane, OV_THREADS);
  } else if (chunk == 1) {
    ov_draw_marker(P, g, A.R, lane, OV_THREADS);
    if (A.label) {                                                // (uniform over the workgroup, like `chunk`)
      __shared__ uint8_t chars[OV_MAX_CHARS];
      __shared__ int nchars;
      if (lane == 0) nchars = ov_label_chars(A.ids[(size_t)row * 8], chars);
      __syncthreads();
      ov_draw_label(P, g, chars, nchars, A.s, lane, OV_THREADS);
    }
  } else {
    // trail point k (0 = oldest) of this row is the centre of row (row - (trail length - 1) + k); segment s joins points s, s + 1
    const int nseg = g[OV_TRAIL] - 1;
    const int seg = (chunk - 2) * OV_SEGS_PER_BLOCK + lane / OV_SEG_LANES;
    if (seg >= nseg) return;
    const int32_t* p0 = A.geom + (size_t)(row - nseg + seg) * OV_GEOM;
    ov_draw_segment(P, p0[OV_CX], p0[OV_CY], p0[OV_GEOM + OV_CX], p0[OV_GEOM + OV_CY], A.t, lane % OV_SEG_LANES, OV_SEG_LANES);
  }
}

}  // namespace vbt

using namespace vbt;

struct vbt_overlay {
  int device = 0, H = 0, W = 0, fmt = 0;
  vbt_overlay_params prm{};
  uint8_t c0 = 0, c1 = 0, c2 = 0;        // the colour in the frames' format
  size_t frame_bytes = 0;
  int chunks = 2;                        // workgroups per row: box, marker + label, ceil((trail - 1) / 16) of trail segments
  int n = 0, fmax = 0;
  uint8_t* blob = nullptr;               // rows | frow | fstart | geom in one allocation
  const OverlayRow* d_rows = nullptr;
  const int32_t *d_frow = nullptr, *d_fstart = nullptr;
  int32_t* d_geom = nullptr;
  std::vector<int32_t> fstart;           // the host's copy of the index: sizes the grid of a draw
};

namespace {

// the refusals of vbt_overlay_set_rows that need no handle and no device
int check_rows(const OverlayRow* rows, int n, double fps) {
  if (n < 0 || (n > 0 && !rows)) { set_error("vbt_overlay_set_rows: bad argument (n %d, rows %p)", n, (const void*)rows); return VBT_ERR_ARG; }
  if (!(fps > 0) || !std::isfinite(fps)) { set_error("vbt_overlay_set_rows: fps must be positive and finite, got %g", fps); return VBT_ERR_ARG; }
  for (int i = 0; i < n; i++) {
    const OverlayRow& r = rows[i];
    const double v[7] = {r.time, r.x, r.y, r.dx, r.dy, r.h, r.w};
    for (double d : v)
      if (!std::isfinite(d)) { set_error("vbt_overlay_set_rows: row %d holds a non-finite value", i); return VBT_ERR_ARG; }
    if (r.id < 0) { set_error("vbt_overlay_set_rows: row %d has a negative id %lld", i, (long long)r.id); return VBT_ERR_ARG; }
    if (r.w < 0 || r.h < 0) { set_error("vbt_overlay_set_rows: row %d has a negative plate width or height", i); return VBT_ERR_ARG; }
    if (i > 0 && (rows[i - 1].id > r.id || (rows[i - 1].id == r.id && rows[i - 1].time > r.time))) {
      set_error("vbt_overlay_set_rows: rows are not sorted by (id, time) at row %d", i);
      return VBT_ERR_ARG;
    }
  }
  return VBT_OK;
}

void overlay_free_rows(vbt_overlay* o) {
  if (o->blob) (void)hipFree(o->blob);   // (waits for the draws still reading it)
  o->blob = nullptr; o->d_rows = nullptr; o->d_frow = o->d_fstart = nullptr; o->d_geom = nullptr;
  o->n = 0; o->fmax = 0; o->fstart.clear();
}

}  // namespace

extern "C" {

void vbt_overlay_default_params(vbt_overlay_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->trail = 120; p->thickness = 2; p->radius = 10; p->label_scale = 3;
  p->rgb[0] = p->rgb[1] = p->rgb[2] = 255;
  p->label = 1; p->box = 1;
}

int vbt_overlay_create(int device, int H, int W, int pix_fmt, const vbt_overlay_params* params, vbt_overlay** out) {
  if (!out) { set_error("vbt_overlay_create: out is NULL"); return VBT_ERR_ARG; }
  *out = nullptr;
  vbt_overlay_params p;
  vbt_overlay_default_params(&p);
  if (params) p = *params;
  if (pix_fmt != VBT_PIX_RGB24 && !pix_fmt_is_yuv(pix_fmt)) { set_error("vbt_overlay_create: unknown pixel format %d", pix_fmt); return VBT_ERR_ARG; }
  if (H < 1 || W < 1 || H > 16384 || W > 16384) { set_error("vbt_overlay_create: frames of 1..16384 pixels a side, got %d x %d", H, W); return VBT_ERR_ARG; }
  if (pix_fmt_is_yuv(pix_fmt) && ((H & 1) || (W & 1))) { set_error("vbt_overlay_create: YUV 4:2:0 frames have even H and W, got %d x %d", H, W); return VBT_ERR_ARG; }
  if (p.trail < 1 || p.trail > 65536) { set_error("vbt_overlay_create: trail %d outside 1..65536", p.trail); return VBT_ERR_ARG; }
  if (p.thickness < 0 || p.thickness > 1024) { set_error("vbt_overlay_create: thickness %d outside 0..1024", p.thickness); return VBT_ERR_ARG; }
  if (p.radius < 0 || p.radius > 16384) { set_error("vbt_overlay_create: radius %d outside 0..16384", p.radius); return VBT_ERR_ARG; }
  if (p.label_scale < 1 || p.label_scale > 64) { set_error("vbt_overlay_create: label_scale %d outside 1..64", p.label_scale); return VBT_ERR_ARG; }
  if (int rc = use_device("vbt_overlay_create", device, /*set_current=*/false)) return rc;
  vbt_overlay* o = new vbt_overlay();
  o->device = device; o->H = H; o->W = W; o->fmt = pix_fmt; o->prm = p;
  const int r = p.rgb[0], g = p.rgb[1], b = p.rgb[2];
  if (pix_fmt == VBT_PIX_RGB24) {
    o->c0 = (uint8_t)r; o->c1 = (uint8_t)g; o->c2 = (uint8_t)b;
    o->frame_bytes = (size_t)H * W * 3;
  } else {
    o->c0 = (uint8_t)(((66 * r + 129 * g + 25 * b + 128) >> 8) + 16);
    o->c1 = (uint8_t)(((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128);
    o->c2 = (uint8_t)(((112 * r - 94 * g - 18 * b + 128) >> 8) + 128);
    o->frame_bytes = (size_t)H * W * 3 / 2;
  }
  o->chunks = 2 + (p.trail - 1 + OV_SEGS_PER_BLOCK - 1) / OV_SEGS_PER_BLOCK;
  *out = o;
  return VBT_OK;
}

void vbt_overlay_destroy(vbt_overlay* o) {
  if (!o) return;
  if (hipSetDevice(o->device) == hipSuccess) overlay_free_rows(o);
  delete o;
}

int vbt_overlay_set_rows(vbt_overlay* o, const void* rows_host, int n, double fps, void* stream) {
  const OverlayRow* rows = (const OverlayRow*)rows_host;
  if (int rc = check_rows(rows, n, fps)) return rc;
  if (!o) { set_error("vbt_overlay_set_rows: handle is NULL"); return VBT_ERR_ARG; }
  // frame numbers, by the statement the prepare kernel runs: the dense index frame -> rows, a counting sort
  std::vector<int32_t> frame((size_t)n);
  int fmax = 0;
  for (int i = 0; i < n; i++) {
    frame[i] = ov_frame_number(rows[i].time, fps);
    if (frame[i] > OV_MAX_FRAME) { set_error("vbt_overlay_set_rows: row %d is frame %d, above %d", i, frame[i], OV_MAX_FRAME); return VBT_ERR_CAPACITY; }
    fmax = std::max(fmax, frame[i]);
  }
  VBT_HIP_CHECK(hipSetDevice(o->device));
  overlay_free_rows(o);
  if (n == 0) return VBT_OK;
  std::vector<int32_t> fstart((size_t)fmax + 2, 0), frow((size_t)n, 0);
  for (int i = 0; i < n; i++)
    if (frame[i] >= 1) fstart[(size_t)frame[i] + 1]++;           // rows of frames < 1 are never drawn; they still feed trails
  for (int f = 1; f <= fmax + 1; f++) fstart[f] += fstart[f - 1];
  {
    std::vector<int32_t> next(fstart.begin(), fstart.end() - 1);
    for (int i = 0; i < n; i++)
      if (frame[i] >= 1) frow[next[frame[i]]++] = i;
  }
  const size_t rows_b = (size_t)n * sizeof(OverlayRow), frow_b = (size_t)n * 4, fstart_b = fstart.size() * 4;
  const size_t up_b = (rows_b + frow_b + fstart_b + 31) & ~(size_t)31, geom_b = (size_t)n * OV_GEOM * 4;
  std::vector<uint8_t> up(up_b, 0);
  memcpy(up.data(), rows, rows_b);
  memcpy(up.data() + rows_b, frow.data(), frow_b);
  memcpy(up.data() + rows_b + frow_b, fstart.data(), fstart_b);
  VBT_HIP_CHECK(hipMalloc((void**)&o->blob, up_b + geom_b));
  o->d_rows = (const OverlayRow*)o->blob;
  o->d_frow = (const int32_t*)(o->blob + rows_b);
  o->d_fstart = (const int32_t*)(o->blob + rows_b + frow_b);
  o->d_geom = (int32_t*)(o->blob + up_b);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(o->blob, up.data(), up_b, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    overlay_prepare_kernel<<<dim3((unsigned)((n + OV_THREADS - 1) / OV_THREADS)), OV_THREADS, 0, st>>>(o->d_rows, n, fps, o->H, o->W, o->prm.trail, o->d_geom);
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(st);                 // (`up` leaves scope: the copy must have read it)
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    overlay_free_rows(o);
    set_error("vbt_overlay_set_rows failed: %s", hipGetErrorString(e));
    return VBT_ERR_HIP;
  }
  o->n = n; o->fmax = fmax; o->fstart = std::move(fstart);
  return VBT_OK;
}

int vbt_overlay_draw(vbt_overlay* o, uint8_t* frames_dev, int B, int frame0, int frame_step, void* stream) {
  if (!o || !frames_dev || B < 0 || frame0 < 1 || frame_step < 1 || (long)frame0 + (long)(B - 1) * frame_step > INT32_MAX) {
    set_error("vbt_overlay_draw: bad argument (B >= 0, frame0 >= 1, frame_step >= 1, frame numbers inside int32)");
    return VBT_ERR_ARG;
  }
  if (B == 0 || o->n == 0) return VBT_OK;
  VBT_HIP_CHECK(hipSetDevice(o->device));
  OverlayDrawArgs A{};
  A.geom = o->d_geom; A.ids = (const int64_t*)o->d_rows; A.fstart = o->d_fstart; A.frow = o->d_frow;
  A.frame_bytes = o->frame_bytes; A.frame_step = frame_step; A.fmax = o->fmax; A.chunks = o->chunks;
  A.H = o->H; A.W = o->W; A.fmt = o->fmt; A.t = o->prm.thickness; A.R = o->prm.radius; A.s = o->prm.label_scale;
  A.label = o->prm.label; A.box = o->prm.box; A.c0 = o->c0; A.c1 = o->c1; A.c2 = o->c2;
  constexpr int MAX_Y = 32768;                                    // frames per launch (grid.y)
  for (int b0 = 0; b0 < B; b0 += MAX_Y) {
    const int nb = std::min(MAX_Y, B - b0);
    int most = 0;                                                 // rows of the fullest frame of this launch
    for (int i = 0; i < nb; i++) {
      const long f = (long)frame0 + (long)(b0 + i) * frame_step;
      if (f > o->fmax) break;
      most = std::max(most, o->fstart[f + 1] - o->fstart[f]);
    }
    if (most == 0) continue;
    A.frames = frames_dev + (size_t)b0 * o->frame_bytes;
    A.frame0 = (int)((long)frame0 + (long)b0 * frame_step);
    overlay_draw_kernel<<<dim3((unsigned)most * (unsigned)o->chunks, (unsigned)nb), OV_THREADS, 0, (hipStream_t)stream>>>(A);
  }
  VBT_HIP_CHECK(hipGetLastError());
  return VBT_OK;
}

int vbt_overlay_geometry(vbt_overlay* o, int32_t* out, int cap, int* n) {
  if (!o || !n || cap < 0 || (cap > 0 && !out)) { set_error("vbt_overlay_geometry: bad argument"); return VBT_ERR_ARG; }
  *n = o->n;
  if (cap < o->n) { set_error("vbt_overlay_geometry: %d rows, room for %d", o->n, cap); return VBT_ERR_CAPACITY; }
  if (o->n == 0) return VBT_OK;
  VBT_HIP_CHECK(hipSetDevice(o->device));
  VBT_HIP_CHECK(hipMemcpy(out, o->d_geom, (size_t)o->n * OV_GEOM * 4, hipMemcpyDeviceToHost));
  return VBT_OK;
}

}  // extern "C"
