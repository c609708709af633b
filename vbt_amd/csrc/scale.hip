// Scaled export on the device (gfx950): frames of H x W in, frames of h x w out, in the source's own pixel format
// (include/vbt_hip.h, "Scaled export": the contract; scale_core.h: its statements; tests/scale_ref.py: the numpy statement of it).
//   scale_kernel  grid (tile, frame), one launch per vbt_scaler_run.  A tile is 4 rows of 256 output bytes of one plane; a wavefront
//     takes a row, so the row's table entry (y0, ay) is wave-uniform and loaded once, and a lane produces 4 consecutive output bytes
//     of it: per byte the x entry of its pixel and four taps.  The 4 bytes leave as one 32-bit store where the plane's rows begin
//     4-aligned (base, frame size, plane offset and row bytes all multiples of 4), as bytes otherwise.  Nothing but the taps is read;
//     every byte of dst is written once.
// The tables are built on the host in double (sc_axis_table) and uploaded once per handle.
#include <algorithm>

#include "common.h"
#include "dev_mem.h"
#include "scale_core.h"

namespace vbt {

constexpr int SC_THREADS = 256;
constexpr int SC_RUN = 4;                                // output bytes per lane
constexpr int SC_TILE_BYTES = 64 * SC_RUN;               // of a row, per wavefront
constexpr int SC_TILE_ROWS = SC_THREADS / 64;
constexpr int SC_MAX_FRAMES = 65535;                     // grid.y

struct ScPlane {
  const ScTap *ty, *tx;
  size_t src_off, dst_off;
  int src_rows, src_n, src_row_bytes, dst_rows, dst_row_bytes, C;
  int tiles_x, tile0;                                    // tiles per row of tiles; the plane's first tile in the grid
  int words;                                             // every run of the plane is 4 whole bytes at a 4-aligned address
};

struct ScArgs {
  const uint8_t* src;
  uint8_t* dst;
  size_t src_frame, dst_frame;
  int n_planes;
  ScPlane p[3];
};

template <int C>
__device__ __forceinline__ void scale_tile(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const ScPlane& P, int tile) {
  const int tr = tile / P.tiles_x, tc = tile - tr * P.tiles_x;
  const int y = tr * SC_TILE_ROWS + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int j0 = (tc * 64 + (int)(threadIdx.x & 63)) * SC_RUN;
  if (y >= P.dst_rows || j0 >= P.dst_row_bytes) return;
  const ScTap ty = P.ty[y];
  const uint8_t* r0 = src + P.src_off + (size_t)ty.i0 * P.src_row_bytes;
  const uint8_t* r1 = src + P.src_off + (size_t)sc_i1(ty.i0, P.src_rows) * P.src_row_bytes;
  const int n = min(SC_RUN, P.dst_row_bytes - j0);
  uint32_t word = 0;
#pragma unroll
  for (int e = 0; e < SC_RUN; e++) {
    if (e >= n) break;
    const int j = j0 + e, px = j / C, c = j - px * C;
    const ScTap tx = P.tx[px];
    word |= (uint32_t)sc_sample_at(r0, r1, C, c, tx.i0, sc_i1(tx.i0, P.src_n), tx.a, ty.a) << (8 * e);
  }
  uint8_t* d = dst + P.dst_off + (size_t)y * P.dst_row_bytes + j0;
  if (P.words) {
    *(uint32_t*)d = word;
  } else {
    for (int e = 0; e < n; e++) d[e] = (uint8_t)(word >> (8 * e));
  }
}

__global__ __launch_bounds__(SC_THREADS) void scale_kernel(ScArgs A) {
  const int b = (int)blockIdx.x;
  const int k = (A.n_planes > 1 && b >= A.p[1].tile0) + (A.n_planes > 2 && b >= A.p[2].tile0);
  const ScPlane& P = A.p[k];
  const uint8_t* src = A.src + (size_t)blockIdx.y * A.src_frame;
  uint8_t* dst = A.dst + (size_t)blockIdx.y * A.dst_frame;
  switch (P.C) {
    case 1: scale_tile<1>(src, dst, P, b - P.tile0); break;
    case 2: scale_tile<2>(src, dst, P, b - P.tile0); break;
    default: scale_tile<3>(src, dst, P, b - P.tile0); break;
  }
}

}  // namespace vbt

using namespace vbt;

struct vbt_scaler {
  int device = 0, H = 0, W = 0, h = 0, w = 0, fmt = 0;
  ScTableLayout L{};
  DevBuf<ScTap> tab;
  ScArgs args{};
  unsigned tiles = 0;
};

namespace {

// a frame size the scaler takes: VBT_ERR_ARG naming the pair otherwise
int check_size(const char* who, const char* names, int H, int W, int pix_fmt) {
  const int eh = sc_check_side(H, pix_fmt), ew = sc_check_side(W, pix_fmt);
  if (eh == 1 || ew == 1) { set_error("%s: %s of 1..%d pixels a side, got %d x %d", who, names, SC_MAX_SIDE, H, W); return VBT_ERR_ARG; }
  if (eh || ew) { set_error("%s: YUV 4:2:0 frames have even %s, got %d x %d", who, names, H, W); return VBT_ERR_ARG; }
  return VBT_OK;
}

}  // namespace

extern "C" {

int vbt_display_size(int H, int W, int pix_fmt, int display_height, int* h, int* w) {
  const char* who = "vbt_display_size";
  if (!h || !w) { set_error("%s: h or w is NULL", who); return VBT_ERR_ARG; }
  if (pix_fmt != VBT_PIX_RGB24 && !sc_is_yuv(pix_fmt)) { set_error("%s: unknown pixel format %d (pix_fmt)", who, pix_fmt); return VBT_ERR_ARG; }
  if (int rc = check_size(who, "H and W", H, W, pix_fmt)) return rc;
  if (display_height < 1 || display_height > SC_MAX_SIDE) { set_error("%s: display_height %d outside 1..%d", who, display_height, SC_MAX_SIDE); return VBT_ERR_ARG; }
  if (sc_check_side(display_height, pix_fmt)) { set_error("%s: display_height %d is odd: YUV 4:2:0 frames have an even height", who, display_height); return VBT_ERR_ARG; }
  int hh, ww;
  sc_display_size(H, W, pix_fmt, display_height, &hh, &ww);
  if (sc_check_side(ww, pix_fmt)) {
    set_error("%s: display_height %d gives a width of %d for a %d x %d (W x H) source, outside %d..%d", who, display_height, ww, W, H, sc_is_yuv(pix_fmt) ? 2 : 1, SC_MAX_SIDE);
    return VBT_ERR_ARG;
  }
  *h = hh; *w = ww;
  return VBT_OK;
}

int vbt_scaler_create(int device, int H, int W, int h, int w, int pix_fmt, vbt_scaler** out) {
  const char* who = "vbt_scaler_create";
  if (!out) { set_error("%s: out is NULL", who); return VBT_ERR_ARG; }
  *out = nullptr;
  if (pix_fmt != VBT_PIX_RGB24 && !sc_is_yuv(pix_fmt)) { set_error("%s: unknown pixel format %d (pix_fmt)", who, pix_fmt); return VBT_ERR_ARG; }
  if (int rc = check_size(who, "H and W", H, W, pix_fmt)) return rc;
  if (int rc = check_size(who, "h and w", h, w, pix_fmt)) return rc;
  std::unique_ptr<vbt_scaler> s(new vbt_scaler());
  s->device = device; s->H = H; s->W = W; s->h = h; s->w = w; s->fmt = pix_fmt;
  s->L = sc_table_layout(h, w, pix_fmt);
  std::vector<ScTap> host((size_t)s->L.total);
  sc_build_tables(H, W, h, w, pix_fmt, s->L, host.data());
  if (int rc = use_device(who, device)) return rc;
  hipError_t e = s->tab.alloc(host.size());
  if (e == hipSuccess) e = hipMemcpy(s->tab.get(), host.data(), host.size() * sizeof(ScTap), hipMemcpyHostToDevice);   // the four tables, one copy
  if (e != hipSuccess) { set_error("%s: %zu bytes of device memory for the tables: %s", who, host.size() * sizeof(ScTap), hipGetErrorString(e)); return VBT_ERR_HIP; }
  ScArgs& A = s->args;
  A.src_frame = sc_frame_bytes(H, W, pix_fmt); A.dst_frame = sc_frame_bytes(h, w, pix_fmt);
  ScPlaneGeom G[3];
  A.n_planes = sc_planes(H, W, h, w, pix_fmt, G);
  unsigned tiles = 0;
  for (int k = 0; k < A.n_planes; k++) {
    ScPlane& P = A.p[k];
    const ScPlaneGeom& g = G[k];
    P.ty = s->tab.get() + s->L.at[g.chroma][0]; P.tx = s->tab.get() + s->L.at[g.chroma][1];
    P.src_off = g.src_off; P.dst_off = g.dst_off;
    P.src_rows = g.src_rows; P.src_n = g.src_n; P.src_row_bytes = g.src_n * g.C;
    P.dst_rows = g.dst_rows; P.dst_row_bytes = g.dst_n * g.C; P.C = g.C;
    P.tiles_x = (P.dst_row_bytes + SC_TILE_BYTES - 1) / SC_TILE_BYTES;
    P.tile0 = (int)tiles;
    P.words = A.dst_frame % 4 == 0 && g.dst_off % 4 == 0 && P.dst_row_bytes % 4 == 0;       // and a 4-aligned dst: vbt_scaler_run
    tiles += (unsigned)P.tiles_x * (unsigned)((P.dst_rows + SC_TILE_ROWS - 1) / SC_TILE_ROWS);
  }
  s->tiles = tiles;
  *out = s.release();
  return VBT_OK;
}

void vbt_scaler_destroy(vbt_scaler* s) {
  if (!s) return;
  if (s->tab) (void)hipSetDevice(s->device);
  delete s;   // (the tables' free waits for the kernels still using them)
}

int vbt_scaler_run(vbt_scaler* s, const uint8_t* src_dev, uint8_t* dst_dev, int B, void* stream) {
  const char* who = "vbt_scaler_run";
  if (!s || !src_dev || !dst_dev || B < 1) { set_error("%s: bad argument (handle %p, src_dev %p, dst_dev %p, B %d >= 1)", who, (const void*)s, (const void*)src_dev, (const void*)dst_dev, B); return VBT_ERR_ARG; }
  if (B > SC_MAX_FRAMES) { set_error("%s: %d frames, above %d in one call", who, B, SC_MAX_FRAMES); return VBT_ERR_CAPACITY; }
  VBT_HIP_CHECK(hipSetDevice(s->device));
  ScArgs A = s->args;
  A.src = src_dev; A.dst = dst_dev;
  if ((uintptr_t)dst_dev & 3)
    for (int k = 0; k < A.n_planes; k++) A.p[k].words = 0;
  scale_kernel<<<dim3(s->tiles, (unsigned)B), SC_THREADS, 0, (hipStream_t)stream>>>(A);
  VBT_HIP_CHECK(hipGetLastError());
  return VBT_OK;
}

int vbt_scaler_tables(vbt_scaler* s, int plane, int axis, int32_t* i0, int32_t* a, int cap, int* n) {
  const char* who = "vbt_scaler_tables";
  if (!s || !n || cap < 0 || (cap > 0 && (!i0 || !a))) { set_error("%s: bad argument (handle, n, cap >= 0, i0 and a with cap > 0)", who); return VBT_ERR_ARG; }
  if (plane < 0 || plane > 1 || axis < 0 || axis > 1 || s->L.n[plane][axis] == 0) {
    set_error("%s: plane %d, axis %d: plane 0 (luma or RGB) or, with a YUV handle, 1 (chroma); axis 0 (y) or 1 (x)", who, plane, axis);
    return VBT_ERR_ARG;
  }
  const int cnt = s->L.n[plane][axis];
  *n = cnt;
  if (cap < cnt) { set_error("%s: %d entries, room for %d", who, cnt, cap); return VBT_ERR_CAPACITY; }
  VBT_HIP_CHECK(hipSetDevice(s->device));
  std::vector<ScTap> t((size_t)cnt);
  VBT_HIP_CHECK(hipMemcpy(t.data(), s->tab.get() + s->L.at[plane][axis], t.size() * sizeof(ScTap), hipMemcpyDeviceToHost));
  for (int k = 0; k < cnt; k++) { i0[k] = t[(size_t)k].i0; a[k] = t[(size_t)k].a; }
  return VBT_OK;
}

}  // extern "C"
