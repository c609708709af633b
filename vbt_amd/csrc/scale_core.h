// Scaled export (include/vbt_hip.h, "Scaled export"): the size rule, the axis table and the four-tap sample, as host + device
// statements, so that the kernels of scale.hip and mjpeg.hip and a host loop (tests/fuzz/scale_check.cc) run the same ones.
// No kernel lives here.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else   // a host compiler (tests/fuzz/scale_check.cc): the same statements, no HIP header needed
#include <stddef.h>
#define __host__
#define __device__
#endif
#include <math.h>

#include "../../include/vbt_hip.h"

namespace vbt {

constexpr int SC_MAX_SIDE = 16384;
constexpr int SC_ONE = 2048;                // the weight of a whole pixel: 11 bits per axis, 22 per sample

struct ScTap { int32_t i0, a; };            // one entry of an axis table: the first source index and the weight of the second

inline bool sc_is_yuv(int pix_fmt) { return pix_fmt == VBT_PIX_NV12 || pix_fmt == VBT_PIX_I420; }

// What is wrong with a side of a frame in `pix_fmt`: 0 = nothing, 1 = outside 1..16384, 2 = odd with a YUV format
inline int sc_check_side(int n, int pix_fmt) {
  if (n < 1 || n > SC_MAX_SIDE) return 1;
  return sc_is_yuv(pix_fmt) && (n & 1) ? 2 : 0;
}

// (h, w) of a source of H x W shown display_height lines high: the reference's int(h * (float(W) / float(H))), in double, truncated;
// YUV 4:2:0: w rounded down to even.  The sides are not checked here (sc_check_side).
inline void sc_display_size(int H, int W, int pix_fmt, int display_height, int* h, int* w) {
  const double ratio = (double)W / (double)H;
  double v = (double)display_height * ratio;
  v = v < 0.0 ? 0.0 : (v > 1073741824.0 ? 1073741824.0 : v);
  int ww = (int)v;
  if (sc_is_yuv(pix_fmt)) ww &= ~1;
  *h = display_height;
  *w = ww;
}

// The table of an axis with n_src source and n_dst destination samples (half-pixel centres), in double; a lies in 0..2048.
inline void sc_axis_table(int n_src, int n_dst, ScTap* t) {
  const double step = (double)n_src / (double)n_dst;
  for (int o = 0; o < n_dst; o++) {
    double f = ((double)o + 0.5) * step - 0.5;
    f = f > 0.0 ? f : 0.0;
    int i0 = (int)floor(f);
    i0 = i0 < n_src - 1 ? i0 : n_src - 1;
    t[o].i0 = i0;
    t[o].a = (int32_t)rint((f - (double)i0) * (double)SC_ONE);
  }
}

// The tables of a handle, one after the other: plane 0 (luma, or RGB) y [h] and x [w], then for YUV plane 1 (chroma) y [h/2] and x [w/2]
struct ScTableLayout {
  int at[2][2], n[2][2];                    // [plane][axis: 0 = y, 1 = x]
  int total;
};
inline ScTableLayout sc_table_layout(int h, int w, int pix_fmt) {
  ScTableLayout L{};
  const int c = sc_is_yuv(pix_fmt) ? 1 : 0;
  L.n[0][0] = h; L.n[0][1] = w; L.n[1][0] = c * (h / 2); L.n[1][1] = c * (w / 2);
  L.at[0][0] = 0; L.at[0][1] = h; L.at[1][0] = h + w; L.at[1][1] = h + w + L.n[1][0];
  L.total = L.at[1][1] + L.n[1][1];
  return L;
}
inline void sc_build_tables(int H, int W, int h, int w, int pix_fmt, const ScTableLayout& L, ScTap* t) {
  sc_axis_table(H, h, t + L.at[0][0]);
  sc_axis_table(W, w, t + L.at[0][1]);
  if (L.n[1][0]) sc_axis_table(H / 2, h / 2, t + L.at[1][0]);
  if (L.n[1][1]) sc_axis_table(W / 2, w / 2, t + L.at[1][1]);
}

__host__ __device__ inline int sc_i1(int i0, int n_src) { return i0 + 1 < n_src ? i0 + 1 : n_src - 1; }

// The sample: the largest sum is 255 * 2^22 + 2^21 < 2^31
__host__ __device__ inline int sc_sample(int p00, int p01, int p10, int p11, int ax, int ay) {
  return ((p00 * (SC_ONE - ax) + p01 * ax) * (SC_ONE - ay) + (p10 * (SC_ONE - ax) + p11 * ax) * ay + (1 << 21)) >> 22;
}

// Channel c of pixel (tx, ty) of a plane of `C` interleaved channels: r0 and r1 are the plane's rows ty.i0 and i1(ty.i0), x1 = i1(tx.i0)
__host__ __device__ inline int sc_sample_at(const uint8_t* r0, const uint8_t* r1, int C, int c, int x0, int x1, int ax, int ay) {
  return sc_sample(r0[x0 * C + c], r0[x1 * C + c], r1[x0 * C + c], r1[x1 * C + c], ax, ay);
}

// The planes of a frame as the scale kernel walks them: RGB24 one plane of 3 channels; NV12 luma + one plane of 2 (U, V interleaved);
// I420 luma + U + V.  Offsets in bytes from the frame's start; a row of a plane is n * C bytes, rows follow each other directly.
struct ScPlaneGeom {
  size_t src_off, dst_off;
  int src_rows, src_n, dst_rows, dst_n, C, chroma;    // n: pixels per row; chroma: the plane uses the chroma table pair
};

inline int sc_planes(int H, int W, int h, int w, int pix_fmt, ScPlaneGeom* p) {
  if (pix_fmt == VBT_PIX_RGB24) {
    p[0] = ScPlaneGeom{0, 0, H, W, h, w, 3, 0};
    return 1;
  }
  p[0] = ScPlaneGeom{0, 0, H, W, h, w, 1, 0};
  const size_t S = (size_t)H * W, D = (size_t)h * w;
  if (pix_fmt == VBT_PIX_NV12) {
    p[1] = ScPlaneGeom{S, D, H / 2, W / 2, h / 2, w / 2, 2, 1};
    return 2;
  }
  p[1] = ScPlaneGeom{S, D, H / 2, W / 2, h / 2, w / 2, 1, 1};
  p[2] = ScPlaneGeom{S + S / 4, D + D / 4, H / 2, W / 2, h / 2, w / 2, 1, 1};
  return 3;
}

inline size_t sc_frame_bytes(int H, int W, int pix_fmt) { return pix_fmt == VBT_PIX_RGB24 ? (size_t)H * W * 3 : (size_t)H * W * 3 / 2; }

// One frame on the host: what vbt_scaler_run computes, a byte at a time.  ty / tx: the luma (or RGB) pair, cty / ctx: the chroma pair.
inline void sc_scale_frame_host(const uint8_t* src, uint8_t* dst, int H, int W, int h, int w, int pix_fmt, const ScTap* ty, const ScTap* tx,
                                const ScTap* cty, const ScTap* ctx) {
  ScPlaneGeom P[3];
  const int np = sc_planes(H, W, h, w, pix_fmt, P);
  for (int k = 0; k < np; k++) {
    const ScPlaneGeom& g = P[k];
    const ScTap* py = g.chroma ? cty : ty;
    const ScTap* px = g.chroma ? ctx : tx;
    const size_t srow = (size_t)g.src_n * g.C, drow = (size_t)g.dst_n * g.C;
    for (int y = 0; y < g.dst_rows; y++) {
      const uint8_t* r0 = src + g.src_off + (size_t)py[y].i0 * srow;
      const uint8_t* r1 = src + g.src_off + (size_t)sc_i1(py[y].i0, g.src_rows) * srow;
      for (int x = 0; x < g.dst_n; x++)
        for (int c = 0; c < g.C; c++)
          dst[g.dst_off + (size_t)y * drow + (size_t)x * g.C + c] =
              (uint8_t)sc_sample_at(r0, r1, g.C, c, px[x].i0, sc_i1(px[x].i0, g.src_n), px[x].a, py[y].a);
    }
  }
}

}  // namespace vbt
