// Tracking overlay (include/vbt_hip.h, "tracking overlay"): the per-row integers and the per-primitive walks, as host + device
// functions of (lane, lanes) so that the kernels of overlay.hip and a host loop run the same statements.
// Every walk enumerates a candidate set that contains the primitive's covered pixels inside the frame and applies the contract's
// test to each candidate; Painter::put is the only store and checks the frame's bounds itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vbt_hip.h"

namespace vbt {

struct OverlayRow {  // the 64-byte record of vbt_tracker_rows_all
  int64_t id;
  double time, x, y, dx, dy, h, w;
};

// geometry record of a row (vbt_overlay_geometry): 8 int32
enum { OV_FRAME = 0, OV_CX, OV_CY, OV_XMIN, OV_YMIN, OV_XMAX, OV_YMAX, OV_TRAIL, OV_GEOM = 8 };

__host__ __device__ inline int32_t ov_trunc(double v) {
  const double lim = 1048576.0;                       // +-2^20
  v = v < -lim ? -lim : (v > lim ? lim : v);
  return (int32_t)v;                                   // truncates toward zero
}

__host__ __device__ inline int32_t ov_frame_number(double time, double fps) {
  const double lim = 1073741824.0;                    // +-2^30
  double v = time * fps;
  v = v < -lim ? -lim : (v > lim ? lim : v);
  return (int32_t)llrint(v);
}

// g[OV_FRAME .. OV_YMAX] of one row (the trail length needs the row's neighbours: overlay_prepare_kernel)
__host__ __device__ inline void ov_row_geometry(const OverlayRow& r, double fps, int H, int W, int32_t* g) {
  g[OV_FRAME] = ov_frame_number(r.time, fps);
  g[OV_CX] = ov_trunc(r.x * W);
  g[OV_CY] = ov_trunc(r.y * H);
  g[OV_XMIN] = ov_trunc((r.x - r.w / 2) * W);
  g[OV_XMAX] = ov_trunc((r.x + r.w / 2) * W);
  g[OV_YMIN] = ov_trunc((r.y - r.h / 2) * H);
  g[OV_YMAX] = ov_trunc((r.y + r.h / 2) * H);
}

// One frame and the one colour.  All stores are plain byte stores of the same value: primitives (and workgroups) that overlap
// race on a pixel, and that is harmless by construction - whoever wins, the byte is the colour.
struct Painter {
  uint8_t* frame;
  int H, W, fmt;
  uint8_t c0, c1, c2;  // r, g, b or Y, U, V
  __host__ __device__ void put(int px, int py) const {
    if ((unsigned)px >= (unsigned)W || (unsigned)py >= (unsigned)H) return;   // covered pixels outside the frame are dropped
    if (fmt == VBT_PIX_RGB24) {
      uint8_t* p = frame + ((size_t)py * W + px) * 3;
      p[0] = c0; p[1] = c1; p[2] = c2;
      return;
    }
    frame[(size_t)py * W + px] = c0;
    uint8_t* chroma = frame + (size_t)H * W;
    if (fmt == VBT_PIX_NV12) {
      uint8_t* p = chroma + (size_t)(py >> 1) * W + (size_t)(px >> 1) * 2;
      p[0] = c1; p[1] = c2;
    } else {
      const size_t i = (size_t)(py >> 1) * (W >> 1) + (px >> 1);
      chroma[i] = c1;
      chroma[(size_t)(H >> 1) * (W >> 1) + i] = c2;
    }
  }
};

// f(px, py) for every pixel of [x0, x1] x [y0, y1] inside the frame, pixel i of the clipped rectangle going to lane i % lanes
template <class F>
__host__ __device__ inline void ov_walk_rect(const Painter& P, int x0, int x1, int y0, int y1, int lane, int lanes, F f) {
  x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0;
  x1 = x1 > P.W - 1 ? P.W - 1 : x1; y1 = y1 > P.H - 1 ? P.H - 1 : y1;
  if (x0 > x1 || y0 > y1) return;
  const unsigned w = (unsigned)(x1 - x0 + 1), total = w * (unsigned)(y1 - y0 + 1);   // <= 2^28: a frame is at most 16384 a side
  for (unsigned i = (unsigned)lane; i < total; i += (unsigned)lanes) f(x0 + (int)(i % w), y0 + (int)(i / w));
}

// rule 1
__host__ __device__ inline void ov_draw_box(const Painter& P, const int32_t* g, int t, int lane, int lanes) {
  const int a = t / 2, b = (t + 1) / 2;
  const int ox0 = g[OV_XMIN] - a, ox1 = g[OV_XMAX] + a, oy0 = g[OV_YMIN] - a, oy1 = g[OV_YMAX] + a;
  const int ix0 = g[OV_XMIN] + b, ix1 = g[OV_XMAX] - b, iy0 = g[OV_YMIN] + b, iy1 = g[OV_YMAX] - b;
  const bool hollow = ix0 <= ix1 && iy0 <= iy1;
  auto test = [&](int px, int py) {
    const bool outer = px >= ox0 && px <= ox1 && py >= oy0 && py <= oy1;
    const bool inner = hollow && px >= ix0 && px <= ix1 && py >= iy0 && py <= iy1;
    if (outer && !inner) P.put(px, py);
  };
  if (!hollow) { ov_walk_rect(P, ox0, ox1, oy0, oy1, lane, lanes, test); return; }
  ov_walk_rect(P, ox0, ox1, oy0, iy0 - 1, lane, lanes, test);       // top and bottom bands over the whole width,
  ov_walk_rect(P, ox0, ox1, iy1 + 1, oy1, lane, lanes, test);
  ov_walk_rect(P, ox0, ix0 - 1, iy0, iy1, lane, lanes, test);       // left and right bands between them
  ov_walk_rect(P, ix1 + 1, ox1, iy0, iy1, lane, lanes, test);
}

// rule 3
__host__ __device__ inline void ov_draw_marker(const Painter& P, const int32_t* g, int R, int lane, int lanes) {
  const int cx = g[OV_CX], cy = g[OV_CY];
  ov_walk_rect(P, cx - R, cx + R, cy - R, cy + R, lane, lanes, [&](int px, int py) {
    const int64_t ddx = px - cx, ddy = py - cy;
    if (ddx * ddx + ddy * ddy <= (int64_t)R * R) P.put(px, py);
  });
}

// rule 4.  Glyph g: 35 bits, bitmap row r in bits 5 (6 - r) + 4 .. 5 (6 - r), column 0 the highest of the five.
enum { OV_GLYPH_I = 10, OV_GLYPH_D = 11, OV_MAX_CHARS = 21 };   // "id" + the 19 digits of 2^63 - 1
__host__ __device__ inline uint64_t ov_glyph(int g) {
  switch (g) {
    case 0: return 0x3a33ae62eull; case 1: return 0x11842108eull; case 2: return 0x3a211111full; case 3: return 0x7c441062eull;
    case 4: return 0x08ca97c42ull; case 5: return 0x7e1e0862eull; case 6: return 0x1910f462eull; case 7: return 0x7c2222108ull;
    case 8: return 0x3a317462eull; case 9: return 0x3a317844cull; case OV_GLYPH_I: return 0x100c2108eull; default: return 0x042d9c62full;
  }
}
// the label's characters, left to right; returns their number
__host__ __device__ inline int ov_label_chars(int64_t id, uint8_t* chars) {
  uint8_t dig[20];
  int nd = 0;
  uint64_t v = id < 0 ? 0 : (uint64_t)id;
  do { dig[nd++] = (uint8_t)(v % 10); v /= 10; } while (v);
  chars[0] = OV_GLYPH_I; chars[1] = OV_GLYPH_D;
  for (int k = 0; k < nd; k++) chars[2 + k] = dig[nd - 1 - k];
  return 2 + nd;
}
__host__ __device__ inline void ov_draw_label(const Painter& P, const int32_t* g, const uint8_t* chars, int nchars, int s, int lane, int lanes) {
  const int xmin = g[OV_XMIN], ymin = g[OV_YMIN];
  const int yb = ymin - 15 > 15 ? ymin - 15 : ymin + 15, top = yb - 7 * s + 1, pitch = 6 * s;
  ov_walk_rect(P, xmin, xmin + pitch * nchars - s - 1, top, yb, lane, lanes, [&](int px, int py) {
    const int rx = px - xmin, k = rx / pitch, c = (rx - k * pitch) / s, r = (py - top) / s;
    if (c < 5 && ((ov_glyph(chars[k]) >> (5 * (6 - r) + 4 - c)) & 1)) P.put(px, py);
  });
}

// rule 2's test; the end points already clamped to [-32768, 32768]
__host__ __device__ inline bool ov_segment_covers(int px, int py, int x0, int y0, int x1, int y1, int t) {
  const int64_t dx = x1 - x0, dy = y1 - y0, qx = px - x0, qy = py - y0;
  const int64_t L2 = dx * dx + dy * dy, u = qx * dx + qy * dy, tt = (int64_t)t * t;
  if (u > 0 && u < L2) {
    const int64_t c = qx * dy - qy * dx, m = 2 * (c < 0 ? -c : c);
    return m <= 3037000499ll && m * m <= tt * L2;       // m^2 would leave int64 above that, and t^2 L2 stays below it
  }
  const int64_t ex = u <= 0 ? qx : px - x1, ey = u <= 0 ? qy : py - y1;
  return 4 * (ex * ex + ey * ey) <= tt;
}

__host__ __device__ inline int ov_clamp_point(int v) { return v < -32768 ? -32768 : (v > 32768 ? 32768 : v); }

// Rule 2 for one segment.  A covered pixel lies within t/2 of a point S of the segment.  Along the segment's major axis (m; n is the
// other one, |dn/dm| <= 1) S is at most t/2 from the pixel's own m clamped onto the segment, so S's n is within t/2 of the
// segment's n there and the pixel's n within t of it: the candidates are, for every m from both end points widened by (t+1)/2,
// the 2t + 3 values of n around the segment (one more each side than that bound, for the floor of the double product).
// The walk is therefore proportional to the segment's length, not to the area of its bounding box.
__host__ __device__ inline void ov_draw_segment(const Painter& P, int x0, int y0, int x1, int y1, int t, int lane, int lanes) {
  x0 = ov_clamp_point(x0); y0 = ov_clamp_point(y0); x1 = ov_clamp_point(x1); y1 = ov_clamp_point(y1);
  const int dx = x1 - x0, dy = y1 - y0, a = (t + 1) / 2;
  const bool xmajor = (dx < 0 ? -dx : dx) >= (dy < 0 ? -dy : dy);
  const int m0 = xmajor ? x0 : y0, m1 = xmajor ? x1 : y1, n0 = xmajor ? y0 : x0, n1 = xmajor ? y1 : x1;
  const int Wm = xmajor ? P.W : P.H, Wn = xmajor ? P.H : P.W;
  const int mlo = m0 < m1 ? m0 : m1, mhi = m0 < m1 ? m1 : m0, nlo = n0 < n1 ? n0 : n1, nhi = n0 < n1 ? n1 : n0;
  if (nhi + a < 0 || nlo - a > Wn - 1) return;          // the segment's widened bounding box misses the frame
  const int M0 = mlo - a < 0 ? 0 : mlo - a, M1 = mhi + a > Wm - 1 ? Wm - 1 : mhi + a;
  if (M0 > M1) return;
  const double slope = m1 != m0 ? (double)(n1 - n0) / (double)(m1 - m0) : 0.0;
  const int span = 2 * t + 3;
  for (int m = M0 + lane; m <= M1; m += lanes) {
    const int mc = m < mlo ? mlo : (m > mhi ? mhi : m);
    const int nc = n0 + (int)floor((double)(mc - m0) * slope);
    for (int j = 0; j < span; j++) {
      const int n = nc - t - 1 + j;
      const int px = xmajor ? m : n, py = xmajor ? n : m;
      if ((unsigned)n < (unsigned)Wn && ov_segment_covers(px, py, x0, y0, x1, y1, t)) P.put(px, py);
    }
  }
}

}  // namespace vbt
