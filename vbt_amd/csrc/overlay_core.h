// Tracking overlay (include/vbt_hip.h, "tracking overlay"): the per-row integers and the per-primitive walks, as host + device
// functions of (lane, lanes) so that the kernels of overlay.hip and a host loop run the same statements.
// Every walk enumerates a candidate set that contains the primitive's covered pixels inside the frame and applies the contract's
// test to each candidate; Painter::put is the only store and checks the frame's bounds itself.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else   // a host compiler (tests/fuzz/overlay_follow_check.cc): the same statements, no HIP header needed
#include <math.h>
#include <stddef.h>
#define __host__
#define __device__
#endif

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

// ---- following a device row log (include/vbt_hip.h, "Following a device row log") ----
// Per log row: its geometry record and a link record; per frame number: the newest accepted row of the frame and their count (the
// frame's rows hang on OV_LINK_FNEXT, so they need not be neighbours in the log); per id: the newest accepted row (OvIdSlot, open
// addressing).  OV_TRAIL = 0 marks a skipped row.
enum { OV_LINK_PREV = 0, OV_LINK_SKIP, OV_LINK_DEPTH, OV_LINK_FNEXT, OV_LINK = 4 };   // previous row of the id, its 16th ancestor, rows of the id so far, next row of the frame
enum { OV_SKIP_HOPS = 16 };
enum { OV_STATE_CURSOR = 0, OV_STATE_FLAGS = 1, OV_STATE = 4 };

struct OvIdSlot {
  int64_t id;      // -1: free
  int32_t last;    // log index of the id's newest accepted row, -1: none yet
  int32_t pad;
};

struct OvFollow {
  const OverlayRow* rows;   // the followed log (borrowed)
  int32_t* geom;            // [rows_cap][OV_GEOM]
  int32_t* link;            // [rows_cap][OV_LINK]
  int32_t* findex;          // [max_frame + 1][2]: newest accepted row, accepted rows
  OvIdSlot* table;          // [table_mask + 1], a power of two >= 2 rows_cap: it never fills
  int32_t* state;           // [OV_STATE]
  double fps;
  int rows_cap, max_frame, max_rows_per_frame, table_mask, H, W, trail;
};

__host__ __device__ inline bool ov_finite(double v) { return __builtin_isfinite(v); }

// What a row shows on its own: g[OV_FRAME .. OV_YMAX] (zeros for a row set_rows would refuse: its doubles have no integers) and 0,
// VBT_OVERLAY_FOLLOW_BAD_ROW or _FRAME_RANGE
__host__ __device__ inline int ov_follow_static(const OverlayRow& r, double fps, int H, int W, int max_frame, int32_t* g) {
  for (int k = 0; k < OV_GEOM; k++) g[k] = 0;
  const bool fin = ov_finite(r.time) && ov_finite(r.x) && ov_finite(r.y) && ov_finite(r.dx) && ov_finite(r.dy) && ov_finite(r.h) && ov_finite(r.w);
  if (!fin || r.id < 0 || r.w < 0 || r.h < 0) return VBT_OVERLAY_FOLLOW_BAD_ROW;
  ov_row_geometry(r, fps, H, W, g);
  return g[OV_FRAME] < 1 || g[OV_FRAME] > max_frame ? VBT_OVERLAY_FOLLOW_FRAME_RANGE : 0;
}

// slot of `id`, taking a free one for it if `insert`; -1: not there (or, never, a full table)
__host__ __device__ inline int ov_follow_find(OvIdSlot* table, int mask, int64_t id, bool insert) {
  unsigned h = (unsigned)(((uint64_t)id * 0x9E3779B97F4A7C15ull) >> 32) & (unsigned)mask;
  for (int probe = 0; probe <= mask; probe++, h = (h + 1) & (unsigned)mask) {
    if (table[h].id == id) return (int)h;
    if (table[h].id < 0) {
      if (!insert) return -1;
      table[h].last = -1;
      table[h].id = id;
      return (int)h;
    }
  }
  return -1;
}

// 16th ancestor of a row with `depth` rows of its id up to itself, whose previous one is `prev`; the links of all older rows are final
__host__ __device__ inline int ov_follow_skip(const int32_t* link, int prev, int depth) {
  if (depth <= OV_SKIP_HOPS) return -1;
  int a = prev;
  for (int k = 1; k < OV_SKIP_HOPS && a >= 0; k++) a = link[(size_t)a * OV_LINK + OV_LINK_PREV];
  return a;
}

__host__ __device__ inline void ov_follow_store(const OvFollow& F, int i, const int32_t* g, int prev, int skip, int depth, int fnext) {
  for (int k = 0; k < OV_GEOM; k++) F.geom[(size_t)i * OV_GEOM + k] = g[k];
  int32_t* l = F.link + (size_t)i * OV_LINK;
  l[OV_LINK_PREV] = prev; l[OV_LINK_SKIP] = skip; l[OV_LINK_DEPTH] = depth; l[OV_LINK_FNEXT] = fnext;
}

// The step of log row i, every earlier row done: accept or skip, geometry, links, frame index, id table.  Returns the row's flag (0:
// accepted).  The follow kernel takes 64 rows at a time through the same statements and falls back on this one where a row's fate
// depends on another row of its group; a host loop over it is the statement of follow mode.
__host__ __device__ inline int ov_follow_row(const OvFollow& F, int i) {
  const OverlayRow r = F.rows[i];
  int32_t g[OV_GEOM];
  int flag = ov_follow_static(r, F.fps, F.H, F.W, F.max_frame, g);
  int slot = -1, prev = -1, cnt = 0;
  if (!flag) {
    slot = ov_follow_find(F.table, F.table_mask, r.id, true);
    if (slot < 0) flag = VBT_OVERLAY_FOLLOW_BAD_ROW;
  }
  if (!flag) {
    prev = F.table[slot].last;
    cnt = F.findex[2 * (size_t)g[OV_FRAME] + 1];
    if (prev >= 0 && r.time < F.rows[prev].time) flag = VBT_OVERLAY_FOLLOW_ORDER;
    else if (cnt >= F.max_rows_per_frame) flag = VBT_OVERLAY_FOLLOW_FRAME_FULL;
  }
  if (flag) {
    ov_follow_store(F, i, g, -1, -1, 0, -1);
    return flag;
  }
  const int depth = prev >= 0 ? F.link[(size_t)prev * OV_LINK + OV_LINK_DEPTH] + 1 : 1;
  g[OV_TRAIL] = depth < F.trail ? depth : F.trail;
  int32_t* fi = F.findex + 2 * (size_t)g[OV_FRAME];
  ov_follow_store(F, i, g, prev, ov_follow_skip(F.link, prev, depth), depth, cnt > 0 ? fi[0] : -1);
  fi[0] = i; fi[1] = cnt + 1;
  F.table[slot].last = i;
  return 0;
}

// The trail segment `seg` (0 = the newest) of `row`, seg < g[OV_TRAIL] - 1: end point rows (older, newer), by seg / 16 skip links and
// seg % 16 previous-row links.  A link that is not there (-1; never, for a segment of the row's trail) ends the walk: *older = -1.
__host__ __device__ inline void ov_follow_segment(const int32_t* link, int row, int seg, int* older, int* newer) {
  int a = row;
  for (int k = 0; k < seg / OV_SKIP_HOPS && a >= 0; k++) a = link[(size_t)a * OV_LINK + OV_LINK_SKIP];
  for (int k = 0; k < seg % OV_SKIP_HOPS && a >= 0; k++) a = link[(size_t)a * OV_LINK + OV_LINK_PREV];
  *newer = a;
  *older = a >= 0 ? link[(size_t)a * OV_LINK + OV_LINK_PREV] : -1;
}

// row number `slot` (0 = the newest) of a frame with more than `slot` accepted rows (-1 if the list ends before it: never)
__host__ __device__ inline int ov_follow_frame_row(const int32_t* findex, const int32_t* link, int64_t f, int slot) {
  int row = findex[2 * (size_t)f];
  for (int k = 0; k < slot && row >= 0; k++) row = link[(size_t)row * OV_LINK + OV_LINK_FNEXT];
  return row;
}

// ---- rep panel (include/vbt_hip.h, "Rep panel"): a gather - every pixel of the panel rectangle is tested and written once ----

// record of a phase (vbt_overlay_hud_table): 6 int32; OV_HUD_COUNT = the concentric phases among phases 0 .. this one
enum { OV_HUD_FS = 0, OV_HUD_FE, OV_HUD_ROM, OV_HUD_ACV, OV_HUD_TYPE, OV_HUD_COUNT, OV_HUD_REC = 6 };
enum { OV_HUD_CELLS_X = 52, OV_HUD_CELLS_Y = 50, OV_HUD_LINE = 8, OV_HUD_CHARS = 24, OV_HUD_BARS = 8, OV_HUD_SPAN = 47, OV_HUD_BAR_CELLS = 12 };
enum { OV_GLYPH_R = 12, OV_GLYPH_E, OV_GLYPH_P, OV_GLYPH_O, OV_GLYPH_M, OV_GLYPH_A, OV_GLYPH_C, OV_GLYPH_V, OV_GLYPH_DOT, OV_GLYPH_SPACE };

__host__ __device__ inline uint64_t ov_hud_glyph(int g) {
  switch (g) {
    case OV_GLYPH_R: return 0x7a31f5251ull; case OV_GLYPH_E: return 0x7e10f421full; case OV_GLYPH_P: return 0x7a31f4210ull;
    case OV_GLYPH_O: return 0x3a318c62eull; case OV_GLYPH_M: return 0x4775ac631ull; case OV_GLYPH_A: return 0x3a31fc631ull;
    case OV_GLYPH_C: return 0x3a308422eull; case OV_GLYPH_V: return 0x46318c544ull; case OV_GLYPH_DOT: return 0x18cull;
    case OV_GLYPH_SPACE: return 0;
    default: return ov_glyph(g);
  }
}

// centimetres (per second) of a ROM / ACV in metres: the panel's own rounding
__host__ __device__ inline int32_t ov_centi(double v) {
  if (!(v > 0)) return 0;                              // NaN too
  const double c = v * 100.0;
  return (int32_t)llrint(c < 9999.0 ? c : 9999.0);
}

// The record of one phase (time_start, time_end, y_start, y_end, rom, type), for vbt_overlay_set_hud on the host and for
// overlay_hud_follow_kernel on the device: both tables come from these statements.  IEEE double without contraction: one multiply
// before llrint (ov_frame_number, ov_centi), one divide.
enum { OV_MAX_FRAME = 1 << 24 };                                  // the frame index is dense: 64 MB at most
enum { OV_HUD_PHASE_OK = 0, OV_HUD_PHASE_NONFINITE, OV_HUD_PHASE_TYPE, OV_HUD_PHASE_ENDS_BEFORE, OV_HUD_PHASE_ORDER, OV_HUD_PHASE_FRAME };

// What vbt_overlay_set_hud refuses a phase for on its doubles, the first that holds in its order of tests; prev = the phase before
// it in the table (NULL: it is the first)
__host__ __device__ inline int ov_hud_phase_check(const double* r, const double* prev) {
  for (int k = 0; k < 6; k++)
    if (!ov_finite(r[k])) return OV_HUD_PHASE_NONFINITE;
  if (r[5] != 0.0 && r[5] != 1.0 && r[5] != 2.0) return OV_HUD_PHASE_TYPE;
  if (r[1] < r[0]) return OV_HUD_PHASE_ENDS_BEFORE;
  if (prev && (r[0] < prev[0] || r[1] < prev[1])) return OV_HUD_PHASE_ORDER;
  return OV_HUD_PHASE_OK;
}

// t[OV_HUD_FS .. OV_HUD_TYPE] of a phase that passed ov_hud_phase_check (its doubles are finite: every cast is defined); returns
// OV_HUD_PHASE_FRAME when it ends above frame 2^24.  t[OV_HUD_COUNT] is the caller's: it needs the phases before this one.
__host__ __device__ inline int ov_hud_phase_record(const double* r, double fps, int32_t* t) {
  t[OV_HUD_FS] = ov_frame_number(r[0], fps);
  t[OV_HUD_FE] = ov_frame_number(r[1], fps);
  if (t[OV_HUD_FE] > OV_MAX_FRAME) return OV_HUD_PHASE_FRAME;
  const double dur = r[1] - r[0];
  t[OV_HUD_ROM] = ov_centi(r[4]);
  t[OV_HUD_ACV] = dur > 0 ? ov_centi(r[4] / dur) : 0;
  t[OV_HUD_TYPE] = (int32_t)r[5];
  return OV_HUD_PHASE_OK;
}

// The panel's table from a phase list no longer than `cap`, in table order: the STATEMENT of what overlay_hud_follow_kernel forms 64
// phases at a time.  Returns the number of records (0 with a flag) and ORs VBT_OVERLAY_HUD_FOLLOW_BAD_PHASE / _CAPACITY into *flags.
// The library itself does not call it: the kernel restates this loop with ballots (the running count as a prefix sum over the lanes,
// carried from stride to stride), so the host program that runs this under sanitizers (tests/fuzz/overlay_hud_follow_check.cc)
// proves ov_hud_phase_check / ov_hud_phase_record and this loop, not the kernel's carry - that is the GPU tests'
// (tests/test_gpu_overlay_hud_live.py, with a leader of more than 128 phases for the strides).
__host__ __device__ inline int ov_hud_follow_table(const double* ph, int n, int cap, double fps, int32_t* tab, int* flags) {
  if (n > cap) { *flags |= VBT_OVERLAY_HUD_FOLLOW_CAPACITY; return 0; }
  int count = 0;
  for (int i = 0; i < n; i++) {
    const double* r = ph + (size_t)i * 6;
    int32_t* t = tab + (size_t)i * OV_HUD_REC;
    if (ov_hud_phase_check(r, i > 0 ? r - 6 : nullptr) || ov_hud_phase_record(r, fps, t)) { *flags |= VBT_OVERLAY_HUD_FOLLOW_BAD_PHASE; return 0; }
    count += t[OV_HUD_TYPE] == 0;
    t[OV_HUD_COUNT] = count;
  }
  return n;
}

// state of a panel that follows the live analysis (vbt_overlay_hud_follow): phases in the table, sticky flags, the leader (int64)
enum { OV_HUD_STATE_P = 0, OV_HUD_STATE_FLAGS = 1, OV_HUD_STATE_LEADER = 2, OV_HUD_STATE = 4 };

// first i of [lo, hi) with tab[i][col] >= v, hi if there is none; the column does not decrease along the table
__host__ __device__ inline int ov_hud_lower_bound(const int32_t* tab, int lo, int hi, int col, int64_t v) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)tab[(size_t)mid * OV_HUD_REC + col] >= v) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// n of frame f: the concentric phases with fe <= f
__host__ __device__ inline int ov_hud_completed(const int32_t* tab, int P, int64_t f) {
  const int ub = ov_hud_lower_bound(tab, 0, P, OV_HUD_FE, f + 1);
  return ub > 0 ? tab[(size_t)(ub - 1) * OV_HUD_REC + OV_HUD_COUNT] : 0;
}
// table index of completed rep number m (0-based, m < n): the first phase whose running count reaches m + 1
__host__ __device__ inline int ov_hud_rep(const int32_t* tab, int P, int m) { return ov_hud_lower_bound(tab, 0, P, OV_HUD_COUNT, (int64_t)m + 1); }

// v (< 100000) in decimal, right-aligned in 5
__host__ __device__ inline void ov_hud_number(int v, uint8_t* out) {
  for (int k = 4; k >= 0; k--) {
    out[k] = (uint8_t)(k == 4 || v ? v % 10 : OV_GLYPH_SPACE);
    v /= 10;
  }
}
// field(v) of the contract, v <= 9999
__host__ __device__ inline void ov_hud_field(int n, int v, uint8_t* out) {
  if (n == 0) { for (int k = 0; k < 5; k++) out[k] = OV_GLYPH_SPACE; return; }
  const int w = v / 100;
  out[0] = (uint8_t)(w >= 10 ? w / 10 % 10 : OV_GLYPH_SPACE); out[1] = (uint8_t)(w % 10); out[2] = OV_GLYPH_DOT;
  out[3] = (uint8_t)(v / 10 % 10); out[4] = (uint8_t)(v % 10);
}
__host__ __device__ inline int ov_hud_bar_height(int acv_cm, int s, int full_scale_cm) {
  const int64_t top = (int64_t)OV_HUD_BAR_CELLS * s, hb = (int64_t)acv_cm * top / full_scale_cm;
  return (int)(hb < 1 ? 1 : (hb > top ? top : hb));
}

// What every pixel of a frame's panel needs, formed once per frame (per workgroup, in LDS)
struct OvHudState {
  int32_t n;
  int32_t hb[OV_HUD_BARS];           // 0: the slot is empty
  int32_t lo, hi;                    // the phases the timeline's columns can meet are [lo, hi)
  uint8_t chars[OV_HUD_CHARS];
};
// The state in OV_HUD_PARTS independent parts, one per lane (or per turn of a host loop): 0 = n and the text, 1 + j = bar j, 9 = [lo, hi)
enum { OV_HUD_PARTS = 2 + OV_HUD_BARS };
__host__ __device__ inline void ov_hud_state_part(const int32_t* tab, int P, int64_t f, int frame_step, int s, int full_scale_cm, int part, OvHudState& st) {
  if (part == OV_HUD_PARTS - 1) {
    int64_t first = f - (int64_t)(OV_HUD_SPAN * s - 1) * frame_step;              // the frame of column 0
    first = first < 1 ? 1 : first;
    const int lo = ov_hud_lower_bound(tab, 0, P, OV_HUD_FE, first), last = ov_hud_lower_bound(tab, 0, P, OV_HUD_FE, f);
    st.hi = last < P ? last + 1 : P;                                              // the phase that holds frame f itself is the last candidate
    st.lo = lo < st.hi ? lo : st.hi;
    return;
  }
  const int n = ov_hud_completed(tab, P, f);
  if (part == 0) {
    int rom = 0, acv = 0;
    if (n > 0) {
      const int32_t* r = tab + (size_t)ov_hud_rep(tab, P, n - 1) * OV_HUD_REC;
      rom = r[OV_HUD_ROM]; acv = r[OV_HUD_ACV];
    }
    st.n = n;
    uint8_t* c = st.chars;
    c[0] = OV_GLYPH_R; c[1] = OV_GLYPH_E; c[2] = OV_GLYPH_P; ov_hud_number(n < 99999 ? n : 99999, c + 3);
    c[8] = OV_GLYPH_R; c[9] = OV_GLYPH_O; c[10] = OV_GLYPH_M; ov_hud_field(n, rom, c + 11);
    c[16] = OV_GLYPH_A; c[17] = OV_GLYPH_C; c[18] = OV_GLYPH_V; ov_hud_field(n, acv, c + 19);
    return;
  }
  const int j = part - 1, m = (n > OV_HUD_BARS ? n - OV_HUD_BARS : 0) + j;
  st.hb[j] = m < n ? ov_hud_bar_height(tab[(size_t)ov_hud_rep(tab, P, m) * OV_HUD_REC + OV_HUD_ACV], s, full_scale_cm) : 0;
}

// The contract's test for the panel pixel (rx, ry), counted from the panel's origin, of frame f
__host__ __device__ inline bool ov_hud_covers(const OvHudState& st, const int32_t* tab, int rx, int ry, int s, int64_t f, int frame_step) {
  const int ux = rx - 2 * s;
  if (ux < 0 || ux >= OV_HUD_SPAN * s) return false;                              // text, bars and timeline all span 47 cells
  if (ry < 29 * s) {                                                              // text: lines at 2 s, 11 s, 20 s, 7 cells high
    const int uy = ry - 2 * s;
    if (uy < 0 || uy >= 27 * s) return false;
    const int l = uy / (9 * s), r = (uy - l * 9 * s) / s, k = ux / (6 * s), c = (ux - k * 6 * s) / s;
    return r < 7 && c < 5 && ((ov_hud_glyph(st.chars[l * OV_HUD_LINE + k]) >> (5 * (6 - r) + 4 - c)) & 1);
  }
  if (ry < 41 * s) {                                                              // bars: bottom at 41 s, at most 12 cells high
    const int k = ux / (6 * s);
    return ux - k * 6 * s < 5 * s && ry >= 41 * s - st.hb[k];
  }
  if (ry < 43 * s || ry >= 47 * s) return false;
  const int64_t fc = f - (int64_t)(OV_HUD_SPAN * s - 1 - ux) * frame_step;
  if (fc < 1) return false;
  const int i = ov_hud_lower_bound(tab, st.lo, st.hi, OV_HUD_FE, fc);             // fs does not decrease either: no later phase can hold fc
  if (i >= st.hi || !((int64_t)tab[(size_t)i * OV_HUD_REC + OV_HUD_FS] < fc)) return false;
  const int type = tab[(size_t)i * OV_HUD_REC + OV_HUD_TYPE];
  return type == 0 || (type == 1 && ry >= 45 * s);
}

}  // namespace vbt
