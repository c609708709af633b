// Raster core: what the figure renderers (figure_core.h, curve_figure_core.h) share - the record table with its clip, the text test,
// the search on a column table and the test of four adjacent pixels against one curve segment - as host + device functions of plain
// integers and doubles, one IEEE operation per statement.  A figure names its record layout (FigRec, CfRec) and its glyph function as
// template arguments.  The kernels, the set functions' validation and the host programs of tests/fuzz run these statements.
#pragma once
#include "overlay_core.h"

#if defined(__HIPCC__)
#define VBT_RASTER_FN __host__ __device__ __forceinline__
#else
#define VBT_RASTER_FN inline
#endif

namespace vbt {

// ---- records ----
// A record is L::REC int32.  Fields 0..6 are every layout's: [x0, x1] x [y0, y1] is what of it can be seen (frame coordinates, clipped;
// empty when x0 > x1 or y0 > y1), (ox, oy) its own origin.  The layout says where value, aux, a text's length, turn and characters sit.
enum { REC_KIND = 0, REC_X0, REC_Y0, REC_X1, REC_Y1, REC_OX, REC_OY };

// rep figure: 12 int32, the text's n | rot << 8 in aux
struct FigRec {
  enum { REC = 12, CHARS = 7, VALUE = 10, AUX = 11 };
  static VBT_RASTER_FN int text_n(const int32_t* r) { return r[AUX] & 255; }
  static VBT_RASTER_FN int text_rot(const int32_t* r) { return r[AUX] >> 8; }
  static VBT_RASTER_FN void set_text(int32_t* r, int n, int rot) { r[AUX] = n | (rot << 8); }
};

// curve figure: 28 int32, the text's rot in aux and n in a field of its own
struct CfRec {
  enum { REC = 28, VALUE = 7, AUX = 8, N = 9, CHARS = 12 };
  static VBT_RASTER_FN int text_n(const int32_t* r) { return r[N]; }
  static VBT_RASTER_FN int text_rot(const int32_t* r) { return r[AUX]; }
  static VBT_RASTER_FN void set_text(int32_t* r, int n, int rot) { r[AUX] = rot; r[N] = n; }
};

struct Recs { int32_t* rec; int cap, n; };
struct Clip { int x0, y0, x1, y1; };

template <class L>
__host__ __device__ inline int32_t* rec_new(Recs& R, int kind) {
  if (R.n >= R.cap) return nullptr;                                    // (never: the capacity is sized for every record of a figure)
  int32_t* r = R.rec + (size_t)R.n * L::REC;
  for (int k = 0; k < L::REC; k++) r[k] = 0;
  r[REC_KIND] = kind;
  R.n++;
  return r;
}

// a rectangle [x0, x1] x [y0, y1] clipped to c; the record, for the caller that gives it another origin
template <class L>
__host__ __device__ inline int32_t* rec_box(Recs& R, int kind, int x0, int y0, int x1, int y1, const Clip& c, int value, int aux) {
  int32_t* r = rec_new<L>(R, kind);
  if (!r) return nullptr;
  r[REC_X0] = x0 > c.x0 ? x0 : c.x0; r[REC_Y0] = y0 > c.y0 ? y0 : c.y0;
  r[REC_X1] = x1 < c.x1 ? x1 : c.x1; r[REC_Y1] = y1 < c.y1 ? y1 : c.y1;
  r[REC_OX] = x0; r[REC_OY] = y0; r[L::VALUE] = value; r[L::AUX] = aux;
  return r;
}

// n characters of a 5 x 7 font at scale s: six columns each but the last
VBT_RASTER_FN int text_width(int n, int s) { return (6 * n - 1) * s; }

// n characters whose box has its top left corner at (ox, oy); rot: turned a quarter so that it reads bottom to top
template <class L>
__host__ __device__ inline void rec_text(Recs& R, int kind, int s, int ox, int oy, const uint8_t* chars, int n, int rot, const Clip& c, int value) {
  const int wu = text_width(n, s), hu = 7 * s;
  int32_t* r = rec_box<L>(R, kind, ox, oy, ox + (rot ? hu : wu) - 1, oy + (rot ? wu : hu) - 1, c, value, 0);
  if (!r) return;
  L::set_text(r, n, rot);
  for (int k = 0; k < n; k++) r[L::CHARS + k / 4] |= (int32_t)((uint32_t)chars[k] << (8 * (k % 4)));
}

// whether text record r covers pixel (px, py) of its visible box; Glyph gives a character's 35 bits (rows top to bottom, five bits each)
template <class L, uint64_t (*Glyph)(int)>
VBT_RASTER_FN bool text_covers(const int32_t* r, int s, int px, int py) {
  const int n = L::text_n(r), rot = L::text_rot(r);
  const int rx = px - r[REC_OX], ry = py - r[REC_OY];
  const int ux = rot ? text_width(n, s) - 1 - ry : rx, uy = rot ? rx : ry;
  const int k = ux / (6 * s), c = (ux - k * 6 * s) / s, row = uy / s;
  if (c >= 5) return false;
  const int g = (int)(((uint32_t)r[L::CHARS + k / 4] >> (8 * (k % 4))) & 255u);
  return (Glyph(g) >> (5 * (6 - row) + 4 - c)) & 1;
}

// ---- curves ----

// llrint after the clamp to +-32768; a NaN (from inf / inf only) goes to -32768
VBT_RASTER_FN int32_t fig_clamp_round(double v) {
  if (!(v >= -32768.0)) return -32768;
  if (v > 32768.0) return 32768;
  return (int32_t)llrint(v);
}

// first point i of [lo, hi) with col_i >= v, hi if none; point i has its column at pts[(i - base) * stride], and the columns do not decrease
VBT_RASTER_FN int col_lower_bound(const int32_t* pts, int stride, int base, int lo, int hi, int v) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (pts[(size_t)(mid - base) * stride] >= v) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// which of the pixels (qx0 + e, qy), e < n <= 4 (rectangle coordinates, columns outside [0, PW) never) the segment from (ca, ra) to
// (cb, rb), ca <= cb, of thickness t covers: rule 2 of the overlay.  Bit e of the result.
VBT_RASTER_FN unsigned quad_segment_mask(int qx0, int n, int qy, int PW, int ca, int ra, int cb, int rb, int t) {
  const int h = (t + 1) / 2;
  // a covered pixel lies within t / 2 of a point of the segment: outside its box widened by h nothing is covered
  if (qx0 + n - 1 < ca - h || qx0 > cb + h || qy < (ra < rb ? ra : rb) - h || qy > (ra < rb ? rb : ra) + h) return 0;
  unsigned m = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int e = 0; e < 4; e++) {
    const int qx = qx0 + e;
    if (e < n && qx >= 0 && qx < PW && ov_segment_covers(qx, qy, ca, ra, cb, rb, t)) m |= 1u << e;
  }
  return m;
}

}  // namespace vbt
