// LDS geometry of the row-band SeparableConv kernels (band_block.h).  Plain C++: the kernel reads the constants at compile time, the
// planner and the variant resolver (plan_geom.h: band_lds) and the host test (tests/test_band_dw_compact_host.py) at run time.
#pragma once

constexpr int BD_WP_TAIL = 1024;          // bias (512 B) | multipliers (512 B) behind the projection weights in LDS
// chained form: the compact depthwise operands ([cg][lane] x 4 B, weight_pack.h: pack_band_dw_compact) | bias (256 B) | multipliers
// (256 B) behind that.  (Until the operands were rebuilt in registers this was twelve 1 KB operands: 12.5 KB.)
constexpr int BD_WD_COMPACT = 4 * 64 * 4;
constexpr int BD_WD_CHAIN = BD_WD_COMPACT + 512;

// LDS bytes of one row band of `rows` rows of a W-pixel-wide map: T0 (the band with its 1-pixel border, CS bytes per pixel), then
//   two-stage form: D (the depthwise output, 16-padded pixels) | the projection panel (NT x KS KB) and its tail
//   chained form:   the projection panel and its tail | the depthwise area (BD_WD_CHAIN)
constexpr int band_lds_bytes(int rows, int W, int CS, int Cout, int KS, bool chained) {
  const int NT = (Cout + 15) / 16;
  const int t0 = (rows + 2) * (W + 2) * CS, wp = NT * KS * 1024 + BD_WP_TAIL;
  return chained ? t0 + wp + BD_WD_CHAIN : t0 + (((rows * W + 15) >> 4) << 4) * CS + wp;
}
