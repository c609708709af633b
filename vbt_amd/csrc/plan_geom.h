// Tile and LDS geometry the planner (planner.hip: what a step is built for) and the variant resolvers (detector.hip: what a launch needs)
// both ask.  Pure host functions of the kernels' argument structs; each has its one definition here.
#pragma once
#include <algorithm>

#include "launchers.h"   // FusedArgs, BandArgs, FB_* / BD_* tile constants (argument headers only)

namespace vbt {

// tile of the fused MBConv / SeparableConv kernels (fused_block.h) and of the stand-alone depthwise on LDS tiles: the cheapest cut
inline void choose_tile(int OH, int OW, int KK, int S, bool expand, int* TXo, int* TYo, int slots = 64) {
  double best = 1e300;
  for (int TX = 1; TX <= std::min(OW, 64); TX++) {
    int TXp = (TX + 3) & ~3;
    int TY = std::min(OH, slots / TXp);
    if (TY < 1) continue;
    int tiles = ((OW + TX - 1) / TX) * ((OH + TY - 1) / TY);
    int NPh = ((TXp - 1) * S + KK) * ((TY - 1) * S + KK);
    // halo pixels cost expand work + LDS loads; every tile also pays the 64-slot depthwise/project work
    double cost = tiles * ((expand ? 1.0 : 0.35) * NPh + (double)slots);
    if (cost < best) { best = cost; *TXo = TX; *TYo = TY; }
  }
}

// LDS bytes of one fused tile (fused_block.h): the input halo of a TX x TY tile (T0S bytes per pixel), the expanded halo (est bytes per
// pixel; 0: no expand stage), the depthwise output of 64 * ppw pixels and, for a single-chunk SeparableConv / node, the projection
// weights + bias / multipliers staged in LDS.  (Rounding the E rows up to 16 bytes changes only the 72-byte rows: FB_EST and 48 are
// multiples of 16.)
// e_bytes >= 0: the expanded halo takes that many bytes instead (the quad-planar E of the Toeplitz depthwise: tpz_geom).
inline int fused_tile_lds(const FusedArgs& a, int k, int stride, int TX, int TY, int est, int ppw, int nbp, int e_bytes = -1) {
  const int TXp = (TX + 3) & ~3;
  const int NPh = ((TXp - 1) * stride + k) * ((TY - 1) * stride + k);
  int lds = ((NPh * a.T0S + 15) & ~15) + (e_bytes >= 0 ? e_bytes : ((NPh * est + 15) & ~15)) + ppw * 64 * FB_DST;
  if (!est && a.nchunks == 1 && nbp <= 2) lds += nbp * (4096 + 512);
  return lds;
}

// LDS bytes of one row band (band_block.h).
// chained: the form without the depthwise tile D, with the compact depthwise operands staged behind the projection panel instead
// (band_block.h; the arithmetic is band_geom.h's)
inline int band_lds(const BandArgs& a, bool chained = false) {
  return band_lds_bytes(a.rows, a.W, a.CS, a.Cout, a.KS, chained);
}

}  // namespace vbt
