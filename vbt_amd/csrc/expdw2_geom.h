// Geometry of the second form of the expand + depthwise kernel (expdw2_block.h): bands, the LDS layout, what a wave owns, and which steps
// may run the small-map instantiation.  Plain C++: the planner and the host tests read it at run time, the kernel takes its bounds from it.
#pragma once
#include <algorithm>
#include <vector>

#include "tpz_geom.h"   // DS_READ_B128_GROUPS

namespace vbt {

constexpr int XD2_NPG = 8;     // position groups a band may have (128 positions = 512 output pixels)
// The small-map instantiation (variant 300 + chunks per workgroup): bands of at most XD2S_NPG position groups whose input is at most
// 2 pixel groups per wave on XD2S_WAVES waves - the 10 x 10 maps.  The kernel is held to 512 / (2 * XD2S_WAVES / 4) = 128 registers, so
// that two workgroups share a CU; the planner offers it only where twice its LDS fits beside that.
constexpr int XD2S_NPG = 2, XD2S_WAVES = 8, XD2S_GPW = 2;
constexpr int XD2_CU_LDS = 160 * 1024;   // LDS of a compute unit (gfx950)

// LDS cycles of the depthwise operand reads (ds_read_b128: four groups of 16 lanes, one cycle per group when its 16-byte pieces
// fall on distinct quarters of the 64 banks; equal addresses broadcast) summed over the positions of a band, for a row stride EYS
inline long xd2_read_cycles(int PR, int XB, int EYS, int RM) {   // PR position rows, RM rows of the expanded image between them
  const int NPOS = PR * XB;
  long cycles = 0;
  for (int pg = 0; pg * 16 < NPOS; pg++)
    for (int k = 0; k < 4; k++) {
      std::vector<int> seen[16];
      int worst = 1;
      for (int j = 0; j < 16; j++) {
        const int lane = DS_READ_B128_GROUPS[k][j], r = lane & 15, g = lane >> 4, n = std::min(pg * 16 + r, NPOS - 1);   // (tpz_geom.h)
        const int addr = (n / XB) * RM * EYS + (n % XB) * 16 + (g >> 1) * EYS + 16 * (g & 1);
        std::vector<int>& v = seen[(addr >> 4) & 15];
        if (std::find(v.begin(), v.end(), addr) == v.end()) v.push_back(addr);
        worst = std::max(worst, (int)v.size());
      }
      cycles += worst;
    }
  return cycles;
}
// npg: position groups of the tallest band; small: the small-map instantiation applies (expdw2_small_ok)
struct ExpDw2Geom { bool ok; int nbands, brows, XB, EQS, EYS, e_bytes, PS, pe_off, pd_off, lds, gpw, gpw16, npg; bool small; };
// the small-map form applies: stride 1, the 8-wave form with two pixel groups per wave, at most XD2S_NPG position groups, and two
// workgroups' LDS on one CU
inline bool expdw2_small_ok(const ExpDw2Geom& g, int stride) {
  return g.ok && stride == 1 && g.gpw == XD2S_GPW && g.npg <= XD2S_NPG && 2 * g.lds <= XD2_CU_LDS;
}
inline ExpDw2Geom expdw2_geom(int H, int W, int OH, int OW, int k, int stride, int pad_t, int KS64, int nbands) {
  ExpDw2Geom g{};
  const int DY = stride, DX = 4 / stride;   // output pixels of a depthwise position: 1 x 4 (stride 1), 2 x 2 (stride 2)
  g.brows = (OH + nbands - 1) / nbands;
  if (DY == 2) g.brows = (g.brows + 1) & ~1;   // whole row pairs per band
  g.nbands = (OH + g.brows - 1) / g.brows;
  g.XB = (OW + DX - 1) / DX;
  const int KT2 = (stride * (DY - 1) + k + 1) / 2, PW = (OW - 1) * stride + k;
  g.EQS = (4 * PW + 15) & ~15;
  int in_rows = 0;
  for (int b = 0; b < g.nbands; b++) {
    const int oy0 = b * g.brows, oy1 = std::min(oy0 + g.brows, OH);
    const int lo = std::max(oy0 * stride - pad_t, 0), hi = std::min(oy0 * stride - pad_t + (oy1 - oy0 - 1) * stride + k, H);
    in_rows = std::max(in_rows, hi - lo);
  }
  const int PR = (g.brows + DY - 1) / DY;   // position rows of the tallest band
  long best = -1;
  for (int pad = 0; pad < 256; pad += 16) {
    const long cyc = xd2_read_cycles(PR, g.XB, 16 * g.EQS + pad, stride * DY);
    if (best < 0 || cyc < best) { best = cyc; g.EYS = 16 * g.EQS + pad; }
  }
  const int PHe = stride * DY * (PR - 1) + 2 * KT2;   // the last MFMA of a position may read a row past the kernel: zero weights, but the row must exist
  g.e_bytes = (PHe * g.EYS + 32 + 15) & ~15;
  int ps4 = g.brows * OW;
  while ((ps4 & 31) != 2) ps4++;
  g.PS = 4 * ps4;
  g.pe_off = g.e_bytes + 16 * g.PS;
  g.pd_off = g.pe_off + 16 * (KS64 * 256 + 32);
  g.lds = g.pd_off + 16 * (KT2 * 256 + 32);
  const int npgi = (in_rows * W + 15) / 16, need = (npgi + 3) / 4;
  g.gpw = need <= 2 ? 2 : need <= 4 ? 4 : need <= 7 ? 7 : 0;
  const int need16 = (npgi + 7) / 8;
  g.gpw16 = need16 <= 1 ? 1 : need16 <= 2 ? 2 : need16 <= 4 ? 4 : 0;
  if (g.gpw16 * KS64 > 8) g.gpw16 = 0;    // (the input operands a wave keeps: 4 registers each; beyond these the kernels spill)
  if (g.gpw * KS64 > 21) g.gpw = 0;
  if (stride == 2) g.gpw = 0;             // stride 2 exists on 16 waves only
  g.npg = (PR * g.XB + 15) / 16;
  g.ok = (g.gpw > 0 || g.gpw16 > 0) && g.lds <= 100 * 1024 && PR * g.XB <= 16 * XD2_NPG && g.e_bytes < 65536 && 16 * g.PS < 65535;   // (16-bit LDS offsets in the kernel)
  g.small = expdw2_small_ok(g, stride);
  return g;
}
inline ExpDw2Geom expdw2_choose(int H, int W, int OH, int OW, int k, int stride, int pad_t, int KS64) {
  ExpDw2Geom g{};
  for (int nb = 1; nb <= OH; nb++) {
    g = expdw2_geom(H, W, OH, OW, k, stride, pad_t, KS64, nb);
    if (g.ok) return g;
  }
  g.ok = false;
  g.small = false;
  return g;
}

}  // namespace vbt
