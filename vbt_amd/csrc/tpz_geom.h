// LDS geometry of the band-Toeplitz depthwise of the fused tile kernels (fused_block.h: TPZ).  Plain C++: the kernel reads it at compile
// time, the planner (fused_tile_lds) and the host tests at run time.
#pragma once

// Band-Toeplitz depthwise of the tile kernels (template flag TPZ; the operand of expdw2_block.h).  The expanded chunk is QUAD-PLANAR,
// E[halo row][channel quad][x][4 channels]; a position is 1 x 4 output pixels (stride 1) or 2 x 2 (stride 2) and a position group
// 16 positions = 64 output pixels: the whole 8 x 8 tile, or half of a 16 x 8 one.  One MFMA multiplies
// A[(output pixel, c)][(ty, x', c')] = w[ty][x' - S dx][c] delta(c, c') (K = 2 rows x 8 columns x 4 channels of the expanded image)
// with one aligned 16-byte read per lane: 2 / 3 instructions per 64 pixels x 4 channels at stride 1 (3x3 / 5x5), 3 / 4 at stride 2.
//   XB   positions per tile row; a position's 8 input columns start at column 4 xk, so a (row, quad) plane holds 4 XB + 4 columns
//   EQS  bytes per (row, quad) plane;  EYS  bytes per halo row = quads x EQS + the pad that spreads the b128 reads over the banks
//   rows halo rows the reads touch: the last MFMA of a position may run one or two rows past the halo (zero weights, but inside E)
//   DSK  bytes the D tile's pixel slots shift per tile row (stride 1): a lane's output dwords then spread over all the banks a
//        16-byte-aligned slot pitch can reach (4-way instead of 8-way stores)
struct TpzGeom { int XB, EQS, EYS, rows, e_bytes, DSK; };
// the lanes a ds_read_b128 serves together: four groups of 16, one LDS cycle each when conflict-free (also planner.hip: xd2_read_cycles)
constexpr int DS_READ_B128_GROUPS[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                            {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                            {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                            {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
// Position (of a group of 16) that lane r of the B operand computes.  ds_read_b128 serves lanes {0-3, 12-15} of one K slice together
// with lanes {4-11} of the next: the first set takes the even positions of the group's first half and the odd ones of its second,
// the other set the rest - a checkerboard, on which the two sets' 16-byte pieces (one column apart) never share a bank quarter.
constexpr int tpz_position(int r) { return 2 * (r & 7) + (((r >> 2) & 1) ^ (((r + 4) >> 3) & 1)); }
// LDS cycles of the stage's operand reads (ds_read_b128: four groups of 16 lanes, one cycle per group when its 16-byte pieces fall on
// distinct quarters of the 64 banks; equal addresses broadcast) over the npg position groups of a tile
constexpr int tpz_read_cycles(int S, int XB, int npg, int EYS) {
  int cycles = 0;
  for (int pg = 0; pg < npg; pg++)
    for (int k = 0; k < 4; k++) {
      int seen[16][16] = {}, ns[16] = {}, worst = 1;
      for (int j = 0; j < 16; j++) {
        const int lane = DS_READ_B128_GROUPS[k][j], g = lane >> 4, n = pg * 16 + tpz_position(lane & 15);
        const int addr = (n / XB) * S * S * EYS + (n % XB) * 16 + (g >> 1) * EYS + 16 * (g & 1), b = (addr >> 4) & 15;
        bool dup = false;
        for (int h = 0; h < ns[b]; h++) dup = dup || seen[b][h] == addr;
        if (!dup) seen[b][ns[b]++] = addr;
        if (ns[b] > worst) worst = ns[b];
      }
      cycles += worst;
    }
  return cycles;
}
constexpr TpzGeom tpz_geom(int KK, int S, int PPW, int NT) {
  TpzGeom g{};
  g.XB = 8 * PPW * S / 4;
  g.EQS = 16 * (g.XB + 1);
  const int KT2 = (S * (S - 1) + KK + 1) / 2;
  g.rows = S * S * (8 / S - 1) + 2 * KT2;
  int best = -1;
  for (int pad = 0; pad < 256; pad += 16) {
    const int cyc = tpz_read_cycles(S, g.XB, PPW, 4 * NT * g.EQS + pad);
    if (best < 0 || cyc < best) { best = cyc; g.EYS = 4 * NT * g.EQS + pad; }
  }
  g.e_bytes = g.rows * g.EYS;
  g.DSK = S == 1 ? 16 : 0;
  return g;
}

// ---- the stage's addresses, shared by the kernel (fused_block.h) and the host test that emulates it ----
// E byte offset of the operand of lane (r = lane & 15, g = lane >> 4) on position group 0: kernel rows 0 / 1 (g >> 1), column half g & 1,
// channel quad q0; quad q0 + q is q EQS further, MFMA mi 2 mi EYS, position group pg pg * tpz_e_group
constexpr int tpz_e_offset(const TpzGeom& G, int S, int r, int g, int q0) {
  const int n = tpz_position(r), y = n / G.XB, xk = n % G.XB;
  return (S * S * y + (g >> 1)) * G.EYS + 16 * xk + 16 * (g & 1) + q0 * G.EQS;
}
constexpr int tpz_e_group(const TpzGeom& G, int S) { return (16 / G.XB) * S * S * G.EYS; }
// the expand epilogue's store of halo pixel (hy, hx), channel quad q
constexpr int tpz_e_store(const TpzGeom& G, int hy, int hx, int q) { return hy * G.EYS + 4 * hx + q * G.EQS; }
// D byte offset of pixel slot `slot` (= py * TXP + px, TXP = 8 PPW; dst = bytes per slot): what the projection stage reads
constexpr int tpz_d_slot(const TpzGeom& G, int PPW, int dst, int slot) { return slot * dst + (slot / (8 * PPW)) * G.DSK; }
// D byte offset of the output dword of lane (r, g) - the 4 channels of quad q0 of output pixel g of its position - on position group 0;
// position group pg is pg * tpz_d_group further (64 slots), quad q0 + q 4 q
constexpr int tpz_d_offset(const TpzGeom& G, int S, int PPW, int dst, int r, int g, int q0) {
  const int n = tpz_position(r), y = n / G.XB, xk = n % G.XB;
  const int py = S == 1 ? y : 2 * y + (g >> 1), px = S == 1 ? 4 * xk + g : 2 * xk + (g & 1);
  return tpz_d_slot(G, PPW, dst, py * 8 * PPW + px) + 4 * q0;
}
constexpr int tpz_d_group(const TpzGeom& G, int PPW, int dst) { return 64 * dst + (64 / (8 * PPW)) * G.DSK; }
