// Arguments of the fused tile kernels (fused_block.h): what launch_step fills and launch_fused_* take, and the tile constants the planner
// sizes LDS with.  No kernel body lives here.
#pragma once
#include "dev_types.h"

namespace vbt {

struct FusedArgs {
  const int8_t* x;
  int8_t* out;
  int H, W, Cin, OH, OW, Cout;
  int pad_t, pad_l;
  int TX, TY, tiles_x, tiles_y;
  int T0S;       // bytes per halo pixel row in LDS
  int nchunks;   // Ce_pad / 64
  int zx;        // zero point of the block input
  // expand (EXPAND only)
  const long* we;
  const int* be;
  const float* me;
  int KSe, ze, loe, hie;
  Rq rqe;
  // 48-channel chunking (template NT = 3) of the same block, for expanded widths that are multiples of 48 but not of 64
  // (6 x {16, 24, 40, 80, 112}): no padded channels in the expand / depthwise stages.  nch3 == 0: not available.
  const long* we3;   // [(c*KSe + ks)*3 + t][lane]: cout = 48c + 12(i>>2) + 4t + (i&3)
  const long* wdm3;  // [(c*3 + cg)*KT + m][lane]: channel 48c + 16cg + i
  const v4i* wp3;    // project weights, K-step c (16x16x64 layout) = channels 48c..48c+47 (+16 zero columns)
  int nch3, KSp3;
  // depthwise
  const float* wd;  // [k*k][Ce_pad]
  const int* bd;    // folded, padded to Ce_pad
  const float* md;
  int zd, lod, hid;
  Rq rqd;
  // depthwise on the matrix pipe (MDW): diagonal-embedded weights [chunk][cg][m][lane] x 8 B and the bias
  // folded for raw int8 inputs (bias - z_x * sum(w))
  const long* wdm;
  const int* bdm;
  // the same for the 16x16x64 MFMA (DW64): [16-channel group q][m][lane] x 16 B, lane (i = lane & 15 -> channel 16q + i,
  // g = lane >> 4): byte j is non-zero only for j == i and holds the weight of tap (m, g):
  //   3x3: (row m, column g), g = 3 is a zero column           -> 3 instructions
  //   5x5: m < 5: (row m, column g); m = 5: (row g, column 4); m = 6: g = 0 -> (4, 4), the rest zero -> 7 instructions
  // so the B operand of (m, g) sits at a compile-time offset from one of two per-lane base addresses
  const v4i* wd64;
  // the same operands as one byte each: [16-channel group q][lane] x 8 B, byte m = the non-zero byte of operand (q, m) of that
  // lane; the kernels rebuild the 16-byte operand in registers (diag_operand)
  const long* wd64c;
  // band-Toeplitz depthwise (TPZ): tap table [channel quad q][m][lane] x 4 bytes (pack_expdw2_taps over all Ce_pad / 4 quads - a
  // 64-channel chunk c starts at quad 16c, a 48-channel chunk at quad 12c); the kernel rebuilds the operands (toeplitz_operand)
  const unsigned* wtz;
  // project
  const v4i* wp;    // packed for the 16x16x64 MFMA (pack_weights64), K = Ce_pad, one K-step per 64-channel chunk
  // the same two panels (wp, wp3) with a tile-major part-filled last block (pack_weights64_tail), read by the kernels with a live-tile
  // count (template NTL > 0); nullptr: Cout % 64 == 0 or no such kernel is built for the step
  const v4i* wpt;
  const v4i* wpt3;
  const int* bp;
  const float* mp;
  int KSp, zo, lop, hip;
  Rq rqp;
  // PLDS: the per-chunk parameter block of the resolved launch (its chunking, depthwise form and panel layout: fused_params_geom.h,
  // pack_fused_chunk_params), nch records and the bias | multiplier tail; nullptr: the launch reads the arrays above
  const unsigned char* cpar;
  // residual ADD: out = ADD(project output, block input), the graph's input order (AddQ: XNNPACK qs8-vadd, detector.hip)
  int has_res;
  AddQ resq;
  // BiFPN node: the tile is the sum (+ReLU6) of two or three sources, each read through a resampling map
  // (0 identity, 1 nearest-neighbour up: src = floor(dst*in/out), 2 max-pool 3x3/2 SAME).  ADD is binary:
  //   n_src == 2: tile = ADD(src0, src1; sumq)
  //   n_src == 3: p = ADD(src0, src1; preq) - the partial sum with its own quantisation - then
  //               tile = ADD(p, src2; sumq) (chain == 1) or ADD(src2, p; sumq) (chain == 2)
  int n_src;
  const int8_t* src[3];
  int sh[3], sw[3], smode[3], spt[3], spl[3];
  int chain;
  AddQ sumq, preq;
};

constexpr int FB_EST = 80;  // E tile bytes per pixel (64 + 16: bank spread, 16-B aligned)
constexpr int FB_DST = 80;  // D tile bytes per pixel: 16-byte aligned rows (the projection reads 16 bytes per lane), 20-dword pitch: conflict-free


// Several independent problems (e.g. the same head layer on all 5 pyramid levels of both heads) in ONE grid:
// a workgroup finds its problem from the cumulative tile counts and runs the same body.
struct MultiTiles {
  int n;
  int start[13];  // start[p] = first workgroup of problem p, start[n] = grid size
};

// stand-alone depthwise conv on LDS tiles (dw_tile_kernel)
struct DwTileArgs {
  const int8_t* x;
  int8_t* out;
  const float* wf;   // [k*k][C]
  const int* bias;   // folded
  const float* mult;
  const long* wdm;   // matrix-pipe form [chunk][cg][m][lane] (MDW)
  const int* bdm;    // bias folded for raw int8 inputs, padded to 64-channel chunks
  const float* mdm;  // multipliers padded to 64-channel chunks
  int H, W, C, OH, OW, pad_t, pad_l, TX, TY, tiles_x, tiles_y, zx;
  Rq rq;
};

}  // namespace vbt
