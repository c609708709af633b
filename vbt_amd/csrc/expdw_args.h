// Arguments and workgroup constants of the two whole-image expand + depthwise kernels (expdw_block.h, expdw2_block.h).  No kernel body
// lives here.
#pragma once
#include "dev_types.h"
#include "expdw2_geom.h"   // XD2_NPG, XD2S_*

namespace vbt {

// ---- first form (expdw_block.h) ----
// Waves per workgroup.  Measured end to end with three forwards in flight (A/B of two builds on one box): 16 waves 90.2 k
// frames/s, 8 waves 91.9 k (92.5 k with the chunks per workgroup re-tuned), 4 waves 86.6 k.  A 16-wave workgroup is faster alone
// (15 vs 21 us on b6) but holds every SIMD of its CU at each of its barriers; 8 waves leave issue slots to the other forwards.
#ifndef VBT_XD_WAVES
#define VBT_XD_WAVES 8
#endif
constexpr int XD_WAVES = VBT_XD_WAVES, XD_THREADS = 64 * XD_WAVES;
constexpr int XD_EST = 80;   // bytes per pixel of E and D rows (64 + 16: bank spread, 16-byte aligned)

struct ExpDwArgs {
  const int8_t* x;   // [B][H][W][Cin]
  int8_t* out;       // [B][OH][OW][Ce]: the graph's depthwise output tensor
  int H, W, Cin, OH, OW, Ce;
  int PW, PH;        // bordered E image (PH: of the tallest band)
  int t0_bytes, e_bytes;   // LDS bytes of T0 / E (sized for the tallest band)
  int pad_t, pad_l;
  int T0S;           // odd multiple of 16 bytes >= Cin
  int nchunks, cpw;  // 64-channel chunks in all / per workgroup
  int nbands, brows; // row bands per image (1: the whole image) / output rows per band: maps of more than 400 pixels (Lite1 / Lite2)
                     // do not fit LDS as a whole - a workgroup then owns `brows` output rows and expands the input rows they need
  const v4i* we;     // expand weights [chunk][ks][t][lane] x 16 B: row i of tile t = channel 64c + 16t + i, k = 64ks + 16g + j
  const int* be;     // bias with the input zero point folded, padded to 64 * nchunks
  const float* me;
  Rq rqe;
  unsigned zeb;      // zero point of the expanded tensor x4
  const long* wdc;   // depthwise [chunk][cg][lane] x 8 B: byte m = weight of tap 4m + g (0 past the kernel) for channel 64c + 16cg + (lane & 15);
                     // the MFMA operand (that byte on the diagonal of 16) is rebuilt in registers (diag_operand)
  const int* bd;     // bias with the expanded tensor's zero point folded
  const float* md;
  Rq rqd;
};

// ---- second form (expdw2_block.h) ----
struct ExpDw2Args {
  const int8_t* x;   // [B][H][W][Cin]
  int8_t* out;       // [B][OH][OW][Ce]: the graph's depthwise output tensor
  int H, W, Cin, OH, OW, Ce;
  int pad_t, pad_l;
  int nchunks, cpw;  // 64-channel chunks in all / per workgroup
  int nbands, brows; // row bands per image / output rows per band
  int XB;            // position columns per row: blocks of 4 output columns (stride 1) / of 2 (stride 2)
  int EQS, EYS;      // E: bytes per (row, quad) = 4 * padded width rounded to 16; bytes per row = 16 * EQS + bank-spreading pad
  int e_bytes;       // LDS bytes of E (tallest band, + slack for the reads past the last row)
  int PS;            // D: bytes per quad plane (4 * pixels of the tallest band, rounded so that PS / 4 = 2 mod 32)
  int pe_off;        // LDS byte offsets of the parameter areas Pe / Pd (behind D)
  int pd_off;
  // per chunk, 16-byte pieces, copied to LDS as they are:
  const v4i* pe;     // expand: weights [ks][t][lane] x 16 B (row i of tile t = channel 64 c + 16 t + i, k = 64 ks + 16 g + j) | bias (input zero
                     // point folded) x 64 | multipliers x 64                                          = KS64 * 256 + 32 pieces
  const v4i* pd;     // depthwise: [quad][mi][lane] dwords, byte j = w[2 mi + (g >> 1) - S dy][4 (g & 1) + j - S dx][64 c + 4 quad + cc] for A row
                     // (lane & 15) = 4 q + cc with q = dx (stride 1: dy = 0) or 2 dy + dx (stride 2); 0 outside the kernel; the MFMA operand
                     // (dword j = that byte at byte position cc) is rebuilt in registers | bias (expanded zero point folded) x 64 |
                     // multipliers x 64                                                                = KT2 * 256 + 32 pieces
  Rq rqe;
  unsigned zeb;      // zero point of the expanded tensor x4
  Rq rqd;
#ifdef VBT_XD_PROF
  unsigned long long* prof;
#endif
};

}  // namespace vbt
