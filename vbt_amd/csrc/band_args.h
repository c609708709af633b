// Arguments and workgroup constants of the row-band SeparableConv kernels (band_block.h).  No kernel body lives here.
#pragma once
#include "dev_types.h"
#include "band_geom.h"   // BD_WP_TAIL, BD_WD_CHAIN

namespace vbt {

#ifndef VBT_BD_WAVES
#define VBT_BD_WAVES 16
#endif
constexpr int BD_WAVES = VBT_BD_WAVES, BD_THREADS = 64 * BD_WAVES;
constexpr int BD_LIT = 3;           // lane-iterations of the load stage whose global loads are in flight together (plain input)
constexpr int BD_LIT_NODE = 1;      // the same for a node's source loads (up to three 16-byte loads per iteration; registers: the head layers share this kernel)
constexpr int BD_LIT_NODE_WIDE = 3; // maps of more than 64 channels: LDS leaves at most four waves per SIMD, so 128 registers are free to use

struct BandArgs {
  const int8_t* x;   // [B][H][W][C] (plain input; unused when n_src > 0)
  int8_t* out;       // [B][H][W][Cout]
  int H, W, Cout, rows, nbands;
  int C, CS;         // input channels (% 8 == 0) / bytes per pixel row of T0 and D: odd multiple of 16 >= C
  int NCG, KS;       // 16-channel groups of the depthwise: ceil(C / 16) / projection K-steps of 64: ceil(C / 64)
  unsigned zx4;      // zero point of the depthwise input x4
  const v4i* wd;     // [cg][m][lane] x 16 B: row i = channel 16cg + i, k = 16g + j -> tap 4m + g, diagonal j == i
  const unsigned* wdc;   // chained form (C == 64, else null): [cg][lane] x 4 B, byte m = the weight of tap min(4m + g, 8) (0 past tap 8) for channel 16cg + (lane & 15)
  const int* bd;     // bias with the input zero point folded (16 NCG)
  const float* md;
  Rq rqd;
  const v4i* wp;     // [t][ks][lane] x 16 B: row i = output channel 16t + i, k = 64ks + 16g + j
  const v4i* wpc;    // chained form (C == 64, else null): [t][lane] x 16 B: row i = output channel 16t + i, byte 4cg + j = k 16cg + 4g + j
  const int* bp;     // bias with the depthwise output's zero point folded, padded to 64-channel blocks
  const float* mp;
  Rq rqp;
  // BiFPN node: see FusedArgs (fused_args.h)
  int n_src, chain;
  const int8_t* src[3];
  int sh[3], sw[3], smode[3], spt[3], spl[3];
  AddQ sumq, preq;
#ifdef VBT_BD_PROF
  unsigned long long* prof;
#endif
};

// the kernels of several problems in one grid (the head layers): waves per workgroup, pixels of a band at most
#ifndef VBT_BD_HEAD_WAVES
#define VBT_BD_HEAD_WAVES 8
#endif
#ifndef VBT_BD_HEAD_MAXPX
#define VBT_BD_HEAD_MAXPX 240
#endif
constexpr int BD_HEAD_WAVES = VBT_BD_HEAD_WAVES, BD_HEAD_MAXPX = VBT_BD_HEAD_MAXPX;
// Maps of more than 64 channels (Lite1 / Lite2): 16 waves, held to 64 registers so that two workgroups still share a CU.  With 6 or 7
// channel groups only NCG * (NW / NCG) waves work in the depthwise stage - 7 of 8, each with every pixel group of the band, against 14 of
// 16 with half of them (tools/probes/bd_probe.hip, Lite2 head layer at 56x56: 24 000 cycles per band on 8 waves, 16 300 on 16; with
// one 16-wave workgroup per CU - what an 84-register build gets - the launch was slower all the same).
constexpr int BD_HEAD_WAVES_WIDE = 16;

}  // namespace vbt
