// Arguments of the fused network entry (stem_block.h).  No kernel body lives here.
#pragma once
#include "dev_types.h"

namespace vbt {

struct StemBlockArgs {
  const uint8_t* frames;
  int8_t* out;
  int H, W, SH, SW, Cout;
  int spad_t, spad_l;   // SAME padding of the stem
  int tiles_x, tiles_y;
  unsigned in_pad4;     // out-of-image input byte (uint8 domain, zero point + 128) x 4
  const long* ws;       // stem weights [t(2)][lane] x 8 B; row i of tile t = cout 8(i>>2) + 4t + (i&3)
  const int* bs;        // [32] folded bias
  const float* ms;      // [32]
  Rq rqs;
  unsigned zs4;         // stem output zero point x 4
  const v4i* wd64;      // depthwise [cg(2)][3][lane] x 16 B (FusedArgs::wd64 layout)
  const int* bdm;
  const float* mdm;
  Rq rqd;
  const long* wp;       // project [lane] x 8 B (row i = cout i, K = 32)
  const int* bp;        // [16] folded
  const float* mp;      // [16]
  Rq rqp;
  // the direct form (stem_block_direct_kernel)
  unsigned in_pad4s;    // in_pad4 in the int8 domain (every byte XOR 0x80)
  const v4i* ws64;      // stem weights [t(2)][lane] x 16 B: lane group g < 3 = kernel row g, bytes 0..8 its nine taps, zero elsewhere
  const long* wpc;      // project [lane] x 8 B in the K order the depthwise leaves in registers (pack_stem_block_proj_chain)
};

}  // namespace vbt
