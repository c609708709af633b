// Arguments of the whole-image MBConv kernel (image_block.h) beside its FusedArgs, and the workgroup shape the resolver sizes its bundles
// by.  No kernel body lives here.
#pragma once

namespace vbt {

constexpr int IB_WAVES = 16, IB_THREADS = 64 * IB_WAVES, IB_NPF = 3;  // NPF uint4 prefetch registers per lane (48 KB bundles)

struct ImageBundle {       // byte offsets inside one chunk's record
  const unsigned char* data;
  int bytes;               // record size, multiple of 16
  int o_be, o_me, o_dw, o_bd, o_md, o_wp;
};

}  // namespace vbt
