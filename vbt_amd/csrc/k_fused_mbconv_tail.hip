// Fused MBConv blocks on LDS tiles whose part-filled last projection block is tile-major (fused_block.h, NTL > 0): the instantiations
// of VBT_FUSED_TAIL_ROWS (fused_built.h), in a translation unit of their own so that the build stays parallel.
#include "launchers.h"
#include "fused_block.h"

namespace vbt {

int launch_fused_mbconv_tail(const FusedArgs& a, const FusedLaunch& L, hipStream_t st) {
  const dim3 grid(L.grid);
  const int k = L.k, s = L.stride, kse = a.KSe;
  if ((L.nt3 ? a.wpt3 : a.wpt) && (!L.tpz || a.wtz)) {   // the tile-major panel of the chunking, the tap table of the Toeplitz form
#define FB_ROW(KK, S, NBP, KSE, NT, PPW, DW64, TPZ, NTL)                                                                   \
    if (fused_tail_row(L, kse, L.ntl, KK, S, NBP, KSE, NT, PPW, DW64, TPZ, NTL) && L.nt3 == (NT == 3)) {                   \
      fused_block_kernel<KK, S, NBP, true, true, KSE, NT, PPW, DW64, TPZ, NTL><<<grid, 256, L.lds_bytes, st>>>(a);         \
      return VBT_OK;                                                                                                       \
    }
    VBT_FUSED_TAIL_ROWS(FB_ROW)
#undef FB_ROW
  }
  set_error("fused_mbconv: no instantiation with %d live tiles in the last projection block for k=%d s=%d nbp=%d KSe=%d", L.ntl, k, s, L.nbp, kse);
  return VBT_ERR_ARG;
}

}  // namespace vbt
