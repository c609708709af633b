// Fused MBConv blocks on LDS tiles with the chunk parameters fetched once per workgroup and handed over through LDS (fused_block.h:
// PLDS): the instantiations of VBT_FUSED_PARAMS_ROWS (fused_built.h), with a live-tile count (NTL > 0) and block-major (NTL = 0), in a
// translation unit of their own so that the build stays parallel.
#include "launchers.h"
#include "fused_block.h"

namespace vbt {

int launch_fused_mbconv_params(const FusedArgs& a, const FusedLaunch& L, hipStream_t st) {
  const dim3 grid(L.grid);
  const int k = L.k, kse = a.KSe, ntl = L.ntl;
  if (L.params && a.cpar) {
#define FB_ROW(KK, S, NBP, KSE, NT, PPW, DW64, TPZ, NTL, WAVES)                                                            \
    if (fused_params_row(L, kse, ntl, KK, S, NBP, KSE, NT, PPW, DW64, TPZ, NTL)) {                                         \
      fused_block_kernel<KK, S, NBP, true, true, KSE, NT, PPW, DW64, TPZ, NTL, true><<<grid, 256, L.lds_bytes, st>>>(a);   \
      return VBT_OK;                                                                                                       \
    }
    VBT_FUSED_PARAMS_ROWS(FB_ROW)
#undef FB_ROW
  }
  set_error("fused_mbconv: no instantiation with the chunk parameters in LDS for k=%d s=%d nbp=%d KSe=%d ntl=%d", k, L.stride, L.nbp, kse, ntl);
  return VBT_ERR_ARG;
}

}  // namespace vbt
