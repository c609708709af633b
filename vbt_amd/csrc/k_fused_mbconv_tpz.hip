// Fused MBConv blocks on LDS tiles with the band-Toeplitz depthwise (fused_block.h, TPZ = true): the instantiations of
// VBT_FUSED_TPZ_ROWS (fused_built.h), in a translation unit of their own so that the build stays parallel.
#include "launchers.h"
#include "fused_block.h"

namespace vbt {

int launch_fused_mbconv_tpz(const FusedArgs& a, const FusedLaunch& L, hipStream_t st) {
  const dim3 grid(L.grid);
  const int k = L.k, s = L.stride, nbp = L.nbp, kse = a.KSe;
  if (L.dw64 && a.wtz) {
#define FB_ROW(KK, S, NBP, KSE, NT, PPW, DW64, TPZ, NTL)                                                                   \
    if (fused_tpz_row(k, s, nbp, kse, L.ppw2, KK, S, NBP, KSE, PPW) && L.nt3 == (NT == 3)) {                               \
      fused_block_kernel<KK, S, NBP, true, true, KSE, NT, PPW, DW64, TPZ, NTL><<<grid, 256, L.lds_bytes, st>>>(a);         \
      return VBT_OK;                                                                                                       \
    }
    VBT_FUSED_TPZ_ROWS(FB_ROW)
#undef FB_ROW
  }
  set_error("fused_mbconv: no Toeplitz-depthwise instantiation for k=%d s=%d nbp=%d KSe=%d%s", k, s, nbp, kse, L.ppw2 ? " on 16 x 8 tiles" : "");
  return VBT_ERR_ARG;
}

}  // namespace vbt
