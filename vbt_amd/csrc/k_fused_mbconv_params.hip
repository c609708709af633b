// Fused MBConv blocks on LDS tiles with the chunk parameters fetched once per workgroup and handed over through LDS (fused_block.h:
// PLDS): the instantiations listed by fused_params_built (launchers.h), with a live-tile count (NTL > 0) and block-major (NTL = 0), in a
// translation unit of their own so that the build stays parallel.
#include "launchers.h"

namespace vbt {

#define FBP(KK, S, KSE, PPW, TPZ, NTL)                                                                                  \
  do {                                                                                                                  \
    fused_block_kernel<KK, S, 1, true, true, KSE, 3, PPW, true, TPZ, NTL, true><<<grid, 256, L.lds_bytes, st>>>(a);     \
    return VBT_OK;                                                                                                      \
  } while (0)

int launch_fused_mbconv_params(const FusedArgs& a, const FusedLaunch& L, hipStream_t st) {
  const dim3 grid(L.grid);
  const int k = L.k, kse = a.KSe, ntl = L.ntl;
  if (L.params && a.cpar && fused_params_built(L, kse, ntl)) {
    if (!L.tpz) {   // diagonal 16x16x64 depthwise, stride 2, 8 x 8 tiles, one K-step in the expand
      if (k == 3 && ntl) FBP(3, 2, 1, 1, false, 2);
      if (k == 3) FBP(3, 2, 1, 1, false, 0);
      if (ntl) FBP(5, 2, 1, 1, false, 3);
      FBP(5, 2, 1, 1, false, 0);
    }
    // Toeplitz depthwise, stride 1, 16 x 8 tiles
    if (k == 3) FBP(3, 1, 1, 2, true, 2);
    if (ntl) FBP(5, 1, 2, 2, true, 3);
    FBP(5, 1, 2, 2, true, 0);
  }
  set_error("fused_mbconv: no instantiation with the chunk parameters in LDS for k=%d s=%d nbp=%d KSe=%d ntl=%d", k, L.stride, L.nbp, kse, ntl);
  return VBT_ERR_ARG;
}

}  // namespace vbt
