// Fused MBConv blocks on LDS tiles with the band-Toeplitz depthwise (fused_block.h, TPZ = true): the instantiations listed by
// fused_tpz_built (launchers.h), in a translation unit of their own so that the build stays parallel.
#include "launchers.h"

namespace vbt {

#define FB_TPZ1(KK, S, NBP, KSE)   /* 8 x 8 tiles */                                                                              \
  do {                                                                                                                            \
    if (L.nt3) fused_block_kernel<KK, S, NBP, true, true, KSE, 3, 1, true, true><<<grid, 256, L.lds_bytes, st>>>(a);              \
    else fused_block_kernel<KK, S, NBP, true, true, KSE, 4, 1, true, true><<<grid, 256, L.lds_bytes, st>>>(a);                    \
    return VBT_OK;                                                                                                                \
  } while (0)
#define FB_TPZ2(KK, S, NBP, KSE)   /* 16 x 8 tiles */                                                                             \
  do {                                                                                                                            \
    if (L.nt3) fused_block_kernel<KK, S, NBP, true, true, KSE, 3, 2, true, true><<<grid, 256, L.lds_bytes, st>>>(a);              \
    else fused_block_kernel<KK, S, NBP, true, true, KSE, 4, 2, true, true><<<grid, 256, L.lds_bytes, st>>>(a);                    \
    return VBT_OK;                                                                                                                \
  } while (0)
#define FB_TPZ(KK, S, NBP, KSE) do { if (L.ppw2) FB_TPZ2(KK, S, NBP, KSE); else FB_TPZ1(KK, S, NBP, KSE); } while (0)

int launch_fused_mbconv_tpz(const FusedArgs& a, const FusedLaunch& L, hipStream_t st) {
  const dim3 grid(L.grid);
  const int k = L.k, s = L.stride, nbp = L.nbp, kse = a.KSe;
  if (L.dw64 && a.wtz && fused_tpz_built(k, s, nbp, kse, L.ppw2)) {
    if (k == 3 && s == 2 && nbp == 1 && kse == 1) FB_TPZ(3, 2, 1, 1);
    if (k == 3 && s == 1 && nbp == 1 && kse == 1) FB_TPZ(3, 1, 1, 1);
    if (k == 5 && s == 2 && nbp == 1 && kse == 1) FB_TPZ1(5, 2, 1, 1);
    if (k == 5 && s == 1 && nbp == 1 && kse == 2) FB_TPZ(5, 1, 1, 2);
  }
  set_error("fused_mbconv: no Toeplitz-depthwise instantiation for k=%d s=%d nbp=%d KSe=%d%s", k, s, nbp, kse, L.ppw2 ? " on 16 x 8 tiles" : "");
  return VBT_ERR_ARG;
}

}  // namespace vbt
