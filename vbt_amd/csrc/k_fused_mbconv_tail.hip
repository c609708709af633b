// Fused MBConv blocks on LDS tiles whose part-filled last projection block is tile-major (fused_block.h, NTL > 0): the instantiations
// listed by fused_tail_built (launchers.h), in a translation unit of their own so that the build stays parallel.
#include "launchers.h"

namespace vbt {

#define FB_TAIL1(KK, S, KSE, NTL)   /* Toeplitz depthwise, 8 x 8 tiles */                                                          \
  do {                                                                                                                            \
    if (L.nt3) fused_block_kernel<KK, S, 1, true, true, KSE, 3, 1, true, true, NTL><<<grid, 256, L.lds_bytes, st>>>(a);           \
    else fused_block_kernel<KK, S, 1, true, true, KSE, 4, 1, true, true, NTL><<<grid, 256, L.lds_bytes, st>>>(a);                 \
    return VBT_OK;                                                                                                                \
  } while (0)
#define FB_TAIL2(KK, S, KSE, NTL)   /* Toeplitz depthwise, 16 x 8 tiles */                                                         \
  do {                                                                                                                            \
    if (L.nt3) fused_block_kernel<KK, S, 1, true, true, KSE, 3, 2, true, true, NTL><<<grid, 256, L.lds_bytes, st>>>(a);           \
    else fused_block_kernel<KK, S, 1, true, true, KSE, 4, 2, true, true, NTL><<<grid, 256, L.lds_bytes, st>>>(a);                 \
    return VBT_OK;                                                                                                                \
  } while (0)
#define FB_TAIL(KK, S, KSE, NTL) do { if (L.ppw2) FB_TAIL2(KK, S, KSE, NTL); else FB_TAIL1(KK, S, KSE, NTL); } while (0)

int launch_fused_mbconv_tail(const FusedArgs& a, const FusedLaunch& L, hipStream_t st) {
  const dim3 grid(L.grid);
  const int k = L.k, s = L.stride, kse = a.KSe;
  if (fused_tail_built(L, kse, L.ntl) && (L.nt3 ? a.wpt3 : a.wpt)) {
    if (L.tpz && a.wtz) {
      if (k == 3 && s == 2 && kse == 1) FB_TAIL(3, 2, 1, 2);
      if (k == 3 && s == 1 && kse == 1) FB_TAIL(3, 1, 1, 2);
      if (k == 5 && s == 2 && kse == 1) FB_TAIL1(5, 2, 1, 3);
      if (k == 5 && s == 1 && kse == 2) FB_TAIL(5, 1, 2, 3);
    } else if (!L.tpz && L.dw64) {   // diagonal 16x16x64 depthwise, 8 x 8 tiles, 48-channel chunks, one K-step in the expand
      if (k == 3) fused_block_kernel<3, 2, 1, true, true, 1, 3, 1, true, false, 2><<<grid, 256, L.lds_bytes, st>>>(a);
      else fused_block_kernel<5, 2, 1, true, true, 1, 3, 1, true, false, 3><<<grid, 256, L.lds_bytes, st>>>(a);
      return VBT_OK;
    } else if (!L.tpz) {   // 3x3/2, two projection blocks, K <= 64, 64-channel chunks, 16x16x32 depthwise
      fused_block_kernel<3, 2, 2, true, true, 2, 4, 1, false, false, 1><<<grid, 256, L.lds_bytes, st>>>(a);
      return VBT_OK;
    }
  }
  set_error("fused_mbconv: no instantiation with %d live tiles in the last projection block for k=%d s=%d nbp=%d KSe=%d", L.ntl, k, s, L.nbp, kse);
  return VBT_ERR_ARG;
}

}  // namespace vbt
