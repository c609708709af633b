// Whole-image expand + depthwise of the low-resolution MBConv blocks, both forms of the kernel (expdw_block.h, expdw2_block.h).
#include "launchers.h"
#include "expdw_block.h"
#include "expdw2_block.h"

namespace vbt {

int launch_expdw(const ExpDwArgs& a, int k, int stride, int KS64, unsigned grid_x, int lds_bytes, hipStream_t st) {
  const dim3 grid(grid_x);
#define XD_LAUNCH(KK, S)                                                                                             \
  do {                                                                                                               \
    VBT_LDS_OPT_IN(expdw_image_kernel<KK, S, 2>);                                                                    \
    VBT_LDS_OPT_IN(expdw_image_kernel<KK, S, 3>);                                                                    \
    VBT_LDS_OPT_IN(expdw_image_kernel<KK, S, 4>);                                                                    \
    if (KS64 == 2) expdw_image_kernel<KK, S, 2><<<grid, XD_THREADS, lds_bytes, st>>>(a);                             \
    else if (KS64 == 3) expdw_image_kernel<KK, S, 3><<<grid, XD_THREADS, lds_bytes, st>>>(a);                        \
    else expdw_image_kernel<KK, S, 4><<<grid, XD_THREADS, lds_bytes, st>>>(a);                                       \
  } while (0)
  if (k == 3 && stride == 1) XD_LAUNCH(3, 1);
  else if (k == 5 && stride == 1) XD_LAUNCH(5, 1);
  else XD_LAUNCH(5, 2);
#undef XD_LAUNCH
  return VBT_OK;
}

template <int KK, int S, int KS64, int NW, int GPW, int NPGB = XD2_NPG>
static int launch_expdw2_t(const ExpDw2Args& a, unsigned grid, int lds_bytes, hipStream_t st) {
  VBT_LDS_OPT_IN(expdw2_kernel<KK, S, KS64, NW, GPW, NPGB>);
  expdw2_kernel<KK, S, KS64, NW, GPW, NPGB><<<dim3(grid), 64 * NW, lds_bytes, st>>>(a);
  return VBT_OK;
}

// the small-map instantiation (expdw2_geom.h: expdw2_small_ok): stride 1, XD2S_WAVES waves, XD2S_GPW pixel groups per wave
static int launch_expdw2_small(const ExpDw2Args& a, int k, int KS64, unsigned grid, int lds_bytes, hipStream_t st) {
#define XD2S(KK, KS) launch_expdw2_t<KK, 1, KS, XD2S_WAVES, XD2S_GPW, XD2S_NPG>(a, grid, lds_bytes, st)
  if (k == 3) return KS64 == 2 ? XD2S(3, 2) : KS64 == 3 ? XD2S(3, 3) : XD2S(3, 4);
  return KS64 == 2 ? XD2S(5, 2) : KS64 == 3 ? XD2S(5, 3) : XD2S(5, 4);
#undef XD2S
}

int launch_expdw2(const ExpDw2Args& a, int k, int stride, int KS64, int nw, int gpw, bool small, unsigned grid, int lds_bytes, hipStream_t st) {
#define XD2_GPW(KK, KS)                                                                    \
  do {                                                                                     \
    if (stride == 2) {   /* 16 waves only */                                               \
      if (gpw == 1) { if (launch_expdw2_t<KK, 2, KS, 16, 1>(a, grid, lds_bytes, st)) return VBT_ERR_HIP; }             \
      else if (gpw == 2) { if (launch_expdw2_t<KK, 2, KS, 16, 2>(a, grid, lds_bytes, st)) return VBT_ERR_HIP; }        \
      else { if (launch_expdw2_t<KK, 2, KS, 16, 4>(a, grid, lds_bytes, st)) return VBT_ERR_HIP; }                      \
    } else if (nw == 16) {                                                                 \
      if (gpw == 1) { if (launch_expdw2_t<KK, 1, KS, 16, 1>(a, grid, lds_bytes, st)) return VBT_ERR_HIP; }             \
      else if (gpw == 2) { if (launch_expdw2_t<KK, 1, KS, 16, 2>(a, grid, lds_bytes, st)) return VBT_ERR_HIP; }        \
      else { if (launch_expdw2_t<KK, 1, KS, 16, 4>(a, grid, lds_bytes, st)) return VBT_ERR_HIP; }                      \
    } else {                                                                               \
      if (gpw == 2) { if (launch_expdw2_t<KK, 1, KS, 8, 2>(a, grid, lds_bytes, st)) return VBT_ERR_HIP; }              \
      else if (gpw == 4) { if (launch_expdw2_t<KK, 1, KS, 8, 4>(a, grid, lds_bytes, st)) return VBT_ERR_HIP; }         \
      else { if (launch_expdw2_t<KK, 1, KS, 8, 7>(a, grid, lds_bytes, st)) return VBT_ERR_HIP; }                       \
    }                                                                                      \
  } while (0)
#define XD2_KS(KK)                  \
  do {                              \
    if (KS64 == 2) XD2_GPW(KK, 2);  \
    else if (KS64 == 3) XD2_GPW(KK, 3); \
    else XD2_GPW(KK, 4);            \
  } while (0)
  const bool gpw_ok = nw == 16 ? (gpw == 1 || gpw == 2 || gpw == 4) : (gpw == 2 || gpw == 4 || gpw == 7);
  if ((k != 3 && k != 5) || (stride != 1 && stride != 2) || (stride == 2 && nw != 16) || KS64 < 2 || KS64 > 4 || (nw != 8 && nw != 16) || !gpw_ok) {
    set_error("expdw2: no kernel for k %d, stride %d, %d K steps, %d waves, %d groups per wave", k, stride, KS64, nw, gpw);
    return VBT_ERR_ARG;
  }
  if (small) {
    if (stride != 1 || nw != XD2S_WAVES || gpw != XD2S_GPW) { set_error("expdw2: the small-map form is stride 1, %d waves, %d groups per wave", XD2S_WAVES, XD2S_GPW); return VBT_ERR_ARG; }
    return launch_expdw2_small(a, k, KS64, grid, lds_bytes, st);
  }
  if (k == 3) XD2_KS(3);
  else XD2_KS(5);
#undef XD2_KS
#undef XD2_GPW
  return VBT_OK;
}

}  // namespace vbt
