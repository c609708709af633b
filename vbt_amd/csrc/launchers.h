// Host-side entry points of the kernel translation units (k_*.hip).  Each kernel family is compiled in its own translation
// unit - the template instantiations of the fused MBConv / SeparableConv tiles alone are most of the library's build time -
// and the launch logic (detector.hip) reaches the kernels only through these launchers: plain argument structs in, one launch
// enqueued on `st` out.  A launcher returns VBT_OK, VBT_ERR_ARG (no such instantiation) or VBT_ERR_HIP (an LDS opt-in refused) and
// sets the error text.
// This header and everything it includes holds argument structs, constants and host functions only: no kernel, no device helper.  A
// kernel unit includes it plus the kernel headers (*_block.h) it launches; a host unit parses no kernel.
#pragma once
#include "dev_types.h"           // v4i, Rq, AddQ, Epi: what the argument structs embed
#include "fused_args.h"          // FusedArgs, MultiTiles, DwTileArgs, FB_EST, FB_DST
#include "fused_built.h"         // FusedLaunch; fused_tpz_built, fused_tail_built, fused_params_built and the lists behind them
#include "fused_params_geom.h"   // FPF_*
#include "stem_block_args.h"     // StemBlockArgs
#include "image_block_args.h"    // ImageBundle, IB_*
#include "expdw_args.h"          // ExpDwArgs, XD_*, ExpDw2Args, XD2_NPG
#include "band_args.h"           // BandArgs, BD_*
#include "op_args.h"             // PwArgs, PwKernel, PwMulti, StemArgs, DwArgs, MapArgs, PostArgs

namespace vbt {

// the depthwise form of a launch, as fused_params_geom.h numbers them
static inline int fused_params_form(const FusedLaunch& L) { return L.tpz ? FPF_TOEPLITZ : L.dw64 ? FPF_DIAG64 : FPF_MATRIX; }
int launch_fused_block(const FusedArgs& a, const FusedLaunch& L, hipStream_t st);
int launch_fused_multi(const FusedArgs* d_args, const MultiTiles& mt, int k, int stride, int nbp, bool mdw, int lds_bytes, unsigned grid,
                       hipStream_t st);
int launch_dw_tile(const DwTileArgs& a, int k, int stride, bool mdw, dim3 grid, int lds_bytes, hipStream_t st);
// one workgroup per image (image_block.h)
int launch_mbconv_image(const FusedArgs& a, const ImageBundle& wb, int k, int stride, int maxu, int PW, int PH, int NB, int lds_bytes, int B,
                        hipStream_t st);
// SeparableConv / BiFPN node on row bands (band_block.h): one problem by value, or several problems in one grid
// chained: the chained depthwise + projection form (64-channel maps; lds_bytes is then band_lds of that form)
int launch_band_one(const BandArgs& a, bool chained, unsigned grid, int lds_bytes, hipStream_t st);
int launch_band_multi(const BandArgs* d_probs, const MultiTiles& mt, int C, bool chained, unsigned grid, int lds_bytes, hipStream_t st);   // C: channels of the maps (all problems alike)
// whole-image expand + depthwise (expdw_block.h)
int launch_expdw(const ExpDwArgs& a, int k, int stride, int KS64, unsigned grid, int lds_bytes, hipStream_t st);
// the same on the second form of the kernel (expdw2_block.h); nw = waves per workgroup (8 or 16; stride 2: 16), gpw = input pixel groups
// per wave (8 waves: 2, 4 or 7; 16 waves: 1, 2 or 4); small: the small-map instantiation (expdw2_geom.h: stride 1, 8 waves, gpw 2)
int launch_expdw2(const ExpDw2Args& a, int k, int stride, int KS64, int nw, int gpw, bool small, unsigned grid, int lds_bytes, hipStream_t st);
// network entry: stem 3x3/2 + first SeparableConv (stem_block.h)
// (direct: the second form of the kernel, plan variant 1)
int launch_stem_block(const StemBlockArgs& a, bool direct, unsigned grid, hipStream_t st);

// ---- the single-op kernels (op_args.h) ----
// pointwise conv, one of six forms (k_pointwise.hip); lds_bytes: the dynamic LDS of PW_E (its weight panel)
int launch_pw(const PwArgs& a, const PwKernel& k, dim3 grid, int lds_bytes, hipStream_t st);
// several pointwise convs in one grid; lds_bytes: the conv output + first pooled map of a problem that carries its two max pools, else 0
int launch_pw_multi(const PwMulti& pm, unsigned grid, int lds_bytes, hipStream_t st);
// stem conv 3x3/2 on the uint8 frames, 64 output pixels per workgroup (k_ops.hip, with the five below)
int launch_stem(const StemArgs& a, hipStream_t st);
// stand-alone depthwise conv, row form or column walker (DwArgs::rows); k x k taps, stride 1 or 2
int launch_dw(const DwArgs& a, int k, int stride, dim3 grid, hipStream_t st);
int launch_add(const int8_t* xa, const int8_t* xb, const AddQ& q, int8_t* out, long n4, hipStream_t st);   // n4: dwords
int launch_maxpool(const MapArgs& a, hipStream_t st);
int launch_resize_nn(const MapArgs& a, hipStream_t st);
// decode + NMS, one workgroup per frame (k_postprocess.hip); post_lds_bytes: its dynamic LDS for A anchors
int post_lds_bytes(int A);
int launch_postprocess(const PostArgs& p, int lds_bytes, int B, float* boxes, float* scores, float* classes, int* counts, hipStream_t st);

}  // namespace vbt
