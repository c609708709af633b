// Host-side entry points of the kernel translation units (k_*.hip).  Each kernel family is compiled in its own translation
// unit - the template instantiations of the fused MBConv / SeparableConv tiles alone are most of the library's build time -
// and the launch logic (detector.hip) reaches the kernels only through these launchers: plain argument structs in, one launch
// enqueued on `st` out.  A launcher returns VBT_OK, VBT_ERR_ARG (no such instantiation) or VBT_ERR_HIP (an LDS opt-in refused) and
// sets the error text.
#pragma once
#include "dev_common.h"
#include "fused_block.h"   // FusedArgs, MultiTiles, DwTileArgs, FB_* tile constants (+ the kernel templates)
#include "stem_block.h"    // StemBlockArgs
#include "image_block.h"   // ImageBundle, IB_*
#include "expdw_block.h"   // ExpDwArgs, XD_*
#include "expdw2_block.h"  // ExpDw2Args, XD2_*
#include "band_block.h"    // BandArgs, BD_*
#include "op_args.h"       // PwArgs, PwKernel, PwMulti, StemArgs, DwArgs, MapArgs, PostArgs

namespace vbt {

// fused MBConv / SeparableConv / BiFPN node on LDS tiles (fused_block.h): which instantiation to run
struct FusedLaunch {
  int k, stride, nbp;   // depthwise kernel size / stride, 64-channel output blocks per pass
  bool expand;          // MBConv (expand -> depthwise -> project) or SeparableConv / node (depthwise -> project)
  bool mdw;             // depthwise on the matrix pipe
  bool nt3;             // 48-channel chunks
  bool ppw2;            // 128-pixel (16 x 8) tiles
  bool dw64;            // depthwise on the 16x16x64 MFMA with immediate LDS offsets (8 x 8 or 16 x 8 tiles)
  int lds_bytes;
  unsigned grid;
  bool tpz = false;     // dw64 as a band-Toeplitz product on a quad-planar E (k_fused_mbconv_tpz.hip)
  int ntl = 0;          // live tiles of a tile-major part-filled last projection block (k_fused_mbconv_tail.hip); 0: block-major
  bool params = false;  // chunk parameters once per workgroup, through LDS (fused_block.h: PLDS; k_fused_mbconv_params*.hip); lds_bytes includes the area
};
// The (k, stride, nbp, KSe) the Toeplitz form is built for - what the MBConv steps of the shipped models resolve to (the first five
// four blocks of the EfficientNet-Lite backbones: the fifth is not cut into 8 x 8 tiles and its 16 x 8 tile does not fit 64 KB, the later
// ones have KSe >= 3) - each with 48- and 64-channel chunks on 8 x 8 tiles and, except 5x5/2 (whose 16 x 8 tile needs 66-78 KB), on
// 16 x 8 tiles.  Another shape needs a line here and one in k_fused_mbconv_tpz.hip.
static inline bool fused_tpz_built(int k, int stride, int nbp, int kse, bool ppw2) {
  return (k == 3 && stride == 2 && nbp == 1 && kse == 1) || (k == 3 && stride == 1 && nbp == 1 && kse == 1) ||
         (k == 5 && stride == 2 && nbp == 1 && kse == 1 && !ppw2) || (k == 5 && stride == 1 && nbp == 1 && kse == 2);
}
// The launches built with a live-tile count for a part-filled last projection block (fused_block.h: NTL) - again what the MBConv steps of
// the shipped models resolve to: every Toeplitz form above with the tail of its blocks (3x3: Cout = 24, two tiles; 5x5: Cout = 40 or
// Lite2's 48, three), the diagonal 16x16x64 depthwise on 8 x 8 tiles with 48-channel chunks for the two stride-2 blocks the pinned b256 plan
// keeps on it (3x3/2 -> 24 and 5x5/2 -> 40 channels, K <= 32), and the generic matrix-pipe form of the 3x3/2 block with 40 -> 80 channels
// (64 + one tile) on 64-channel chunks.  Another shape needs a line here and one in k_fused_mbconv_tail.hip.
static inline bool fused_tail_built(const FusedLaunch& L, int kse, int ntl) {
  if (L.tpz) return fused_tpz_built(L.k, L.stride, L.nbp, kse, L.ppw2) && ntl == (L.k == 3 ? 2 : 3);
  if (L.dw64) return L.nt3 && !L.ppw2 && L.stride == 2 && L.nbp == 1 && kse == 1 && ntl == (L.k == 3 ? 2 : 3);
  return L.expand && L.mdw && !L.nt3 && !L.ppw2 && !L.dw64 && L.k == 3 && L.stride == 2 && L.nbp == 2 && kse == 2 && ntl == 1;
}
// The launches built with the chunk parameters in LDS (fused_block.h: PLDS): of the launches above that the shipped plans (profiles/plan_lite0.*,
// plan_lite2.*) resolve to, those whose compiler resource report keeps the waves per SIMD of the other form with no scratch - the diagonal
// 16x16x64 depthwise of the two stride-2 blocks (8 x 8 tiles, 48-channel chunks) with its live-tile count and block-major (ntl == 0), and the
// Toeplitz depthwise on 16 x 8 tiles with 48-channel chunks, 3x3/1 with its live-tile count and 5x5/1 with it and block-major.  Returns the
// waves per SIMD the instantiation runs at (= the workgroups per CU its registers allow; a launch wants as many by LDS), 0: not built.
// Another shape needs a line here and one in k_fused_mbconv_params.hip.
static inline int fused_params_built(const FusedLaunch& L, int kse, int ntl) {
  if (!L.expand || !L.mdw || !L.dw64 || !L.nt3 || L.nbp != 1) return 0;
  const int want = L.k == 3 ? 2 : 3;   // the live-tile count fused_tail_built knows the shape by
  if (ntl != 0 && ntl != want) return 0;
  if (!L.tpz) return !L.ppw2 && L.stride == 2 && kse == 1 ? (L.k == 3 ? 4 : 3) : 0;
  if (!L.ppw2 || L.stride != 1) return 0;
  if (L.k == 3) return kse == 1 && ntl ? 4 : 0;
  return kse == 2 ? 3 : 0;
}
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
// per wave (8 waves: 2, 4 or 7; 16 waves: 1, 2 or 4)
int launch_expdw2(const ExpDw2Args& a, int k, int stride, int KS64, int nw, int gpw, unsigned grid, int lds_bytes, hipStream_t st);
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
