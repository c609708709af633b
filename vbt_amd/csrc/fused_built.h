// Which fused MBConv instantiations the three special units build, one list per unit, and the predicates resolve_fused asks.  Plain C++:
// the predicates and the launchers (k_fused_mbconv_tpz.hip, k_fused_mbconv_tail.hip, k_fused_mbconv_params.hip) expand the same rows, and
// the host test walks the predicates over the whole key space.
//
// A row is one fused_block_kernel<KK, S, NBP, true, true, KSE, NT, PPW, DW64, TPZ, NTL, PLDS> (fused_block.h; PLDS is the params unit's):
//   X(KK, S, NBP, KSE, NT, PPW, DW64, TPZ, NTL)        KK x KK depthwise of stride S, NBP 64-channel output blocks per pass, KSE K-steps in
//                                                      the expand, NT = 3: 48-channel chunks (4: 64), PPW = 2: 16 x 8 tiles (1: 8 x 8), DW64 /
//                                                      TPZ: the depthwise form, NTL: live tiles of a tile-major last projection block
// and the params list adds the waves per SIMD the instantiation runs at.  Another shape needs a row in the list.
#pragma once

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

// The Toeplitz form: what the MBConv steps of the shipped models resolve to (the first four blocks of the EfficientNet-Lite backbones: the
// fifth is not cut into 8 x 8 tiles and its 16 x 8 tile does not fit 64 KB, the later ones have KSe >= 3) - each with 48- and 64-channel
// chunks on 8 x 8 tiles and, except 5x5/2 (whose 16 x 8 tile needs 66-78 KB), on 16 x 8 tiles.
#define VBT_FUSED_TPZ_ROWS(X)                                                                             \
  X(3, 2, 1, 1, 3, 1, true, true, 0) X(3, 2, 1, 1, 4, 1, true, true, 0) X(3, 2, 1, 1, 3, 2, true, true, 0) X(3, 2, 1, 1, 4, 2, true, true, 0) \
  X(3, 1, 1, 1, 3, 1, true, true, 0) X(3, 1, 1, 1, 4, 1, true, true, 0) X(3, 1, 1, 1, 3, 2, true, true, 0) X(3, 1, 1, 1, 4, 2, true, true, 0) \
  X(5, 2, 1, 1, 3, 1, true, true, 0) X(5, 2, 1, 1, 4, 1, true, true, 0)                                                                       \
  X(5, 1, 1, 2, 3, 1, true, true, 0) X(5, 1, 1, 2, 4, 1, true, true, 0) X(5, 1, 1, 2, 3, 2, true, true, 0) X(5, 1, 1, 2, 4, 2, true, true, 0)

// The launches with a live-tile count for a part-filled last projection block (fused_block.h: NTL) - again what the MBConv steps of the
// shipped models resolve to: every Toeplitz form above with the tail of its blocks (3x3: Cout = 24, two tiles; 5x5: Cout = 40 or Lite2's 48,
// three), the diagonal 16x16x64 depthwise on 8 x 8 tiles with 48-channel chunks for the two stride-2 blocks the pinned b256 plan keeps on it
// (3x3/2 -> 24 and 5x5/2 -> 40 channels, K <= 32), and the generic matrix-pipe form of the 3x3/2 block with 40 -> 80 channels (64 + one tile)
// on 64-channel chunks.
#define VBT_FUSED_TAIL_ROWS(X)                                                                            \
  X(3, 2, 1, 1, 3, 1, true, true, 2) X(3, 2, 1, 1, 4, 1, true, true, 2) X(3, 2, 1, 1, 3, 2, true, true, 2) X(3, 2, 1, 1, 4, 2, true, true, 2) \
  X(3, 1, 1, 1, 3, 1, true, true, 2) X(3, 1, 1, 1, 4, 1, true, true, 2) X(3, 1, 1, 1, 3, 2, true, true, 2) X(3, 1, 1, 1, 4, 2, true, true, 2) \
  X(5, 2, 1, 1, 3, 1, true, true, 3) X(5, 2, 1, 1, 4, 1, true, true, 3)                                                                       \
  X(5, 1, 1, 2, 3, 1, true, true, 3) X(5, 1, 1, 2, 4, 1, true, true, 3) X(5, 1, 1, 2, 3, 2, true, true, 3) X(5, 1, 1, 2, 4, 2, true, true, 3) \
  X(3, 2, 1, 1, 3, 1, true, false, 2) X(5, 2, 1, 1, 3, 1, true, false, 3)                                                                     \
  X(3, 2, 2, 2, 4, 1, false, false, 1)

// The launches with the chunk parameters in LDS (fused_block.h: PLDS): of the launches above that the shipped plans (profiles/plan_lite0.*,
// plan_lite2.*) resolve to, those whose compiler resource report keeps the waves per SIMD of the other form with no scratch - the diagonal
// 16x16x64 depthwise of the two stride-2 blocks (8 x 8 tiles, 48-channel chunks) with its live-tile count and block-major (NTL = 0), and the
// Toeplitz depthwise on 16 x 8 tiles with 48-channel chunks, 3x3/1 with its live-tile count and 5x5/1 with it and block-major.
// Last column: the waves per SIMD the instantiation runs at (= the workgroups per CU its registers allow; a launch wants as many by LDS).
#define VBT_FUSED_PARAMS_ROWS(X)                                                       \
  X(3, 2, 1, 1, 3, 1, true, false, 2, 4) X(3, 2, 1, 1, 3, 1, true, false, 0, 4)        \
  X(5, 2, 1, 1, 3, 1, true, false, 3, 3) X(5, 2, 1, 1, 3, 1, true, false, 0, 3)        \
  X(3, 1, 1, 1, 3, 2, true, true, 2, 4)                                                \
  X(5, 1, 1, 2, 3, 2, true, true, 3, 3) X(5, 1, 1, 2, 3, 2, true, true, 0, 3)

#define VBT_FUSED_COUNT_ROW(...) +1
constexpr int FUSED_TPZ_ROWS = 0 VBT_FUSED_TPZ_ROWS(VBT_FUSED_COUNT_ROW);
constexpr int FUSED_TAIL_ROWS = 0 VBT_FUSED_TAIL_ROWS(VBT_FUSED_COUNT_ROW);
constexpr int FUSED_PARAMS_ROWS = 0 VBT_FUSED_PARAMS_ROWS(VBT_FUSED_COUNT_ROW);
#undef VBT_FUSED_COUNT_ROW

// ---- a launch against one row.  The launchers ask the same functions and add what a predicate leaves open (the chunking of a Toeplitz row).

// the shape the Toeplitz form is known by: both chunkings of it are built
static inline bool fused_tpz_row(int k, int stride, int nbp, int kse, bool ppw2, int KK, int S, int NBP, int KSE, int PPW) {
  return k == KK && stride == S && nbp == NBP && kse == KSE && ppw2 == (PPW == 2);
}
// a Toeplitz row by its shape and live-tile count alone, a diagonal row also by its chunking, the generic row in full
static inline bool fused_tail_row(const FusedLaunch& L, int kse, int ntl, int KK, int S, int NBP, int KSE, int NT, int PPW, bool DW64, bool TPZ, int NTL) {
  if (L.tpz != TPZ || ntl != NTL || !fused_tpz_row(L.k, L.stride, L.nbp, kse, L.ppw2, KK, S, NBP, KSE, PPW)) return false;
  if (TPZ) return true;
  if (L.dw64 != DW64 || L.nt3 != (NT == 3)) return false;
  return DW64 || (L.expand && L.mdw);
}
static inline bool fused_params_row(const FusedLaunch& L, int kse, int ntl, int KK, int S, int NBP, int KSE, int NT, int PPW, bool DW64, bool TPZ, int NTL) {
  return L.expand && L.mdw && L.dw64 == DW64 && L.nt3 == (NT == 3) && L.tpz == TPZ && ntl == NTL &&
         fused_tpz_row(L.k, L.stride, L.nbp, kse, L.ppw2, KK, S, NBP, KSE, PPW);
}

// ---- the predicates ----
static inline bool fused_tpz_built(int k, int stride, int nbp, int kse, bool ppw2) {
#define VBT_ROW(KK, S, NBP, KSE, NT, PPW, DW64, TPZ, NTL) || fused_tpz_row(k, stride, nbp, kse, ppw2, KK, S, NBP, KSE, PPW)
  return false VBT_FUSED_TPZ_ROWS(VBT_ROW);
#undef VBT_ROW
}
static inline bool fused_tail_built(const FusedLaunch& L, int kse, int ntl) {
#define VBT_ROW(...) || fused_tail_row(L, kse, ntl, __VA_ARGS__)
  return false VBT_FUSED_TAIL_ROWS(VBT_ROW);
#undef VBT_ROW
}
// Returns the waves per SIMD of the instantiation, 0: not built.
static inline int fused_params_built(const FusedLaunch& L, int kse, int ntl) {
#define VBT_ROW(KK, S, NBP, KSE, NT, PPW, DW64, TPZ, NTL, WAVES) if (fused_params_row(L, kse, ntl, KK, S, NBP, KSE, NT, PPW, DW64, TPZ, NTL)) return WAVES;
  VBT_FUSED_PARAMS_ROWS(VBT_ROW)
#undef VBT_ROW
  return 0;
}

}  // namespace vbt
