// Host-side weight / bias layouts of the detector's kernels: one pure function per layout.  Every function reads the container blob
// (int8 weights, int32 biases, float multipliers) and shapes, and returns the host image of what a kernel reads; none touches the
// model or HIP.  Weight orders in the blob: convs (stem, pointwise) are rows [cout][K], depthwise convs are taps [tap][C].
// The functions sit at global scope, like the geometry headers they share with the kernels (fused_params_geom.h, tpz_geom.h, halo_geom.h).
// v4i, the 16-byte int vector of the MFMA operands, is the includer's, named at global scope before this header: planner.hip names
// dev_common.h's (using vbt::v4i), a plain C++ program (tests/test_band_pack_host.py, tests/test_toeplitz_pack_host.py) defines its own.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fused_params_geom.h"

// Packed MFMA A-operand layout: [(nb*KS + ks)*4 + t][lane][8 bytes]; lane (i = lane&15, g = lane>>4) holds
// W[cout = 64nb + 16(i>>2) + 4t + (i&3)][k = 32ks + 8g + j].  kmap translates packed k -> source k (or -1).
inline void pack_weights(const int8_t* w, int N, int K, int KS, int NB, const std::vector<int>* kmap, std::vector<long>& out) {
  out.assign((size_t)NB * KS * 4 * 64, 0);
  int8_t* o = (int8_t*)out.data();
  for (int nb = 0; nb < NB; nb++)
    for (int ks = 0; ks < KS; ks++)
      for (int t = 0; t < 4; t++)
        for (int lane = 0; lane < 64; lane++) {
          int i = lane & 15, g = lane >> 4;
          int co = 64 * nb + 16 * (i >> 2) + 4 * t + (i & 3);
          for (int j = 0; j < 8; j++) {
            int kp = 32 * ks + 8 * g + j;
            int k = kmap ? (kp < (int)kmap->size() ? (*kmap)[kp] : -1) : (kp < K ? kp : -1);
            int8_t v = (co < N && k >= 0) ? w[(size_t)co * K + k] : 0;
            o[((((size_t)(nb * KS + ks) * 4 + t) * 64 + lane) * 8) + j] = v;
          }
        }
}

// 16x16x64 layout: [(nb*KS + ks)*4 + t][lane][16 bytes]; lane (i = lane&15, g = lane>>4) holds
// W[cout = 64nb + 16(i>>2) + 4t + (i&3)][k = 64ks + 16g + j], zero beyond N / K.
inline void pack_weights64(const int8_t* w, int N, int K, int KS, int NB, std::vector<v4i>& out, const std::vector<int>* kmap = nullptr) {
  out.assign((size_t)NB * KS * 4 * 64, (v4i){0, 0, 0, 0});
  int8_t* o = (int8_t*)out.data();
  for (int nb = 0; nb < NB; nb++)
    for (int ks = 0; ks < KS; ks++)
      for (int t = 0; t < 4; t++)
        for (int lane = 0; lane < 64; lane++) {
          const int i = lane & 15, g = lane >> 4, co = 64 * nb + 16 * (i >> 2) + 4 * t + (i & 3);
          for (int j = 0; j < 16; j++) {
            const int kp = 64 * ks + 16 * g + j;
            const int k = kmap ? (kp < (int)kmap->size() ? (*kmap)[kp] : -1) : (kp < K ? kp : -1);
            o[((((size_t)(nb * KS + ks) * 4 + t) * 64 + lane) * 16) + j] = (co < N && k >= 0) ? w[(size_t)co * K + k] : 0;
          }
        }
}

// The same with a tile-major part-filled last block (N % 64 != 0 and NB == ceil(N / 64)): the full blocks are pack_weights64's byte for
// byte, [(nb*KS + ks)*4 + t][lane]; the last block holds only its NTL = ceil((N % 64) / 16) live tiles, [(NB-1)*KS*4 + ks*NTL + t][lane],
// and lane (i, g) of tile t holds W[cout = 64(NB-1) + 16t + i][k = 64ks + 16g + j], zero beyond N / K.  Lane (r, g) of the accumulator of
// tile t then ends with channels 64(NB-1) + 16t + 4g .. + 3 of pixel r (pack_band_pw's order), so a kernel multiplies and requantises NTL
// tiles of that block instead of four part-filled ones.  N % 64 == 0 (or padding blocks past N): exactly pack_weights64.
inline int proj_tail_tiles(int N) { return ((N % 64) + 15) / 16; }
inline void pack_weights64_tail(const int8_t* w, int N, int K, int KS, int NB, std::vector<v4i>& out, const std::vector<int>* kmap = nullptr) {
  if (N % 64 == 0 || NB != (N + 63) / 64) { pack_weights64(w, N, K, KS, NB, out, kmap); return; }
  const int NTL = proj_tail_tiles(N), nbl = NB - 1;
  std::vector<v4i> full;
  pack_weights64(w, 64 * nbl, K, KS, nbl, full, kmap);   // (rows 0 .. 64 nbl - 1 only: whole blocks)
  out.assign((size_t)nbl * KS * 4 * 64 + (size_t)KS * NTL * 64, (v4i){0, 0, 0, 0});
  std::copy(full.begin(), full.end(), out.begin());
  int8_t* o = (int8_t*)(out.data() + (size_t)nbl * KS * 4 * 64);
  for (int ks = 0; ks < KS; ks++)
    for (int t = 0; t < NTL; t++)
      for (int lane = 0; lane < 64; lane++) {
        const int i = lane & 15, g = lane >> 4, co = 64 * nbl + 16 * t + i;
        for (int j = 0; j < 16; j++) {
          const int kp = 64 * ks + 16 * g + j;
          const int k = kmap ? (kp < (int)kmap->size() ? (*kmap)[kp] : -1) : (kp < K ? kp : -1);
          o[(((size_t)(ks * NTL + t) * 64 + lane) * 16) + j] = (co < N && k >= 0) ? w[(size_t)co * K + k] : 0;
        }
      }
}

// Zero point folded into the bias: out[c] = bq[c] - zp * sum_k w_c[k] for c < n, zero up to `padded` entries.  W_ROWS: w_c[k] =
// w[c*K + k] (convs); W_TAPS: w_c[k] = w[k*n + c] (depthwise, K taps).  A kernel that accumulates u = x_q + 128 passes zp = 128 + z_x.
enum WLayout { W_ROWS, W_TAPS };
inline std::vector<int> fold_bias(const int32_t* bq, const int8_t* w, int n, int K, int zp, WLayout layout, int padded = 0) {
  std::vector<int> out(std::max(n, padded), 0);
  for (int c = 0; c < n; c++) {
    long sw = 0;
    for (int k = 0; k < K; k++) sw += layout == W_ROWS ? w[(size_t)c * K + k] : w[(size_t)k * n + c];
    out[c] = (int)((long)bq[c] - (long)zp * sw);
  }
  return out;
}
// n floats (multipliers; depthwise weights as floats) followed by zeros up to `padded` entries
template <typename T>
inline std::vector<float> pad_floats(const T* v, int n, int padded) {
  std::vector<float> out(std::max(n, padded), 0.0f);
  for (int c = 0; c < n; c++) out[c] = (float)v[c];
  return out;
}
// depthwise weights as floats, [tap][Cp] (the VALU depthwise of the fused tiles; Cp == C: the stand-alone walkers)
inline std::vector<float> dw_weights_f32(const int8_t* w, int C, int kk, int Cp) {
  std::vector<float> out((size_t)kk * Cp, 0.0f);
  for (int t = 0; t < kk; t++)
    for (int c = 0; c < C; c++) out[(size_t)t * Cp + c] = (float)w[(size_t)t * C + c];
  return out;
}

// Depthwise on the matrix pipe, 16x16x32 form: [chunk][cg][m][lane][8], chunks of `group_channels` (64, or 48 for the unpadded
// chunking of fused_block.h) = cg groups of 16: lane (i = lane&15 -> channel group_channels*chunk + 16*cg + i, g): k = 8g + j ->
// tap 2m + (g>>1), channel-in-group 8(g&1) + j; non-zero only on the diagonal
inline std::vector<long> pack_dw_diag(const int8_t* w, int C, int kk, int group_channels) {
  const int NCG = group_channels / 16, nch = (C + group_channels - 1) / group_channels, KT = (kk + 1) / 2;
  std::vector<long> out((size_t)nch * NCG * KT * 64, 0);
  int8_t* o = (int8_t*)out.data();
  for (int ch = 0; ch < nch; ch++)
    for (int cg = 0; cg < NCG; cg++)
      for (int mi = 0; mi < KT; mi++)
        for (int lane = 0; lane < 64; lane++) {
          const int i = lane & 15, g = lane >> 4, c = group_channels * ch + 16 * cg + i, tap = 2 * mi + (g >> 1);
          for (int j = 0; j < 8; j++)
            o[((((size_t)(ch * NCG + cg) * KT + mi) * 64 + lane) * 8) + j] = (tap < kk && 8 * (g & 1) + j == i && c < C) ? w[(size_t)tap * C + c] : 0;
        }
  return out;
}

// Depthwise in the 16x16x64 form of the fused tiles and the stem block (FusedArgs::wd64, StemBlockArgs::wd64): [q][m][lane] x 16 B
// for nq groups of 16 channels, channel 16q + i on the diagonal byte i.  k = 3: m = kernel row, g = column (g < 3).  k = 5: m < 5 =
// kernel row with columns 0..3 in g, m = 5 holds column 4 of rows 0..3, m = 6 the last tap.
inline std::vector<v4i> pack_dw64(const int8_t* w, int C, int k, int nq) {
  const int K64 = k == 3 ? 3 : 7;
  std::vector<v4i> out((size_t)nq * K64 * 64, (v4i){0, 0, 0, 0});
  int8_t* o = (int8_t*)out.data();
  for (int q = 0; q < nq; q++)
    for (int mi = 0; mi < K64; mi++)
      for (int lane = 0; lane < 64; lane++) {
        const int i = lane & 15, g = lane >> 4, c = 16 * q + i;
        int tap = -1;
        if (k == 3) tap = g < 3 ? mi * 3 + g : -1;
        else if (mi < 5) tap = mi * 5 + g;
        else if (mi == 5) tap = g * 5 + 4;
        else tap = g == 0 ? 24 : -1;
        if (tap >= 0 && c < C) o[(((size_t)q * K64 + mi) * 64 + lane) * 16 + i] = w[(size_t)tap * C + c];
      }
  return out;
}
// FusedArgs::wd64c: one byte per operand of pack_dw64, the diagonal byte of each lane: [q][lane][8], byte m
inline std::vector<long> pack_dw64_compact(const std::vector<v4i>& w64, int k) {
  const int K64 = k == 3 ? 3 : 7, nq = (int)(w64.size() / ((size_t)K64 * 64));
  std::vector<long> out((size_t)nq * 64, 0);
  const int8_t* o = (const int8_t*)w64.data();
  int8_t* oc = (int8_t*)out.data();
  for (int q = 0; q < nq; q++)
    for (int mi = 0; mi < K64; mi++)
      for (int lane = 0; lane < 64; lane++)
        oc[((size_t)q * 64 + lane) * 8 + mi] = o[(((size_t)q * K64 + mi) * 64 + lane) * 16 + (lane & 15)];
  return out;
}

// Expand conv of the 48-channel chunking (FusedArgs::we3): [(c*KS + ks)*3 + t][lane][8]; lane (i, kg) holds
// W[cout = 48c + 12(i>>2) + 4t + (i&3)][k = 32ks + 8kg + j]
inline std::vector<long> pack_expand48(const int8_t* w, int Ce, int K, int KS) {
  const int nch3 = Ce / 48;
  std::vector<long> out((size_t)nch3 * KS * 3 * 64, 0);
  int8_t* o = (int8_t*)out.data();
  for (int c = 0; c < nch3; c++)
    for (int ks = 0; ks < KS; ks++)
      for (int t = 0; t < 3; t++)
        for (int lane = 0; lane < 64; lane++) {
          const int i = lane & 15, kg = lane >> 4, co = 48 * c + 12 * (i >> 2) + 4 * t + (i & 3);
          for (int j = 0; j < 8; j++) {
            const int k = 32 * ks + 8 * kg + j;
            o[((((size_t)(c * KS + ks) * 3 + t) * 64 + lane) * 8) + j] = k < K ? w[(size_t)co * K + k] : 0;
          }
        }
  return out;
}
// packed K of the 48-channel projection -> source channel: 64 slots per chunk, the first 48 used
inline std::vector<int> kmap48(int Ce) {
  std::vector<int> kmap((size_t)(Ce / 48) * 64, -1);
  for (int c = 0; c < Ce / 48; c++)
    for (int q = 0; q < 48; q++) kmap[(size_t)c * 64 + q] = 48 * c + q;
  return kmap;
}

// Row-band kernel (band_block.h), depthwise 3x3 in the 16x16x64 form: [cg][m][lane] x 16 B, tap 4m + g, diagonal byte i
inline std::vector<v4i> pack_band_dw(const int8_t* w, int C) {
  const int NCG = (C + 15) / 16;
  std::vector<v4i> out((size_t)NCG * 3 * 64, (v4i){0, 0, 0, 0});
  int8_t* o = (int8_t*)out.data();
  for (int cg = 0; cg < NCG; cg++)
    for (int mi = 0; mi < 3; mi++)
      for (int lane = 0; lane < 64; lane++) {
        const int i = lane & 15, g = lane >> 4, ch = 16 * cg + i, tap = 4 * mi + g;
        for (int j = 0; j < 16; j++) o[(((size_t)(cg * 3 + mi) * 64 + lane) * 16) + j] = (tap < 9 && j == i && ch < C) ? w[(size_t)tap * C + ch] : 0;
      }
  return out;
}
// Row-band kernel, chained form (C <= 64), the same operands in compact form: [cg][lane] x 4 B over four channel groups.  Byte m (m = 0..2) of
// lane (i, g) is the one non-zero byte of pack_band_dw's operand (cg, m, lane): the weight of tap 4m + g for channel 16cg + i, zero where
// 4m + g > 8 or the channel is past C.  The kernel rebuilds the 16-byte operand in registers (dev_common.h: diag_operand).
inline std::vector<unsigned> pack_band_dw_compact(const int8_t* w, int C) {
  std::vector<unsigned> out((size_t)4 * 64, 0u);
  for (int cg = 0; cg < 4; cg++)
    for (int lane = 0; lane < 64; lane++) {
      const int i = lane & 15, g = lane >> 4, ch = 16 * cg + i;
      unsigned v = 0;
      for (int mi = 0; mi < 3; mi++) {
        const int tap = 4 * mi + g;
        if (tap < 9 && ch < C) v |= (unsigned)(uint8_t)w[(size_t)tap * C + ch] << (8 * mi);
      }
      out[(size_t)cg * 64 + lane] = v;
    }
  return out;
}
// Row-band kernel, projection: [t][ks][lane] x 16 B; lane (i, g) holds W[cout = 16t + i][k = 64ks + 16g + j]
inline std::vector<v4i> pack_band_pw(const int8_t* w, int N, int C) {
  const int NT = (N + 15) / 16, KS = (C + 63) / 64;
  std::vector<v4i> out((size_t)NT * KS * 64, (v4i){0, 0, 0, 0});
  int8_t* o = (int8_t*)out.data();
  for (int t = 0; t < NT; t++)
    for (int ks = 0; ks < KS; ks++)
      for (int lane = 0; lane < 64; lane++) {
        const int i = lane & 15, g = lane >> 4, co = 16 * t + i;
        for (int j = 0; j < 16; j++) {
          const int k = 64 * ks + 16 * g + j;
          o[((((size_t)t * KS + ks) * 64 + lane) * 16) + j] = (co < N && k < C) ? w[(size_t)co * C + k] : 0;
        }
      }
  return out;
}
// Row-band kernel, projection of the chained form (C = 64): [t][lane] x 16 B in the K order the depthwise leaves in registers; lane
// (i, g), byte 4cg + j holds W[cout = 16t + i][k = 16cg + 4g + j].  The MFMA pairs byte (g, p) of A with byte (g, p) of B and sums in
// int32, so any K order the two operands share gives the same sum: each (t, i) row is a permutation of pack_band_pw's.
inline std::vector<v4i> pack_band_pw_chain(const int8_t* w, int N, int C) {
  const int NT = (N + 15) / 16;
  std::vector<v4i> out((size_t)NT * 64, (v4i){0, 0, 0, 0});
  int8_t* o = (int8_t*)out.data();
  for (int t = 0; t < NT; t++)
    for (int lane = 0; lane < 64; lane++) {
      const int i = lane & 15, g = lane >> 4, co = 16 * t + i;
      for (int cg = 0; cg < 4; cg++)
        for (int j = 0; j < 4; j++) {
          const int k = 16 * cg + 4 * g + j;
          o[((size_t)t * 64 + lane) * 16 + 4 * cg + j] = (co < N && k < C) ? w[(size_t)co * C + k] : 0;
        }
    }
  return out;
}

// Stem conv K order of the stand-alone stem kernel (3x3x3 -> 32 packed K): 8g + j -> (ky = g, kx = j/3, c = j%3) for g < 3,
// 24 + j -> (ky = j, kx = 2, c = 2)
inline std::vector<int> stem_kmap() {
  std::vector<int> kmap(32, -1);
  for (int g = 0; g < 3; g++)
    for (int j = 0; j < 8; j++) kmap[8 * g + j] = (g * 3 + j / 3) * 3 + j % 3;
  for (int j = 0; j < 3; j++) kmap[24 + j] = (j * 3 + 2) * 3 + 2;
  return kmap;
}
// Stem block (stem_block.h), stem conv: [t][lane][8], cout = 8(i>>2) + 4t + (i&3); K index 8kg + j -> kernel row kg, byte j of its
// 9 (kg < 3); (row j, byte 8) for kg == 3, j < 3
inline std::vector<long> pack_stem_block_stem(const int8_t* w) {
  std::vector<long> out(2 * 64, 0);
  int8_t* o = (int8_t*)out.data();
  for (int t = 0; t < 2; t++)
    for (int lane = 0; lane < 64; lane++) {
      const int i = lane & 15, kg = lane >> 4, co = 8 * (i >> 2) + 4 * t + (i & 3);
      for (int j = 0; j < 8; j++) {
        const int f = kg < 3 ? kg * 9 + j : (j < 3 ? j * 9 + 8 : -1);
        o[((size_t)t * 64 + lane) * 8 + j] = f >= 0 ? w[(size_t)co * 27 + f] : 0;
      }
    }
  return out;
}
// Stem block, projection: [lane][8], row i = cout i (N <= 16), K = 32: k = 8kg + j
inline std::vector<long> pack_stem_block_proj(const int8_t* w, int N) {
  std::vector<long> out(64, 0);
  int8_t* o = (int8_t*)out.data();
  for (int lane = 0; lane < 64; lane++) {
    const int i = lane & 15, kg = lane >> 4;
    for (int j = 0; j < 8; j++) o[(size_t)lane * 8 + j] = i < N ? w[(size_t)i * 32 + 8 * kg + j] : 0;
  }
  return out;
}
// Stem block, direct form, stem conv on the 16x16x64 MFMA: [t][lane] x 16 B, cout as above.  The B operand of lane group g < 3 is the
// 16 bytes of the raw row 2 hy + g from the pixel's first byte on: byte j < 9 = tap (kernel row g, byte j of its 9); every other byte
// (the row's next pixels, lane group 3) is zero here, so whatever the kernel feeds there does not count
inline std::vector<v4i> pack_stem_block_stem64(const int8_t* w) {
  std::vector<v4i> out(2 * 64, (v4i){0, 0, 0, 0});
  int8_t* o = (int8_t*)out.data();
  for (int t = 0; t < 2; t++)
    for (int lane = 0; lane < 64; lane++) {
      const int i = lane & 15, g = lane >> 4, co = 8 * (i >> 2) + 4 * t + (i & 3);
      for (int j = 0; j < 9 && g < 3; j++) o[((size_t)t * 64 + lane) * 16 + j] = w[(size_t)co * 27 + g * 9 + j];
    }
  return out;
}
// Stem block, direct form, projection: [lane][8], row i = cout i (N <= 16) in the K order the depthwise leaves in registers: lane
// (i, g), byte 4cg + j holds W[i][k = 16cg + 4g + j] (a permutation of pack_stem_block_proj's row: see pack_band_pw_chain)
inline std::vector<long> pack_stem_block_proj_chain(const int8_t* w, int N) {
  std::vector<long> out(64, 0);
  int8_t* o = (int8_t*)out.data();
  for (int lane = 0; lane < 64; lane++) {
    const int i = lane & 15, g = lane >> 4;
    for (int cg = 0; cg < 2; cg++)
      for (int j = 0; j < 4; j++) o[(size_t)lane * 8 + 4 * cg + j] = i < N ? w[(size_t)i * 32 + 16 * cg + 4 * g + j] : 0;
  }
  return out;
}

// Expand + depthwise kernels (expdw_block.h), expand panels: [(c*KS + ks)*4 + t][lane] x 16 B; lane (i, g) holds
// W[cout = 64c + 16t + i][k = 64ks + 16g + j]
inline std::vector<v4i> pack_expdw_expand(const int8_t* w, int Ce, int K) {
  const int nch = (Ce + 63) / 64, KS = (K + 63) / 64;
  std::vector<v4i> out((size_t)nch * KS * 4 * 64, (v4i){0, 0, 0, 0});
  int8_t* o = (int8_t*)out.data();
  for (int c = 0; c < nch; c++)
    for (int ks = 0; ks < KS; ks++)
      for (int t = 0; t < 4; t++)
        for (int lane = 0; lane < 64; lane++) {
          const int i = lane & 15, g = lane >> 4, ch = 64 * c + 16 * t + i;
          for (int j = 0; j < 16; j++) {
            const int k = 64 * ks + 16 * g + j;
            o[((((size_t)(c * KS + ks) * 4 + t) * 64 + lane) * 16) + j] = (ch < Ce && k < K) ? w[(size_t)ch * K + k] : 0;
          }
        }
  return out;
}
// Expand + depthwise, first form, depthwise taps: [c][cg][lane][8], byte m = the weight of channel 64c + 16cg + i at tap 4m + g
inline std::vector<long> pack_expdw_taps(const int8_t* w, int Ce, int kk) {
  const int nch = (Ce + 63) / 64, KT = (kk + 3) / 4;
  std::vector<long> out((size_t)nch * 4 * 64, 0);
  int8_t* o = (int8_t*)out.data();
  for (int c = 0; c < nch; c++)
    for (int cg = 0; cg < 4; cg++)
      for (int mi = 0; mi < KT; mi++)
        for (int lane = 0; lane < 64; lane++) {
          const int i = lane & 15, g = lane >> 4, ch = 64 * c + 16 * cg + i, tap = 4 * mi + g;
          o[(((size_t)(c * 4 + cg)) * 64 + lane) * 8 + mi] = (tap < kk && ch < Ce) ? w[(size_t)tap * Ce + ch] : 0;
        }
  return out;
}
// Band-Toeplitz depthwise (expdw2_block.h; fused_block.h: TPZ), tap table of the nq channel quads from channel `base` on:
// [q][m][lane] x 4 bytes.  Operand row i of lane (i, g) computes output pixel i>>2 of a position (1 x 4 at stride 1, 2 x 2 at
// stride 2) for channel base + 4q + (i&3); byte j = the weight at kernel row 2m + (g>>1) - S*dy, column 4(g&1) + j - S*dx, zero
// outside the k x k kernel and past channel Ce.  expdw2: one table per 64-channel chunk c (base 64c, 16 quads); the fused tiles:
// one table over all quads, which serves 64- and 48-channel chunks alike (chunk c starts at quad 16c / 12c).
inline std::vector<unsigned> pack_expdw2_taps(const int8_t* w, int Ce, int base, int nq, int k, int S) {
  const int KT2 = (S * (S - 1) + k + 1) / 2;
  std::vector<unsigned> out((size_t)nq * KT2 * 64, 0);
  for (int q = 0; q < nq; q++)
    for (int mi = 0; mi < KT2; mi++)
      for (int lane = 0; lane < 64; lane++) {
        const int i = lane & 15, g = lane >> 4, qq = i >> 2, cc = i & 3, ch = base + 4 * q + cc;
        const int dy = S == 2 ? qq >> 1 : 0, dx = S == 2 ? qq & 1 : qq;   // the output pixel of the position this operand row computes
        const int ty = 2 * mi + (g >> 1) - S * dy;
        unsigned w4 = 0;
        for (int j = 0; j < 4; j++) {
          const int tx = 4 * (g & 1) + j - S * dx;
          if (ty >= 0 && ty < k && tx >= 0 && tx < k && ch < Ce) w4 |= (unsigned)(uint8_t)w[(size_t)(ty * k + tx) * Ce + ch] << (8 * j);
        }
        out[((size_t)q * KT2 + mi) * 64 + lane] = w4;
      }
  return out;
}

// Per-chunk parameter block of the fused MBConv tile kernels (fused_params_geom.h; fused_block.h: PLDS): everything a chunk's three
// stages read, as one contiguous record per chunk, so that a workgroup fetches it once and hands it to its waves through LDS.  The
// sources are the host images of the arrays the kernels index today, for ONE chunking (NT = 4: we, wdm, wp / wpt; NT = 3: we3, wdm3,
// wp3 / wpt3), one depthwise form (wdw = wd64c, wtz or wdm / wdm3) and one panel layout (NTL > 0: the tile-major panel):
struct FusedParamsSrc {
  const long* we; const int* be; const float* me;         // expand operands | bias | multipliers (padded to 64-channel chunks)
  const void* wdw; const int* bdm; const float* md;       // depthwise operands of the form | raw-input bias | multipliers
  const v4i* wproj; int KSp;                              // projection panel and its K-steps (= chunks)
  const int* bp; const float* mp;                         // projection bias | multipliers, 64 NBP entries each
};
inline size_t fused_chunk_params_bytes(const FusedParamsGeom& g, int nch) { return (size_t)nch * g.chunk + g.pb; }
inline std::vector<unsigned char> pack_fused_chunk_params(const FusedParamsGeom& g, int NT, int NBP, int NTL, int nch, const FusedParamsSrc& s) {
  std::vector<unsigned char> out(fused_chunk_params_bytes(g, nch), 0);
  const int CH = 16 * NT, NBW = NTL ? NBP - 1 : NBP;
  for (int c = 0; c < nch; c++) {
    unsigned char* R = out.data() + (size_t)c * g.chunk;
    memcpy(R, (const unsigned char*)s.we + (size_t)c * g.o_be, g.o_be);
    memcpy(R + g.o_be, s.be + c * CH, 4 * CH);
    memcpy(R + g.o_me, s.me + c * CH, 4 * CH);
    R += g.pe;
    memcpy(R, (const unsigned char*)s.wdw + (size_t)c * g.o_bd, g.o_bd);
    memcpy(R + g.o_bd, s.bdm + c * CH, 4 * CH);
    memcpy(R + g.o_md, s.md + c * CH, 4 * CH);
    R += g.pd;
    for (int nb = 0; nb < NBW; nb++) memcpy(R + nb * 4096, s.wproj + ((size_t)(nb * s.KSp + c) * 4) * 64, 4096);
    if (NTL) memcpy(R + NBW * 4096, s.wproj + ((size_t)NBW * s.KSp * 4 + (size_t)c * NTL) * 64, NTL * 1024);
  }
  unsigned char* T = out.data() + (size_t)nch * g.chunk;
  memcpy(T, s.bp, NBP * 256);
  memcpy(T + NBP * 256, s.mp, NBP * 256);
  return out;
}
