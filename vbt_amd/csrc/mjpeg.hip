// MJPEG export on the device (gfx950): baseline JPEG, 4:2:0, one restart interval per MCU row, of frames that already sit in device
// memory - behind vbt_overlay_draw on the same stream (include/vbt_hip.h, "MJPEG export": the bitstream contract; the numpy statement
// of it is tests/mjpeg_ref.py).  Four launches per batch:
//   mjpeg_transform_kernel  grid (groups of 32 MCUs, MCU row, frame): colour conversion of the group's 512 x 16 pixels into LDS (one
//     thread per 2 x 2 cell: four luma samples, one Cb, one Cr), then one thread per 8 x 8 block: level shift, DCT, quantisation, zigzag;
//     the int16 levels leave through LDS as one contiguous run per workgroup.  Its SCALED instantiation (vbt_mjpeg_create_scaled)
//     takes each pixel of the colour stage from a larger or smaller source through the four-tap sample of scale_core.h.
//   mjpeg_entropy_kernel    grid (MCU row, frame), one workgroup per restart interval, walking it in chunks of 256 blocks, a thread per
//     block: bit count (the DC difference is a subtraction of the neighbour block's quantised DC, so blocks code in parallel), prefix
//     sum, codes OR-ed into an LDS bit buffer at their offsets, then per thread a run of the chunk's bytes: 0xFF count, prefix sum,
//     stuffed bytes out.  The chunk's last partial byte is carried into the next chunk; the interval's is padded with 1-bits.
//   mjpeg_offsets_kernel    grid (frame): prefix sum of the frame's interval sizes -> each interval's place in the frame, the frame's size.
//   mjpeg_gather_kernel     grid (MCU row, frame): sum of the sizes of the frames before -> header (first interval), the interval's bytes,
//     RSTm or EOI, contiguous per frame and frame after frame; the table of frame offsets.
// Where the bit count is taken differs from a "count in the transform kernel" design because the DC term needs the neighbour's DC.
// Scratch is sized for the worst case (vbt_hip.h); every store is still checked against its buffer and a miss raises `flag`.
#include <algorithm>

#include "carver.h"
#include "common.h"
#include "dev_mem.h"
#include "jpeg_parse.h"
#include "scale_core.h"

namespace vbt {

constexpr int MJ_THREADS = 256;
constexpr int MJ_GROUP = 32;                                      // MCUs per workgroup of the transform kernel
constexpr int MJ_GROUP_BLOCKS = MJ_GROUP * 6;
constexpr int MJ_BLOCK_BITS = 1664;                               // >= 22 + 63 * 26 = 1660, the longest block
constexpr int MJ_CHUNK_WORDS = MJ_THREADS * MJ_BLOCK_BITS / 32 + 2;
constexpr int MJ_HEADER = 629;                                    // SOI .. SOS
constexpr int MJ_SLOT_PER_MCU = 2496;                             // >= 2 * ceil(6 * 1660 / 8): an interval's stuffed bytes, per MCU
constexpr int MJ_LROW = 33;                                       // words per block of the level staging (32 + 1: no bank conflicts)
constexpr int MJ_MAX_BATCH = 1024;

#define MJ_ZIGZAG_LIST                                                                                                                   \
  0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, \
      43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63
// natural index of zigzag position k (host: DQT) ...
static const uint8_t MJ_ZIGZAG[64] = {MJ_ZIGZAG_LIST};
// ... and zigzag position of natural index i (device)
__device__ const uint8_t MJ_ZPOS[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                        10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// T[k][n] = rint(2^13 s_k cos((2n+1) k pi / 16)): written out so that the unrolled DCT multiplies by immediates; vbt_mjpeg_create
// recomputes the 64 values in double and refuses to run if one differs.
__host__ __device__ constexpr int mj_cos(int j) {                  // rint(4096 cos(j pi / 16)), j = 1..7
  return j == 1 ? 4017 : j == 2 ? 3784 : j == 3 ? 3406 : j == 4 ? 2896 : j == 5 ? 2276 : j == 6 ? 1567 : 799;
}
__host__ __device__ constexpr int mj_T(int k, int n) {
  if (k == 0) return 2896;
  const int j = ((2 * n + 1) * k) & 31;                           // never 0, 8, 16 or 24 for k = 1..7
  return j < 8 ? mj_cos(j) : j < 16 ? -mj_cos(16 - j) : j < 24 ? -mj_cos(j - 16) : mj_cos(32 - j);
}

// tables the kernels read, one device blob per handle
struct MjTables {
  uint32_t ac[2][256];       // (length << 16) | code of symbol (run << 4) | size; [0] luma, [1] chroma
  uint32_t dc[2][16];
  uint16_t q[2][64];         // natural order
  uint8_t header[640];       // MJ_HEADER bytes
};

struct MjArgs {
  const uint8_t* frames;
  size_t frame_bytes;
  int H, W, fmt, MW, MH, B;
  const MjTables* tab;
  int16_t* levels;           // [B][MH][6 MW][64], zigzag order; the blocks of an MCU: Y00 Y01 Y10 Y11 Cb Cr
  uint8_t* slots;            // [B][MH][slot_bytes]: the stuffed bytes of each interval
  size_t slot_bytes;
  uint32_t* sizes;           // [B][MH] stuffed bytes of each interval
  uint64_t* ioff;            // [B][MH] the interval's offset inside its frame
  uint64_t* fsize;           // [B]
  uint8_t* out;              // the frames, contiguous
  size_t out_bytes;
  uint64_t* offsets;         // [max_batch + 1]: the first B + 1 are the batch's
  uint64_t* flag;            // the overflow flag, the word behind the table: cleared on the stream by every vbt_mjpeg_encode
};

__device__ __forceinline__ int mj_clip8(int v) { return min(max(v, 0), 255); }
// BT.601 limited range -> full range, the exact rational to nearest, ties away from zero
__device__ __forceinline__ int mj_expand_luma(int y) {
  const int n = (y - 16) * 255;
  return mj_clip8(n >= 0 ? (2 * n + 219) / 438 : -((-2 * n + 219) / 438));
}
__device__ __forceinline__ int mj_expand_chroma(int c) {
  const int n = (c - 128) * 255;
  return mj_clip8((n >= 0 ? (2 * n + 224) / 448 : -((-2 * n + 224) / 448)) + 128);
}

// MjScaled (vbt_mjpeg_create_scaled): pixel (py, px) of the H x W frame that vbt_scaler_run would have written, formed from the
// SH x SW source by the shared sample (scale_core.h) - coordinates clamped to H x W as the unscaled colour stage clamps them; that
// frame never exists in memory.
struct MjScale {
  const ScTap *ty, *tx, *cty, *ctx;       // luma (or RGB) pair, chroma pair
  int SH, SW;
};
struct MjScaled {
  const uint8_t* src;
  int H, W, fmt;                          // the size that is encoded
  MjScale S;
  __device__ __forceinline__ void rgb(int py, int px, int* r, int* g, int* b) const {
    const ScTap y = S.ty[min(py, H - 1)], x = S.tx[min(px, W - 1)];
    const uint8_t* r0 = src + (size_t)y.i0 * S.SW * 3;
    const uint8_t* r1 = src + (size_t)sc_i1(y.i0, S.SH) * S.SW * 3;
    const int x1 = sc_i1(x.i0, S.SW);
    *r = sc_sample_at(r0, r1, 3, 0, x.i0, x1, x.a, y.a);
    *g = sc_sample_at(r0, r1, 3, 1, x.i0, x1, x.a, y.a);
    *b = sc_sample_at(r0, r1, 3, 2, x.i0, x1, x.a, y.a);
  }
  __device__ __forceinline__ int luma(int py, int px) const {
    const ScTap y = S.ty[min(py, H - 1)], x = S.tx[min(px, W - 1)];
    return sc_sample_at(src + (size_t)y.i0 * S.SW, src + (size_t)sc_i1(y.i0, S.SH) * S.SW, 1, 0, x.i0, sc_i1(x.i0, S.SW), x.a, y.a);
  }
  __device__ __forceinline__ void chroma(int cy, int cx, int* U, int* V) const {
    const int ch = S.SH >> 1, cw = S.SW >> 1;
    const ScTap y = S.cty[min(cy, (H >> 1) - 1)], x = S.ctx[min(cx, (W >> 1) - 1)];
    const int y1 = sc_i1(y.i0, ch), x1 = sc_i1(x.i0, cw);
    const uint8_t* cp = src + (size_t)S.SH * S.SW;
    if (fmt == VBT_PIX_NV12) {
      *U = sc_sample_at(cp + (size_t)y.i0 * S.SW, cp + (size_t)y1 * S.SW, 2, 0, x.i0, x1, x.a, y.a);
      *V = sc_sample_at(cp + (size_t)y.i0 * S.SW, cp + (size_t)y1 * S.SW, 2, 1, x.i0, x1, x.a, y.a);
    } else {
      *U = sc_sample_at(cp + (size_t)y.i0 * cw, cp + (size_t)y1 * cw, 1, 0, x.i0, x1, x.a, y.a);
      cp += (size_t)ch * cw;
      *V = sc_sample_at(cp + (size_t)y.i0 * cw, cp + (size_t)y1 * cw, 1, 0, x.i0, x1, x.a, y.a);
    }
  }
};

// SCALED (a handle of vbt_mjpeg_create_scaled): A.H x A.W is what is encoded, A.frame_bytes the size of a source frame of S.SH x S.SW,
// and the colour stage takes its pixels through MjScaled; S is not read otherwise.
template <bool SCALED>
__global__ __launch_bounds__(MJ_THREADS) void mjpeg_transform_kernel(MjArgs A, MjScale S) {
  __shared__ __align__(16) uint8_t sY[MJ_GROUP][16][16];
  __shared__ __align__(16) uint8_t sC[2][MJ_GROUP][8][8];
  __shared__ uint16_t sQ[2][64];
  __shared__ uint32_t sL[MJ_GROUP_BLOCKS * MJ_LROW];
  const int tid = threadIdx.x, H = A.H, W = A.W;
  const int m0 = blockIdx.x * MJ_GROUP, nm = min(MJ_GROUP, A.MW - m0), row = blockIdx.y;
  const uint8_t* src = A.frames + (size_t)blockIdx.z * A.frame_bytes;
  if (tid < 128) sQ[tid >> 6][tid & 63] = A.tab->q[tid >> 6][tid & 63];
  // ---- colour: one thread per 2 x 2 cell, consecutive threads = consecutive cells of a row of cells
  const int cw = nm * 8;
  for (int c = tid; c < cw * 8; c += MJ_THREADS) {
    const int cxg = c % cw, cy = c / cw, m = cxg >> 3, cx = cxg & 7;
    const int px0 = m0 * 16 + cxg * 2, py0 = row * 16 + cy * 2;
    if (A.fmt == VBT_PIX_RGB24) {
      int sr = 0, sg = 0, sb = 0;
#pragma unroll
      for (int dy = 0; dy < 2; dy++) {
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
          int r, g, b;
          if constexpr (SCALED) {
            MjScaled{src, H, W, A.fmt, S}.rgb(py0 + dy, px0 + dx, &r, &g, &b);
          } else {
            const uint8_t* p = src + ((size_t)min(py0 + dy, H - 1) * W + min(px0 + dx, W - 1)) * 3;
            r = p[0]; g = p[1]; b = p[2];
          }
          sY[m][cy * 2 + dy][cx * 2 + dx] = (uint8_t)((19595 * r + 38470 * g + 7471 * b + 32768) >> 16);
          sr += r; sg += g; sb += b;
        }
      }
      sC[0][m][cy][cx] = (uint8_t)mj_clip8(((-11059 * sr - 21709 * sg + 32768 * sb + (1 << 17)) >> 18) + 128);
      sC[1][m][cy][cx] = (uint8_t)mj_clip8(((32768 * sr - 27439 * sg - 5329 * sb + (1 << 17)) >> 18) + 128);
    } else {
#pragma unroll
      for (int dy = 0; dy < 2; dy++) {
#pragma unroll
        for (int dx = 0; dx < 2; dx++)
          sY[m][cy * 2 + dy][cx * 2 + dx] = (uint8_t)mj_expand_luma(SCALED ? MjScaled{src, H, W, A.fmt, S}.luma(py0 + dy, px0 + dx)
                                                                           : src[(size_t)min(py0 + dy, H - 1) * W + min(px0 + dx, W - 1)]);
      }
      const int hh = H >> 1, hw = W >> 1, ccy = min(py0 >> 1, hh - 1), ccx = min(px0 >> 1, hw - 1);
      const uint8_t* cp = src + (size_t)H * W;
      int U, V;
      if constexpr (SCALED) {
        MjScaled{src, H, W, A.fmt, S}.chroma(py0 >> 1, px0 >> 1, &U, &V);
      } else if (A.fmt == VBT_PIX_NV12) {
        U = cp[(size_t)ccy * W + 2 * ccx];
        V = cp[(size_t)ccy * W + 2 * ccx + 1];
      } else {
        U = cp[(size_t)ccy * hw + ccx];
        V = cp[(size_t)hh * hw + (size_t)ccy * hw + ccx];
      }
      sC[0][m][cy][cx] = (uint8_t)mj_expand_chroma(U);
      sC[1][m][cy][cx] = (uint8_t)mj_expand_chroma(V);
    }
  }
  __syncthreads();
  // ---- one thread per block
  if (tid < nm * 6) {
    const int m = tid / 6, k = tid % 6;
    const uint8_t* s = k < 4 ? &sY[m][(k >> 1) * 8][(k & 1) * 8] : &sC[k - 4][m][0][0];
    const int stride = k < 4 ? 16 : 8;
    const uint16_t* q = sQ[k >= 4];
    int x[64], a[64];
#pragma unroll
    for (int y = 0; y < 8; y++) {
      const uint2 v = *(const uint2*)(s + y * stride);
#pragma unroll
      for (int n = 0; n < 4; n++) {
        x[y * 8 + n] = (int)((v.x >> (8 * n)) & 255) - 128;
        x[y * 8 + 4 + n] = (int)((v.y >> (8 * n)) & 255) - 128;
      }
    }
#pragma unroll
    for (int y = 0; y < 8; y++) {
#pragma unroll
      for (int u = 0; u < 8; u++) {
        int acc = 0;
#pragma unroll
        for (int n = 0; n < 8; n++) acc += x[y * 8 + n] * mj_T(u, n);
        a[y * 8 + u] = (acc + (1 << 10)) >> 11;
      }
    }
    int16_t* lv = (int16_t*)(sL + tid * MJ_LROW);
#pragma unroll
    for (int v = 0; v < 8; v++) {
#pragma unroll
      for (int u = 0; u < 8; u++) {
        int acc = 0;
#pragma unroll
        for (int y = 0; y < 8; y++) acc += a[y * 8 + u] * mj_T(v, y);
        const int F = (acc + (1 << 14)) >> 15, Q = q[v * 8 + u];
        const int mag = (abs(F) + (Q >> 1)) / Q;
        const int level = F < 0 ? -min(mag, (v | u) == 0 ? 1024 : 1023) : min(mag, 1023);
        lv[MJ_ZPOS[v * 8 + u]] = (int16_t)level;
      }
    }
  }
  __syncthreads();
  // ---- the group's levels are one contiguous run
  uint32_t* dst = (uint32_t*)(A.levels + (((size_t)blockIdx.z * A.MH + row) * (size_t)(6 * A.MW) + (size_t)m0 * 6) * 64);
  for (int e = tid; e < nm * 6 * 32; e += MJ_THREADS) dst[e] = sL[(e >> 5) * MJ_LROW + (e & 31)];
}

// exclusive prefix sum of v over the workgroup (every thread calls it); *total = the sum.  wsum: 4 ints of LDS
__device__ __forceinline__ int mj_block_scan(int v, int* total, int* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  __syncthreads();                                                // the readers of the call before are done with wsum
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < MJ_THREADS / 64; k++) {
    const int s = wsum[k];
    if (k < wave) base += s;
    tot += s;
  }
  *total = tot;
  return base + inc - v;
}

struct MjBitCount {
  int n = 0;
  __device__ __forceinline__ void operator()(uint32_t, int len) { n += len; }
};
// bits into the LDS buffer, most significant bit of a word first
struct MjBitSink {
  uint32_t* w;
  int pos;
  __device__ __forceinline__ void operator()(uint32_t code, int len) {   // 1 <= len <= 27, code < 2^len
    const int word = pos >> 5, off = pos & 31;
    const uint64_t v = (uint64_t)code << (64 - off - len);
    if (word + 1 < MJ_CHUNK_WORDS) {
      atomicOr(&w[word], (uint32_t)(v >> 32));
      if ((uint32_t)v) atomicOr(&w[word + 1], (uint32_t)v);
    }
    pos += len;
  }
};

__device__ __forceinline__ int mj_size(int a) { return 32 - __clz(a); }       // a > 0

// the symbols of one block: its 64 levels in zigzag order at L (16-byte aligned), `pred` the DC predictor
template <class F>
__device__ __forceinline__ void mj_walk_block(const int16_t* __restrict__ L, int pred, const uint32_t* dct, const uint32_t* act, F& put) {
  int run = 0;
  for (int j = 0; j < 8; j++) {
    const uint4 qv = ((const uint4*)L)[j];
    const uint32_t w[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int v = (int)(int16_t)(w[i >> 1] >> ((i & 1) * 16));
      if ((j | i) == 0) {
        const int diff = v - pred, s = diff ? mj_size(abs(diff)) : 0;
        const uint32_t e = dct[s];
        put(((e & 0xFFFF) << s) | (uint32_t)((diff < 0 ? diff - 1 : diff) & ((1 << s) - 1)), (int)(e >> 16) + s);
        continue;
      }
      if (v == 0) { run++; continue; }
      while (run >= 16) { put(act[0xF0] & 0xFFFF, (int)(act[0xF0] >> 16)); run -= 16; }
      const int s = mj_size(abs(v));
      const uint32_t e = act[(run << 4) | s];
      put(((e & 0xFFFF) << s) | (uint32_t)((v < 0 ? v - 1 : v) & ((1 << s) - 1)), (int)(e >> 16) + s);
      run = 0;
    }
  }
  if (run) put(act[0] & 0xFFFF, (int)(act[0] >> 16));
}

__global__ __launch_bounds__(MJ_THREADS) void mjpeg_entropy_kernel(MjArgs A) {
  __shared__ uint32_t sW[MJ_CHUNK_WORDS];
  __shared__ uint32_t sAC[2][256];
  __shared__ uint32_t sDC[2][16];
  __shared__ int wsum[MJ_THREADS / 64];
  const int tid = threadIdx.x, row = blockIdx.x, nblk = 6 * A.MW;
  for (int i = tid; i < 512; i += MJ_THREADS) sAC[i >> 8][i & 255] = A.tab->ac[i >> 8][i & 255];
  if (tid < 32) sDC[tid >> 4][tid & 15] = A.tab->dc[tid >> 4][tid & 15];
  const size_t unit = (size_t)blockIdx.y * A.MH + row;
  const int16_t* L0 = A.levels + unit * (size_t)nblk * 64;
  uint8_t* dst = A.slots + unit * A.slot_bytes;
  const size_t cap = A.slot_bytes;
  size_t out_pos = 0;                                             // bytes of the interval written so far (uniform)
  int carry_bits = 0;                                             // bits of the last, partial byte of the chunk before (uniform) ...
  uint32_t carry_word = 0;                                        // ... and that byte, in the top byte of a word
  __syncthreads();
  for (int c0 = 0; c0 < nblk; c0 += MJ_THREADS) {
    const int b = c0 + tid;
    const bool valid = b < nblk, last = c0 + MJ_THREADS >= nblk;
    int pred = 0, comp = 0;
    if (valid) {
      const int k = b % 6, m = b / 6;
      const int pb = k == 0 ? (m ? b - 3 : -1) : k < 4 ? b - 1 : (m ? b - 6 : -1);
      if (pb >= 0) pred = L0[(size_t)pb * 64];
      comp = k >= 4;
    }
    MjBitCount cnt;
    if (valid) mj_walk_block(L0 + (size_t)b * 64, pred, sDC[comp], sAC[comp], cnt);
    int total;
    const int excl = mj_block_scan(cnt.n, &total, wsum);
    const int bits = carry_bits + total;                          // <= 7 + 256 * 1660
    for (int i = tid; i < min((bits >> 5) + 2, MJ_CHUNK_WORDS); i += MJ_THREADS) sW[i] = i == 0 ? carry_word : 0u;
    __syncthreads();
    if (valid) {
      MjBitSink sink{sW, carry_bits + excl};
      mj_walk_block(L0 + (size_t)b * 64, pred, sDC[comp], sAC[comp], sink);
    }
    __syncthreads();
    int nb = bits >> 3;                                           // whole bytes of this chunk
    if (last && (bits & 7)) {                                     // the interval ends: pad with 1-bits
      if (tid == 0) sW[bits >> 5] |= ((1u << (8 - (bits & 7))) - 1) << (24 - ((bits >> 3) & 3) * 8);
      nb++;
      __syncthreads();
    }
    auto byte_at = [&](int k) { return (sW[k >> 2] >> (24 - 8 * (k & 3))) & 255u; };
    const int S = (((nb + MJ_THREADS - 1) / MJ_THREADS) + 3) & ~3;
    const int k0 = min(tid * S, nb), k1 = min(k0 + S, nb);
    int ff = 0;
    for (int k = k0; k < k1; k++) ff += byte_at(k) == 255u;
    int ff_total;
    const int ff_excl = mj_block_scan(ff, &ff_total, wsum);
    size_t p = out_pos + (size_t)k0 + (size_t)ff_excl;
    for (int k = k0; k < k1; k++) {
      const uint32_t v = byte_at(k);
      if (p < cap) dst[p] = (uint8_t)v;
      p++;
      if (v == 255u) {
        if (p < cap) dst[p] = 0;
        p++;
      }
    }
    out_pos += (size_t)nb + (size_t)ff_total;
    carry_bits = bits & 7;
    carry_word = carry_bits ? byte_at(nb) << 24 : 0u;             // (read before the next chunk's scan lets anyone clear sW)
  }
  if (tid == 0) {
    A.sizes[unit] = (uint32_t)min(out_pos, cap);
    if (out_pos > cap) *A.flag = 1;
  }
}

__global__ __launch_bounds__(MJ_THREADS) void mjpeg_offsets_kernel(MjArgs A) {
  __shared__ int wsum[MJ_THREADS / 64];
  const int tid = threadIdx.x, f = blockIdx.x;
  uint64_t carry = MJ_HEADER;
  for (int j0 = 0; j0 < A.MH; j0 += MJ_THREADS) {
    const int j = j0 + tid;
    // an interval is at most 2496 * 1024 bytes and a chunk holds 256 of them: the int scan holds the sum
    const int v = j < A.MH ? (int)A.sizes[(size_t)f * A.MH + j] + 2 : 0;   // + RSTm, or EOI behind the last
    int total;
    const int excl = mj_block_scan(v, &total, wsum);
    if (j < A.MH) A.ioff[(size_t)f * A.MH + j] = carry + (uint64_t)excl;
    carry += (uint64_t)total;
  }
  if (tid == 0) A.fsize[f] = carry;
}

__global__ __launch_bounds__(MJ_THREADS) void mjpeg_gather_kernel(MjArgs A) {
  __shared__ unsigned long long red[MJ_THREADS];
  const int tid = threadIdx.x, row = blockIdx.x, f = blockIdx.y;
  unsigned long long v = 0;
  for (int g = tid; g < f; g += MJ_THREADS) v += A.fsize[g];
  red[tid] = v;
  __syncthreads();
  for (int s = MJ_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const size_t base = (size_t)red[0];
  const size_t unit = (size_t)f * A.MH + row;
  if (row == 0) {
    for (int k = tid; k < MJ_HEADER; k += MJ_THREADS)
      if (base + k < A.out_bytes) A.out[base + k] = A.tab->header[k];
    if (tid == 0) {
      A.offsets[f] = base;
      if (f == A.B - 1) A.offsets[A.B] = base + A.fsize[f];
    }
  }
  const size_t n = A.sizes[unit], at = base + (size_t)A.ioff[unit];
  const uint8_t* src = A.slots + unit * A.slot_bytes;
  for (size_t k = tid; k < n; k += MJ_THREADS)
    if (at + k < A.out_bytes) A.out[at + k] = src[k];
  if (tid < 2 && at + n + tid < A.out_bytes)
    A.out[at + n + tid] = tid == 0 ? 0xFF : (uint8_t)(row + 1 < A.MH ? 0xD0 + (row & 7) : 0xD9);
  if (tid == 0 && at + n + 2 > A.out_bytes) *A.flag = 1;
}

}  // namespace vbt

using namespace vbt;

struct vbt_mjpeg {
  int device = 0, H = 0, W = 0, fmt = 0, quality = 0, max_batch = 0, MW = 0, MH = 0;   // H x W: the size that is encoded
  size_t frame_bytes = 0, slot_bytes = 0, out_bytes = 0;
  DevBuf<uint8_t> blob;                  // tables | offsets + flag | fsize | ioff | sizes | levels | slots | out | scale tables in one allocation
  MjArgs args{};
  bool scaled = false;                   // vbt_mjpeg_create_scaled with another size than the source's: frame_bytes is the source's
  MjScale scale{};
  int pending = 0;                       // frames of the batch that is encoded and not yet read
};

namespace {

// Annex K.1 / K.2 (natural order)
const uint8_t K1_LUMA[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t K2_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                               99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K.3 (BITS, HUFFVAL): the tables of jpeg_parse.h, which the import falls back to for a frame without DHT
const uint8_t* const DC_LUMA_BITS = jpeg_detail::DC_BITS[0];
const uint8_t* const DC_CHROMA_BITS = jpeg_detail::DC_BITS[1];
const uint8_t* const DC_VALS = jpeg_detail::DC_VALS;
const uint8_t* const AC_LUMA_BITS = jpeg_detail::AC_BITS[0];
const uint8_t* const AC_LUMA_VALS = jpeg_detail::AC_VALS[0];
const uint8_t* const AC_CHROMA_BITS = jpeg_detail::AC_BITS[1];
const uint8_t* const AC_CHROMA_VALS = jpeg_detail::AC_VALS[1];

// canonical codes (Annex C): table[symbol] = (length << 16) | code
void huff_table(const uint8_t* bits, const uint8_t* vals, uint32_t* table) {
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; len++) {
    for (int i = 0; i < bits[len - 1]; i++) table[vals[k++]] = ((uint32_t)len << 16) | code++;
    code <<= 1;
  }
}

void put16(std::vector<uint8_t>& v, int x) { v.push_back((uint8_t)(x >> 8)); v.push_back((uint8_t)x); }

void build_tables(int H, int W, int quality, MjTables* t) {
  memset(t, 0, sizeof(*t));
  huff_table(AC_LUMA_BITS, AC_LUMA_VALS, t->ac[0]);
  huff_table(AC_CHROMA_BITS, AC_CHROMA_VALS, t->ac[1]);
  huff_table(DC_LUMA_BITS, DC_VALS, t->dc[0]);
  huff_table(DC_CHROMA_BITS, DC_VALS, t->dc[1]);
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; i++) {
    t->q[0][i] = (uint16_t)std::min(std::max((K1_LUMA[i] * s + 50) / 100, 1), 255);
    t->q[1][i] = (uint16_t)std::min(std::max((K2_CHROMA[i] * s + 50) / 100, 1), 255);
  }
  std::vector<uint8_t> h = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  for (int c = 0; c < 2; c++) {
    h.insert(h.end(), {0xFF, 0xDB, 0, 67, (uint8_t)c});
    for (int k = 0; k < 64; k++) h.push_back((uint8_t)t->q[c][MJ_ZIGZAG[k]]);
  }
  h.insert(h.end(), {0xFF, 0xC0, 0, 17, 8});
  put16(h, H);
  put16(h, W);
  h.insert(h.end(), {3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
  struct { uint8_t id; const uint8_t* bits; const uint8_t* vals; int n; } dht[4] = {
      {0x00, DC_LUMA_BITS, DC_VALS, 12}, {0x10, AC_LUMA_BITS, AC_LUMA_VALS, 162}, {0x01, DC_CHROMA_BITS, DC_VALS, 12}, {0x11, AC_CHROMA_BITS, AC_CHROMA_VALS, 162}};
  for (const auto& d : dht) {
    h.insert(h.end(), {0xFF, 0xC4});
    put16(h, 19 + d.n);
    h.push_back(d.id);
    h.insert(h.end(), d.bits, d.bits + 16);
    h.insert(h.end(), d.vals, d.vals + d.n);
  }
  h.insert(h.end(), {0xFF, 0xDD, 0, 4});
  put16(h, (W + 15) / 16);
  h.insert(h.end(), {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  memcpy(t->header, h.data(), std::min(h.size(), sizeof(t->header)));
  static_assert(sizeof(t->header) >= MJ_HEADER, "header room");
  if (h.size() != MJ_HEADER) t->header[0] = 0;                    // (caught by the caller)
}

bool dct_table_ok() {
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < 8; k++)
    for (int n = 0; n < 8; n++)
      if ((int)std::rint(8192.0 * (k == 0 ? std::sqrt(1.0 / 8.0) : 0.5) * std::cos((2 * n + 1) * k * pi / 16.0)) != mj_T(k, n)) return false;
  return true;
}

}  // namespace

namespace {

// vbt_mjpeg_create (SH x SW == H x W) and vbt_mjpeg_create_scaled: frames of SH x SW in, JPEGs of H x W out
int mjpeg_create(const char* who, int device, int SH, int SW, int H, int W, int pix_fmt, int quality, int max_batch, vbt_mjpeg** out) {
  if (!out) { set_error("%s: out is NULL", who); return VBT_ERR_ARG; }
  *out = nullptr;
  const bool scaled = SH != H || SW != W;
  if (pix_fmt != VBT_PIX_RGB24 && !pix_fmt_is_yuv(pix_fmt)) { set_error("%s: unknown pixel format %d", who, pix_fmt); return VBT_ERR_ARG; }
  if (SH < 1 || SW < 1 || SH > 16384 || SW > 16384) { set_error("%s: frames of 1..16384 pixels a side, got %d x %d", who, SH, SW); return VBT_ERR_ARG; }
  if (pix_fmt_is_yuv(pix_fmt) && ((SH & 1) || (SW & 1))) { set_error("%s: YUV 4:2:0 frames have even H and W, got %d x %d", who, SH, SW); return VBT_ERR_ARG; }
  if (H < 1 || W < 1 || H > 16384 || W > 16384) { set_error("%s: an output (h and w) of 1..16384 pixels a side, got %d x %d", who, H, W); return VBT_ERR_ARG; }
  if (pix_fmt_is_yuv(pix_fmt) && ((H & 1) || (W & 1))) { set_error("%s: YUV 4:2:0 frames have even h and w, got %d x %d", who, H, W); return VBT_ERR_ARG; }
  if (quality < 1 || quality > 100) { set_error("%s: quality %d outside 1..100", who, quality); return VBT_ERR_ARG; }
  if (max_batch < 1 || max_batch > MJ_MAX_BATCH) { set_error("%s: max_batch %d outside 1..%d", who, max_batch, MJ_MAX_BATCH); return VBT_ERR_ARG; }
  MjTables tab;
  build_tables(H, W, quality, &tab);
  if (!dct_table_ok() || tab.header[0] != 0xFF) { set_error("%s: the built-in tables fail their self-check", who); return VBT_ERR_STATE; }
  const ScTableLayout SL = sc_table_layout(H, W, pix_fmt);
  std::vector<ScTap> taps;
  if (scaled) {
    taps.resize((size_t)SL.total);
    sc_build_tables(SH, SW, H, W, pix_fmt, SL, taps.data());
  }
  if (int rc = use_device(who, device)) return rc;
  std::unique_ptr<vbt_mjpeg> m(new vbt_mjpeg());
  m->device = device; m->H = H; m->W = W; m->fmt = pix_fmt; m->quality = quality; m->max_batch = max_batch;
  m->MW = (W + 15) / 16; m->MH = (H + 15) / 16;
  m->frame_bytes = sc_frame_bytes(SH, SW, pix_fmt);
  m->slot_bytes = (size_t)MJ_SLOT_PER_MCU * m->MW;
  const size_t B = (size_t)max_batch, units = B * m->MH;
  m->out_bytes = B * (MJ_HEADER + (size_t)m->MH * (m->slot_bytes + 2));
  Carver<256> C;   // tables | offsets + flag | fsize | ioff | sizes | levels | slots | out
  const auto r_tab = C.add<MjTables>(1);
  const auto r_offsets = C.add<uint64_t>(B + 2), r_fsize = C.add<uint64_t>(B), r_ioff = C.add<uint64_t>(units);
  const auto r_sizes = C.add<uint32_t>(units);
  const auto r_levels = C.add<int16_t>(units * 6 * m->MW * 64);
  const auto r_slots = C.add<uint8_t>(units * m->slot_bytes), r_out = C.add<uint8_t>(m->out_bytes);
  const auto r_taps = C.add<ScTap>(taps.size());
  const size_t total = C.padded_bytes();
  hipError_t e = m->blob.alloc(total);
  uint8_t* const blob = m->blob.get();
  if (e == hipSuccess) e = hipMemcpy(C.ptr(blob, r_tab), &tab, sizeof(tab), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(C.ptr(blob, r_offsets), 0, (B + 2) * 8);
  if (e == hipSuccess && scaled) e = hipMemcpy(C.ptr(blob, r_taps), taps.data(), taps.size() * sizeof(ScTap), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    set_error("%s: %zu bytes of device memory for %d frames of %d x %d: %s", who, total, max_batch, W, H, hipGetErrorString(e));
    return VBT_ERR_HIP;
  }
  MjArgs& A = m->args;
  A.frame_bytes = m->frame_bytes; A.H = H; A.W = W; A.fmt = pix_fmt; A.MW = m->MW; A.MH = m->MH;
  A.tab = C.ptr(blob, r_tab);
  A.offsets = C.ptr(blob, r_offsets); A.flag = A.offsets + B + 1; A.fsize = C.ptr(blob, r_fsize); A.ioff = C.ptr(blob, r_ioff);
  A.sizes = C.ptr(blob, r_sizes); A.levels = C.ptr(blob, r_levels);
  A.slots = C.ptr(blob, r_slots); A.slot_bytes = m->slot_bytes; A.out = C.ptr(blob, r_out); A.out_bytes = m->out_bytes;
  if (scaled) {
    const ScTap* t = C.ptr(blob, r_taps);
    m->scaled = true;
    m->scale = MjScale{t + SL.at[0][0], t + SL.at[0][1], t + SL.at[1][0], t + SL.at[1][1], SH, SW};
  }
  *out = m.release();
  return VBT_OK;
}

}  // namespace

extern "C" {

int vbt_mjpeg_create(int device, int H, int W, int pix_fmt, int quality, int max_batch, vbt_mjpeg** out) {
  return mjpeg_create("vbt_mjpeg_create", device, H, W, H, W, pix_fmt, quality, max_batch, out);
}

int vbt_mjpeg_create_scaled(int device, int H, int W, int h, int w, int pix_fmt, int quality, int max_batch, vbt_mjpeg** out) {
  return mjpeg_create("vbt_mjpeg_create_scaled", device, H, W, h, w, pix_fmt, quality, max_batch, out);
}

void vbt_mjpeg_destroy(vbt_mjpeg* m) {
  if (!m) return;
  if (m->blob) (void)hipSetDevice(m->device);
  delete m;   // (the blob's free waits for the kernels still using it)
}

int vbt_mjpeg_encode(vbt_mjpeg* m, const uint8_t* frames_dev, int B, void* stream) {
  if (!m || !frames_dev || B < 1) { set_error("vbt_mjpeg_encode: bad argument (handle, frames, B >= 1)"); return VBT_ERR_ARG; }
  if (B > m->max_batch) { set_error("vbt_mjpeg_encode: %d frames, the handle was created for %d", B, m->max_batch); return VBT_ERR_CAPACITY; }
  if (m->pending) { set_error("vbt_mjpeg_encode: the previous batch of %d frames has not been read (vbt_mjpeg_read)", m->pending); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(m->device));
  MjArgs A = m->args;
  A.frames = frames_dev; A.B = B;
  hipStream_t st = (hipStream_t)stream;
  VBT_HIP_CHECK(hipMemsetAsync(A.flag, 0, 8, st));
  const dim3 grid((unsigned)((m->MW + MJ_GROUP - 1) / MJ_GROUP), (unsigned)m->MH, (unsigned)B);
  if (m->scaled)
    mjpeg_transform_kernel<true><<<grid, MJ_THREADS, 0, st>>>(A, m->scale);
  else
    mjpeg_transform_kernel<false><<<grid, MJ_THREADS, 0, st>>>(A, m->scale);
  mjpeg_entropy_kernel<<<dim3((unsigned)m->MH, (unsigned)B), MJ_THREADS, 0, st>>>(A);
  mjpeg_offsets_kernel<<<dim3((unsigned)B), MJ_THREADS, 0, st>>>(A);
  mjpeg_gather_kernel<<<dim3((unsigned)m->MH, (unsigned)B), MJ_THREADS, 0, st>>>(A);
  VBT_HIP_CHECK(hipGetLastError());
  m->pending = B;
  return VBT_OK;
}

int vbt_mjpeg_read(vbt_mjpeg* m, uint8_t* host_buf, uint64_t cap, uint64_t* offsets, void* stream) {
  if (!m || !offsets || (cap > 0 && !host_buf)) { set_error("vbt_mjpeg_read: bad argument"); return VBT_ERR_ARG; }
  if (!m->pending) { set_error("vbt_mjpeg_read: no batch is pending (vbt_mjpeg_encode first)"); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(m->device));
  const int B = m->pending;
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  std::vector<uint64_t> off((size_t)m->max_batch + 2);            // the whole table and the flag behind it: one copy
  VBT_HIP_CHECK(hipMemcpy(off.data(), m->args.offsets, off.size() * 8, hipMemcpyDeviceToHost));
  memcpy(offsets, off.data(), ((size_t)B + 1) * 8);
  const uint64_t flag = off[(size_t)m->max_batch + 1];
  if (flag || off[B] > m->out_bytes) {
    m->pending = 0;                                               // nothing to read: the handle is free for the next batch
    set_error("vbt_mjpeg_read: a stream outgrew its worst-case buffer (flag %llu, %llu bytes)", (unsigned long long)flag, (unsigned long long)off[B]);
    return VBT_ERR_CAPACITY;
  }
  if (cap < off[B]) { set_error("vbt_mjpeg_read: %llu bytes, room for %llu", (unsigned long long)off[B], (unsigned long long)cap); return VBT_ERR_CAPACITY; }
  VBT_HIP_CHECK(hipMemcpy(host_buf, m->args.out, (size_t)off[B], hipMemcpyDeviceToHost));
  m->pending = 0;
  return VBT_OK;
}

}  // extern "C"
