// Pointwise convs of the int8 detector, one graph op per launch (six forms, pw_a ... pw_f) or several in one grid (pw_multi_kernel),
// and their launchers (launchers.h; argument structs: op_args.h).  The only unit that sees these kernels.
#include "launchers.h"
#include "dev_common.h"

namespace vbt {

// ------------------------------------------------------------------------------------------
// pointwise conv on the gfx950 double-rate int8 MFMA (v_mfma_i32_16x16x64_i8: same 16 issue cycles as the legacy
// 16x16x32 form for twice the K; measured in tools/probes).  A operand = packed weights, B operand = 16 input channels
// of one pixel per lane (one 16-byte load).  K is padded to a multiple of 64 with zero weights: the activation bytes
// read beyond a pixel's K channels (the next pixel, or the arena slack) multiply zeros.
// wp = packed weights [nb][ks][t][lane] x 16 bytes (pack_weights64).
// Epilogue: requantisation, optionally followed by the block's residual ADD (integer, XNNPACK qs8-vadd) with `res` (ResArgs).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void store_tile_r(const v4i acc[4], const Epi& e, const ResArgs& ra, int8_t* __restrict__ out, long m, int N,
                                             int nb, int g) {
  int c0 = nb * 64 + 16 * g;
  if (c0 >= N) return;
  unsigned d[4];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    int4 b = *(const int4*)(e.bias + c0 + 4 * t);
    float4 mu = *(const float4*)(e.mult + c0 + 4 * t);
    d[t] = rq_pack_i(acc[t], b, mu, e.rq);
  }
  if (ra.res) {   // N % 8 == 0 for every residual block
    const int8_t* r = ra.res + m * N + c0;
#pragma unroll
    for (int t = 0; t < 4; t++)
      if (c0 + 4 * t < N) d[t] = addq4(d[t], *(const unsigned*)(r + 4 * t), ra.q);
  }
  int8_t* o = out + m * N + c0;
  if ((N & 15) == 0) {
    *(uint4*)o = make_uint4(d[0], d[1], d[2], d[3]);
  } else if ((N & 3) == 0) {
#pragma unroll
    for (int t = 0; t < 4; t++)
      if (c0 + 4 * t < N) *(unsigned*)(o + 4 * t) = d[t];
  } else {
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (c0 + 4 * t + j < N) o[4 * t + j] = (int8_t)(d[t] >> (8 * j));
  }
}
// epilogue operands of one lane's 16 output channels (bias, multipliers, residual bytes): requested BEFORE the K loop so
// that their latency overlaps the weight / activation streams instead of following the last MFMA
struct EpiRegs {
  int4 b[4];
  float4 mu[4];
  unsigned res[4];
};
__device__ __forceinline__ void load_epi(EpiRegs& er, const Epi& e, const ResArgs& ra, long m, int N, int nb, int g) {
  const int c0 = min(nb * 64 + 16 * g, ((N + 15) & ~15) - 16);   // (bias / mult arrays are padded to 64-channel blocks)
#pragma unroll
  for (int t = 0; t < 4; t++) {
    er.b[t] = *(const int4*)(e.bias + c0 + 4 * t);
    er.mu[t] = *(const float4*)(e.mult + c0 + 4 * t);
    er.res[t] = 0u;
  }
  if (ra.res) {
    const int8_t* r = ra.res + m * N + nb * 64 + 16 * g;
#pragma unroll
    for (int t = 0; t < 4; t++)
      if (nb * 64 + 16 * g + 4 * t < N) er.res[t] = *(const unsigned*)(r + 4 * t);
  }
}
__device__ __forceinline__ void store_tile_e(const v4i acc[4], const EpiRegs& er, const Epi& e, const ResArgs& ra, int8_t* __restrict__ out,
                                             long m, int N, int nb, int g) {
  int c0 = nb * 64 + 16 * g;
  if (c0 >= N) return;
  unsigned d[4];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    d[t] = rq_pack_i(acc[t], er.b[t], er.mu[t], e.rq);
    if (ra.res) d[t] = addq4(d[t], er.res[t], ra.q);
  }
  int8_t* o = out + m * N + c0;
  if ((N & 15) == 0) {
    *(uint4*)o = make_uint4(d[0], d[1], d[2], d[3]);
  } else if ((N & 3) == 0) {
#pragma unroll
    for (int t = 0; t < 4; t++)
      if (c0 + 4 * t < N) *(unsigned*)(o + 4 * t) = d[t];
  } else {
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (c0 + 4 * t + j < N) o[4 * t + j] = (int8_t)(d[t] >> (8 * j));
  }
}
// the tile-major part-filled last block `nb` (pack_weights64_tail; N % 4 == 0): tile t of lane (r, g) holds channels 64 nb + 16 t + 4 g .. + 3
// of pixel m: bias, multipliers and the residual dword from that offset, one dword stored per live tile.  The tile loop is a compile-time
// count; only the last tile's store can be off for part of the lanes (N % 16 != 0).
template <int NTL>
__device__ __forceinline__ void store_tail_tiles(const v4i acc[4], const Epi& e, const ResArgs& ra, int8_t* __restrict__ out, long m, int N,
                                                 int nb, int g) {
#pragma unroll
  for (int t = 0; t < NTL; t++) {
    const int c = nb * 64 + 16 * t + 4 * g;   // (bias / mult arrays are padded to 64-channel blocks)
    const int4 b = *(const int4*)(e.bias + c);
    const float4 mu = *(const float4*)(e.mult + c);
    if (c < N) {
      unsigned d = rq_pack_i(acc[t], b, mu, e.rq);
      if (ra.res) d = addq4(d, *(const unsigned*)(ra.res + m * N + c), ra.q);
      *(unsigned*)(out + m * N + c) = d;
    }
  }
}
__device__ __forceinline__ v4i ld16(const int8_t* p) {  // 16 bytes, any 4-byte alignment
  v4i v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// variant A: K <= 256: the activations of 16*MS pixels stay in registers while the wave walks over the channel blocks
template <int KS, int MS>
__global__ __launch_bounds__(256) void pw_a_kernel(const int8_t* __restrict__ x, const v4i* __restrict__ wp, Epi e, ResArgs ra,
                                                   int8_t* __restrict__ out, long M, int K, int N, int NB,
                                                   int nb_per_y) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const long m0 = ((long)blockIdx.x * 4 + wave) * (16 * MS);
  if (m0 >= M) return;
  v4i a[MS][KS];
#pragma unroll
  for (int ms = 0; ms < MS; ms++) {
    long m = min(m0 + 16 * ms + r, M - 1);
    const int8_t* p = x + m * K + 16 * g;
#pragma unroll
    for (int ks = 0; ks < KS; ks++) a[ms][ks] = ld16(p + 64 * ks);
  }
  const int nb0 = blockIdx.y * nb_per_y, nb1 = min(nb0 + nb_per_y, NB);
  for (int nb = nb0; nb < nb1; nb++) {
    v4i acc[MS][4];
#pragma unroll
    for (int ms = 0; ms < MS; ms++)
#pragma unroll
      for (int t = 0; t < 4; t++) acc[ms][t] = (v4i){0, 0, 0, 0};
    const v4i* w = wp + (long)nb * KS * 4 * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < KS; ks++)
#pragma unroll
      for (int t = 0; t < 4; t++) {
        v4i wv = w[(ks * 4 + t) * 64];
#pragma unroll
        for (int ms = 0; ms < MS; ms++)
          acc[ms][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv, a[ms][ks], acc[ms][t], 0, 0, 0);
      }
#pragma unroll
    for (int ms = 0; ms < MS; ms++) {
      long m = m0 + 16 * ms + r;
      if (m < M) store_tile_r(acc[ms], e, ra, out, m, N, nb, g);
    }
  }
}

// variant B: large K, few output channels: accumulators for NBT channel blocks stay in registers
// while the wave streams the K dimension of its 16 pixels.
template <int NBT>
__global__ __launch_bounds__(256) void pw_b_kernel(const int8_t* __restrict__ x, const v4i* __restrict__ wp, Epi e, ResArgs ra,
                                                   int8_t* __restrict__ out, long M, int K, int KS, int N, int NB) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const long m0 = ((long)blockIdx.x * 4 + wave) * 16;
  if (m0 >= M) return;
  const int nb0 = blockIdx.y * NBT;
  v4i acc[NBT][4];
#pragma unroll
  for (int i = 0; i < NBT; i++)
#pragma unroll
    for (int t = 0; t < 4; t++) acc[i][t] = (v4i){0, 0, 0, 0};
  const int8_t* p = x + min(m0 + r, M - 1) * K + 16 * g;
  EpiRegs er[NBT];
#pragma unroll
  for (int i = 0; i < NBT; i++) load_epi(er[i], e, ra, min(m0 + r, M - 1), N, min(nb0 + i, NB - 1), g);
#pragma unroll 4
  for (int ks = 0; ks < KS; ks++) {  // unrolled so that the loads of several k-steps are in flight together
    v4i av = ld16(p + 64 * ks);
#pragma unroll
    for (int i = 0; i < NBT; i++) {
      int nb = min(nb0 + i, NB - 1);
      const v4i* w = wp + ((long)(nb * KS + ks) * 4) * 64 + lane;
#pragma unroll
      for (int t = 0; t < 4; t++) acc[i][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w[t * 64], av, acc[i][t], 0, 0, 0);
    }
  }
  long m = m0 + r;
  if (m < M) {
#pragma unroll
    for (int i = 0; i < NBT; i++)
      if (nb0 + i < NB) store_tile_e(acc[i], er[i], e, ra, out, m, N, nb0 + i, g);
  }
}

// variant C: large K on FEW pixels (low-resolution project convs): the 4 waves of a workgroup share the same
// 16 pixels and split K in four; partial accumulators meet in LDS, then each wave requantises one 16-channel
// tile of every 64-channel block.  Quarter-length serial K loop, 4x the workgroups of variant B.
template <int NBT, int MS>
__global__ __launch_bounds__(256) void pw_c_kernel(const int8_t* __restrict__ x, const v4i* __restrict__ wp, Epi e, ResArgs ra,
                                                   int8_t* __restrict__ out, long M, int K, int KS, int N, int NB) {
  // MS pixel groups per workgroup share every weight operand a wave loads: the weights are 4/5 of the bytes this kernel pulls
  // through L1 (4 KB of weights against 1 KB of activations per K-step and pixel group), and L1 is what it saturates
  __shared__ v4i red[4][MS * NBT * 4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const long m0 = (long)blockIdx.x * (16 * MS);
  const int nb0 = blockIdx.y * NBT;
  v4i acc[MS][NBT][4];
#pragma unroll
  for (int s = 0; s < MS; s++)
#pragma unroll
    for (int i = 0; i < NBT; i++)
#pragma unroll
      for (int t = 0; t < 4; t++) acc[s][i][t] = (v4i){0, 0, 0, 0};
  const int8_t* p[MS];
#pragma unroll
  for (int s = 0; s < MS; s++) p[s] = x + min(m0 + 16 * s + r, M - 1) * K + 16 * g;
  // this wave's epilogue operands (tile t = wave of every block), requested before the K loop
  int4 eb[NBT];
  float4 em[NBT];
  unsigned eres[MS][NBT];
#pragma unroll
  for (int i = 0; i < NBT; i++) {
    const int c0 = min((nb0 + i) * 64 + 16 * g + 4 * wave, NB * 64 - 4);
    eb[i] = *(const int4*)(e.bias + c0);
    em[i] = *(const float4*)(e.mult + c0);
#pragma unroll
    for (int s = 0; s < MS; s++)
      eres[s][i] = (ra.res && (N & 3) == 0 && c0 < N) ? *(const unsigned*)(ra.res + min(m0 + 16 * s + r, M - 1) * N + c0) : 0u;
  }
  const int per = (KS + 3) >> 2;
  const int k0 = wave * per, k1 = min(k0 + per, KS);
#pragma unroll 3
  for (int ks = k0; ks < k1; ks++) {
    v4i av[MS];
#pragma unroll
    for (int s = 0; s < MS; s++) av[s] = ld16(p[s] + 64 * ks);
#pragma unroll
    for (int i = 0; i < NBT; i++) {
      int nb = min(nb0 + i, NB - 1);
      const v4i* w = wp + ((long)(nb * KS + ks) * 4) * 64 + lane;
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const v4i wv = w[t * 64];
#pragma unroll
        for (int s = 0; s < MS; s++) acc[s][i][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv, av[s], acc[s][i][t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < MS; s++)
#pragma unroll
    for (int i = 0; i < NBT; i++)
#pragma unroll
      for (int t = 0; t < 4; t++) red[wave][(s * NBT + i) * 4 + t][lane] = acc[s][i][t];
  __syncthreads();
  // wave w finishes tile t = w of every block: lane -> 4 channels (64 nb + 16 g + 4 t + j) of pixel r
#pragma unroll
  for (int s = 0; s < MS; s++) {
    const long m = m0 + 16 * s + r;
#pragma unroll
    for (int i = 0; i < NBT; i++) {
      const int nb = nb0 + i, t = wave;
      const int c0 = nb * 64 + 16 * g + 4 * t;
      if (nb < NB && c0 < N && m < M) {
        v4i sum = red[0][(s * NBT + i) * 4 + t][lane];
#pragma unroll
        for (int w2 = 1; w2 < 4; w2++) {
          v4i o = red[w2][(s * NBT + i) * 4 + t][lane];
          sum[0] += o[0]; sum[1] += o[1]; sum[2] += o[2]; sum[3] += o[3];
        }
        unsigned d = rq_pack_i(sum, eb[i], em[i], e.rq);
        if (ra.res && (N & 3) == 0) d = addq4(d, eres[s][i], ra.q);
        int8_t* o = out + m * N + c0;
        if ((N & 3) == 0) *(unsigned*)o = d;
        else
          for (int j = 0; j < 4; j++)
            if (c0 + j < N) o[j] = (int8_t)(d >> (8 * j));
      }
    }
  }
}

// variant D: large K, weights shared through LDS.  A workgroup owns 64 * MS pixels x one 64-channel block over the whole K; per
// K-step each wave fetches ONE 16-byte weight operand per lane (a quarter of the block's 4 KB) into a double-buffered LDS copy and
// its own MS activation operands into registers, a step ahead, then reads the four weight tiles back from LDS (256 B/clk/CU
// against the 64 B/clk of the vector-memory path) for 4 * MS MFMAs.  Variants B and C pull every weight operand through the
// vector-memory path once per wave - 4 loads of 1 KB per K-step and wave, 16 address cycles each on the CU's one address unit -
// which is what they saturate (tools/probes: MFMA 5 % busy, three quarters of the wave-cycles waiting).  One barrier per K-step;
// no load is issued under a condition (the prefetch index is clamped) so that the compiler's vmcnt waits stay exact.
template <int MS>
__global__ __launch_bounds__(256) void pw_d_kernel(const int8_t* __restrict__ x, const v4i* __restrict__ wp, Epi e, ResArgs ra,
                                                   int8_t* __restrict__ out, long M, int K, int KS, int N, int NB) {
  __shared__ v4i wbuf[2][4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const long m0 = ((long)blockIdx.x * 4 + wave) * (16 * MS);
  const int nb = blockIdx.y;
  const int8_t* p[MS];
  EpiRegs er[MS];
#pragma unroll
  for (int s = 0; s < MS; s++) {
    const long mc = min(m0 + 16 * s + r, M - 1);
    p[s] = x + mc * K + 16 * g;
    load_epi(er[s], e, ra, mc, N, nb, g);
  }
  v4i acc[MS][4];
#pragma unroll
  for (int s = 0; s < MS; s++)
#pragma unroll
    for (int t = 0; t < 4; t++) acc[s][t] = (v4i){0, 0, 0, 0};
  const v4i* w = wp + ((long)nb * KS * 4 + wave) * 64 + lane;   // this wave's tile of K-step 0; a K-step is 4 * 64 operands further
  v4i wreg = w[0];
  v4i a_cur[MS], a_nxt[MS];
#pragma unroll
  for (int s = 0; s < MS; s++) a_cur[s] = ld16(p[s]);
  wbuf[0][wave][lane] = wreg;
  __syncthreads();
  for (int ks = 0; ks < KS; ks++) {
    const int kn = min(ks + 1, KS - 1);
    wreg = w[(long)kn * 4 * 64];
#pragma unroll
    for (int s = 0; s < MS; s++) a_nxt[s] = ld16(p[s] + 64 * kn);
    asm volatile("" ::: "memory");
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const v4i wv = wbuf[ks & 1][t][lane];
#pragma unroll
      for (int s = 0; s < MS; s++) acc[s][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv, a_cur[s], acc[s][t], 0, 0, 0);
    }
    wbuf[(ks + 1) & 1][wave][lane] = wreg;
#pragma unroll
    for (int s = 0; s < MS; s++) a_cur[s] = a_nxt[s];
    __syncthreads();
  }
#pragma unroll
  for (int s = 0; s < MS; s++) {
    const long m = m0 + 16 * s + r;
    if (m < M) store_tile_e(acc[s], er[s], e, ra, out, m, N, nb, g);
  }
}

// variant E: the whole weight panel of the workgroup's 64-channel block - KS x 4 KB, 44 KB for K = 672, 72 KB for K = 1152 - goes to LDS ONCE, with
// every load of a thread in flight together, then ONE barrier; the K loop has no barrier at all: per step a wave reads its four weight tiles from
// LDS (4 x 1 KB at 128 B/clk) and issues 4 x MS MFMAs, with the activation operands PD steps ahead in registers.  Variant D meets at a
// workgroup barrier once per K-step - 11 to 18 times per launch, four waves each time - and with one to three workgroups per CU nothing fills
// those waits (rocprofv3: 9-10 us per launch for 2-4 GOP, the matrix pipe 5 % busy).  Measured (profiles/r05_ab.md 6): per launch the 20 x 20
// projections gain 0-1.5 us and the 10 x 10 ones lose 2 us when timed alone, yet with three forwards in flight the plan that runs b6-b15 on this
// variant is +0.6 % end to end in every round of the A/B - so the plan uses it, and the launches' 10 us are not their K loop (a variant that kept
// the barrier but requested its loads four steps ahead measured the same).
template <int MS, int PD>
__global__ __launch_bounds__(256) void pw_e_kernel(const int8_t* __restrict__ x, const v4i* __restrict__ wp, Epi e, ResArgs ra,
                                                   int8_t* __restrict__ out, long M, int K, int KS, int N, int NB) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pwe_smem[];
  v4i* wpanel = (v4i*)pwe_smem;   // [KS][4][64]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, g = lane >> 4;
  const long m0 = ((long)blockIdx.x * 4 + wave) * (16 * MS);
  const int nb = blockIdx.y;
  // 1. the panel: KS x 256 operands of 16 bytes, thread t takes t, t + 256, ... - six at a time in flight
  const v4i* wsrc = wp + (long)nb * KS * 4 * 64;
  const int total = KS * 256;
  for (int i0 = tid; i0 < total; i0 += 6 * 256) {
    v4i v[6];
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = wsrc[min(i0 + k * 256, total - 1)];
#pragma unroll
    for (int k = 0; k < 6; k++)
      if (i0 + k * 256 < total) wpanel[i0 + k * 256] = v[k];
  }
  // 2. this wave's epilogue operands and the first PD activation operands, requested before the barrier
  const int8_t* p[MS];
  EpiRegs er[MS];
#pragma unroll
  for (int s = 0; s < MS; s++) {
    const long mc = min(m0 + 16 * s + r, M - 1);
    p[s] = x + mc * K + 16 * g;
    load_epi(er[s], e, ra, mc, N, nb, g);
  }
  v4i aq[PD][MS];
#pragma unroll
  for (int i = 0; i < PD; i++) {
    const int kn = min(i, KS - 1);
#pragma unroll
    for (int s = 0; s < MS; s++) aq[i][s] = ld16(p[s] + 64 * kn);
  }
  v4i acc[MS][4];
#pragma unroll
  for (int s = 0; s < MS; s++)
#pragma unroll
    for (int t = 0; t < 4; t++) acc[s][t] = (v4i){0, 0, 0, 0};
  __syncthreads();
  // 3. the K loop: no barrier
  const v4i* wl = wpanel + lane;
  for (int ks0 = 0; ks0 < KS; ks0 += PD) {
#pragma unroll
    for (int j = 0; j < PD; j++) {
      const int ks = ks0 + j;
      if (ks < KS) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
          const v4i wv = wl[(ks * 4 + t) * 64];
#pragma unroll
          for (int s = 0; s < MS; s++) acc[s][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv, aq[j][s], acc[s][t], 0, 0, 0);
        }
      }
      const int kn = min(ks + PD, KS - 1);
#pragma unroll
      for (int s = 0; s < MS; s++) aq[j][s] = ld16(p[s] + 64 * kn);
    }
  }
#pragma unroll
  for (int s = 0; s < MS; s++) {
    const long m = m0 + 16 * s + r;
    if (m < M) store_tile_e(acc[s], er[s], e, ra, out, m, N, nb, g);
  }
}

// variant F: large K, a workgroup owns its 64 * MS pixels for ALL NB output blocks, so every activation byte is fetched once (variants D and E
// fetch the [M][K] tensor once per 64-channel block, a whole sweep apart in time).  Per K-step the 4 * NB weight tiles (NB x 4 KB) go through a
// double-buffered LDS copy: every thread requests NB 16-byte operands (its wave's tile of every block) TWO steps ahead into registers and stores
// the set requested one step earlier, so a weight load has a whole K-step of MFMAs to arrive in; the activation operands are PD steps ahead in
// registers as in variant E, refilled two steps at a time (PD is even).  One barrier per K-step, between which a wave issues 4 * NB * MS MFMAs (variant D: 4 * MS).  No load is issued
// under a condition (clamped indices), so the compiler's vmcnt waits stay exact; the loop runs KS rounded up to PD steps and only the MFMAs of
// the steps past KS are skipped.  With the packed layout [nb][ks][t][lane] a tile holds channels 16 (i >> 2) + 4 t + (i & 3) of its block, so
// a part-filled last block (N = 80, 112) has four part-filled tiles and no dead one: all 4 * NB tiles are multiplied.
// The epilogue operands are loaded after the K loop, block by block: they would otherwise hold 12 * NB * MS registers through it.
// NTL > 0 (variants 9 / 10): wp is pack_weights64_tail's panel - the part-filled last block holds NTL tile-major tiles (channels 16 t + i on
// row i of tile t) instead of four part-filled ones.  Waves >= NTL request and stage nothing for that block, a K-step multiplies
// 4 (NB - 1) + NTL tiles, and the epilogue requantises NTL tiles of the block, one dword (channels 16 t + 4 g .. + 3) per lane and tile.
template <int NB, int MS, int PD, int NTL = 0>
__global__ __launch_bounds__(256) void pw_f_kernel(const int8_t* __restrict__ x, const v4i* __restrict__ wp, Epi e, ResArgs ra,
                                                   int8_t* __restrict__ out, long M, int K, int KS, int N, int /*NB*/) {
  static_assert(PD % 2 == 0, "the activation queue is refilled in pairs of K-steps");
  static_assert(NTL >= 0 && NTL <= 4 && (NTL == 0 || NB >= 2), "a tile-major last block holds one to four tiles");
  constexpr int NBW = NTL ? NB - 1 : NB;    // blocks of four tiles
  constexpr int NTT = 4 * NBW + NTL;        // tiles per K-step
  __shared__ v4i wbuf[2][NTT][64];
  const int wave = NTL ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool tail_w = wave < NTL;           // this wave stages a tile of the tile-major last block (wave-uniform)
  const int r = lane & 15, g = lane >> 4;
  const long m0 = ((long)blockIdx.x * 4 + wave) * (16 * MS);
  const int8_t* p[MS];
#pragma unroll
  for (int s = 0; s < MS; s++) p[s] = x + min(m0 + 16 * s + r, M - 1) * K + 16 * g;
  const v4i* w = wp + wave * 64 + lane;   // this wave's tile of block 0, K-step 0; a K-step is 4 * 64 operands further, a block KS K-steps
  const long wblk = (long)KS * 4 * 64;
  const v4i* wt = wp + NBW * wblk + wave * 64 + lane;   // NTL: this wave's tile of the last block; a K-step is NTL * 64 operands further
  v4i wst[NB], wnx[NB];   // the weight operands of the next K-step (stored to LDS at the end of this one) and of the one after it
#pragma unroll
  for (int b = 0; b < NBW; b++) wst[b] = w[b * wblk];
  const int k1 = min(1, KS - 1);
#pragma unroll
  for (int b = 0; b < NBW; b++) wnx[b] = w[b * wblk + (long)k1 * 4 * 64];
  if constexpr (NTL > 0) {
    wst[NBW] = wnx[NBW] = (v4i){0, 0, 0, 0};
    if (tail_w) { wst[NBW] = wt[0]; wnx[NBW] = wt[(long)k1 * NTL * 64]; }
  }
  v4i aq[PD][MS];
#pragma unroll
  for (int i = 0; i < PD; i++) {
    const int kn = min(i, KS - 1);
#pragma unroll
    for (int s = 0; s < MS; s++) aq[i][s] = ld16(p[s] + 64 * kn);
  }
  v4i acc[MS][NB][4];
#pragma unroll
  for (int s = 0; s < MS; s++)
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
      for (int t = 0; t < 4; t++) acc[s][b][t] = (v4i){0, 0, 0, 0};
#pragma unroll
  for (int b = 0; b < NBW; b++) wbuf[0][b * 4 + wave][lane] = wst[b];
  if constexpr (NTL > 0) { if (tail_w) wbuf[0][4 * NBW + wave][lane] = wst[NBW]; }
#pragma unroll
  for (int b = 0; b < NB; b++) wst[b] = wnx[b];
  __syncthreads();
  for (int ks0 = 0; ks0 < KS; ks0 += PD) {
#pragma unroll
    for (int j = 0; j < PD; j++) {
      const int ks = ks0 + j;
      const int kw = min(ks + 2, KS - 1);
#pragma unroll
      for (int b = 0; b < NBW; b++) wnx[b] = w[b * wblk + (long)kw * 4 * 64];
      if constexpr (NTL > 0) { if (tail_w) wnx[NBW] = wt[(long)kw * NTL * 64]; }
      asm volatile("" ::: "memory");
      if (ks < KS) {
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
          for (int t = 0; t < (b < NBW ? 4 : NTL); t++) {
            const v4i wv = wbuf[ks & 1][b * 4 + t][lane];
#pragma unroll
            for (int s = 0; s < MS; s++) acc[s][b][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv, aq[j][s], acc[s][b][t], 0, 0, 0);
          }
      }
      if (j & 1) {   // two K-steps of a pixel are one 128-byte line (where its row starts on one): both halves requested together
        const int kn0 = min(ks - 1 + PD, KS - 1), kn = min(ks + PD, KS - 1);
#pragma unroll
        for (int s = 0; s < MS; s++) { aq[j - 1][s] = ld16(p[s] + 64 * kn0); aq[j][s] = ld16(p[s] + 64 * kn); }
      }
#pragma unroll
      for (int b = 0; b < NBW; b++) wbuf[(ks + 1) & 1][b * 4 + wave][lane] = wst[b];
      if constexpr (NTL > 0) { if (tail_w) wbuf[(ks + 1) & 1][4 * NBW + wave][lane] = wst[NBW]; }
#pragma unroll
      for (int b = 0; b < NB; b++) wst[b] = wnx[b];
      __syncthreads();
    }
  }
#pragma unroll
  for (int b = 0; b < NBW; b++)
#pragma unroll
    for (int s = 0; s < MS; s++) {
      const long m = m0 + 16 * s + r;
      EpiRegs er;
      load_epi(er, e, ra, min(m, M - 1), N, b, g);
      if (m < M) store_tile_e(acc[s][b], er, e, ra, out, m, N, b, g);
    }
  if constexpr (NTL > 0) {
#pragma unroll
    for (int s = 0; s < MS; s++) {
      const long m = m0 + 16 * s + r;
      if (m < M) store_tail_tiles<NTL>(acc[s][NBW], e, ra, out, m, N, NBW, g);
    }
  }
}

// ------------------------------------------------------------------------------------------
// Several independent pointwise convs in ONE launch: the 1x1 "lateral" convs the first BiFPN cell applies to the backbone outputs
// (P3 x 1, P4 x 2, P5 x 2) and the P6 conv read nothing but backbone tensors, so they need not wait for each other or for the
// nodes before them - as six launches of 5-11 us they were head and tail of a 3 us kernel each (and six of the 65 launches of
// a batch-1 forward).  A workgroup = 64 pixels x one 64-channel block of one problem, K streamed as in variant B.
// The P6 problem can carry the two 3x3/2 max pools that follow it (P6 = pool(conv(P5)), P7 = pool(P6)): then one workgroup owns one
// image, keeps the conv output in LDS and writes all three tensors.  (PwProb, PwMulti: op_args.h.)
// ------------------------------------------------------------------------------------------

// 3x3 stride-2 max pool of an int8 [H][W][N] map held in LDS (N % 4 == 0), out-of-map taps skipped (SAME): -> global + optional LDS copy
__device__ __forceinline__ void pwm_pool(const unsigned char* src, int H, int W, int N, int OH, int OW, int pt, int pl, int8_t* gout,
                                         unsigned char* lout, int tid) {
  const int N4 = N >> 2, total = OH * OW * N4;
  const float rcp_n4 = frcp(N4), rcp_ow = frcp(OW);
  for (int i = tid; i < total; i += 256) {
    const int pix = fdiv_small(i, rcp_n4), c4 = i - pix * N4;
    const int oy = fdiv_small(pix, rcp_ow), ox = pix - oy * OW;
    unsigned best = 0x80808080u;
#pragma unroll
    for (int ky = 0; ky < 3; ky++) {
      const int iy = oy * 2 + ky - pt;
#pragma unroll
      for (int kx = 0; kx < 3; kx++) {
        const int ix = ox * 2 + kx - pl;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) best = max4_s8(best, *(const unsigned*)(src + (iy * W + ix) * N + 4 * c4));
      }
    }
    *(unsigned*)(gout + (long)pix * N + 4 * c4) = best;
    if (lout) *(unsigned*)(lout + pix * N + 4 * c4) = best;
  }
}

__global__ __launch_bounds__(256) void pw_multi_kernel(PwMulti pm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pwm_smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  int pi = 0;
#pragma unroll
  for (int i = 1; i < PW_MERGE_MAX; i++) pi += (i < pm.n && (int)blockIdx.x >= pm.start[i]) ? 1 : 0;
  const PwProb& q = pm.p[pi];
  const int local = blockIdx.x - pm.start[pi];
  const Epi e{q.bias, q.mult, 0, 0, 0, q.rq};
  const ResArgs ra{nullptr, AddQ{0, 0, 0, 0, 0, 0, 0}};
  if (q.pool1 == nullptr) {
    const int nb = local % q.NB;
    const long m0 = ((long)(local / q.NB) * 4 + wave) * 16;
    if (m0 >= q.M) return;
    const long m = min(m0 + r, (long)q.M - 1);
    const int8_t* px = q.x + m * q.K + 16 * g;
    EpiRegs er;
    load_epi(er, e, ra, m, q.N, nb, g);
    v4i acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = (v4i){0, 0, 0, 0};
    const v4i* w = q.wp + (long)nb * q.KS * 4 * 64 + lane;
#pragma unroll 4
    for (int ks = 0; ks < q.KS; ks++) {
      const v4i av = ld16(px + 64 * ks);
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w[(ks * 4 + t) * 64], av, acc[t], 0, 0, 0);
    }
    if (m0 + r < q.M) store_tile_e(acc, er, e, ra, q.out, m0 + r, q.N, nb, g);
    return;
  }
  // chain: image `local`; conv output kept in LDS for the two pools
  const int HW = q.H * q.W, N = q.N;
  unsigned char* L0 = pwm_smem;                               // [HW][N]
  unsigned char* L1 = L0 + ((HW * N + 15) & ~15);             // [H1 * W1][N]
  const int8_t* xb = q.x + (long)local * HW * q.K;
  int8_t* ob = q.out + (long)local * HW * N;
  const int npg = (HW + 15) >> 4;
  for (int u = wave; u < npg * q.NB; u += 4) {
    const int pg = u / q.NB, nb = u - pg * q.NB;
    const int m = min(16 * pg + r, HW - 1);
    const int8_t* px = xb + (long)m * q.K + 16 * g;
    EpiRegs er;
    load_epi(er, e, ra, m, N, nb, g);
    v4i acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = (v4i){0, 0, 0, 0};
    const v4i* w = q.wp + (long)nb * q.KS * 4 * 64 + lane;
#pragma unroll 4
    for (int ks = 0; ks < q.KS; ks++) {
      const v4i av = ld16(px + 64 * ks);
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w[(ks * 4 + t) * 64], av, acc[t], 0, 0, 0);
    }
    const int c0 = nb * 64 + 16 * g;
    if (16 * pg + r < HW && c0 < N) {     // N % 16 == 0 (checked by the planner): a lane's 16 channels are all real
      const uint4 d = make_uint4(rq_pack_i(acc[0], er.b[0], er.mu[0], e.rq), rq_pack_i(acc[1], er.b[1], er.mu[1], e.rq),
                                 rq_pack_i(acc[2], er.b[2], er.mu[2], e.rq), rq_pack_i(acc[3], er.b[3], er.mu[3], e.rq));
      *(uint4*)(ob + (long)m * N + c0) = d;
      *(uint4*)(L0 + m * N + c0) = d;
    }
  }
  __syncthreads();
  pwm_pool(L0, q.H, q.W, N, q.H1, q.W1, q.pt1, q.pl1, q.pool1 + (long)local * q.H1 * q.W1 * N, L1, tid);
  __syncthreads();
  pwm_pool(L1, q.H1, q.W1, N, q.H2, q.W2, q.pt2, q.pl2, q.pool2 + (long)local * q.H2 * q.W2 * N, nullptr, tid);
}

// ---- launchers: the instantiation PwKernel names, one launch on st ----
int launch_pw(const PwArgs& a, const PwKernel& k, dim3 grid, int lds_bytes, hipStream_t st) {
  const bool built = (k.ms == 1 || k.ms == 2) &&
                     (k.form == PW_A   ? a.KS64 >= 1 && a.KS64 <= 4
                      : k.form == PW_B ? k.nbt >= 1 && k.nbt <= 4
                      : k.form == PW_F ? a.NB >= 2 && a.NB <= PW_F_MAX_NB && (k.ntl == 0 || pw_f_tail_built(a.NB, k.ntl))
                                       : true);
  if (!built) {
    set_error("pw_conv: no kernel of form %d for %d K-steps, %d output blocks (%d tail tiles), ms %d, nbt %d", (int)k.form, a.KS64, a.NB, k.ntl, k.ms, k.nbt);
    return VBT_ERR_ARG;
  }
#define PW(KERNEL, LDS) KERNEL<<<grid, 256, LDS, st>>>(a.x, a.wp, a.e, a.ra, a.out, a.M, a.K, a.KS64, a.N, a.NB)
#define PW_A(KS) (k.ms == 2 ? pw_a_kernel<KS, 2><<<grid, 256, 0, st>>>(a.x, a.wp, a.e, a.ra, a.out, a.M, a.K, a.N, a.NB, a.nb_per_y) \
                            : pw_a_kernel<KS, 1><<<grid, 256, 0, st>>>(a.x, a.wp, a.e, a.ra, a.out, a.M, a.K, a.N, a.NB, a.nb_per_y))
#define PW_F_NB(NBF) (k.ms == 2 ? PW((pw_f_kernel<NBF, 2, 4>), 0) : PW((pw_f_kernel<NBF, 1, 4>), 0))
#define PW_F_TAIL(NBF, NTL) (k.ms == 2 ? PW((pw_f_kernel<NBF, 2, 4, NTL>), 0) : PW((pw_f_kernel<NBF, 1, 4, NTL>), 0))
  switch (k.form) {
    case PW_A: if (a.KS64 == 1) PW_A(1); else if (a.KS64 == 2) PW_A(2); else if (a.KS64 == 3) PW_A(3); else PW_A(4); break;
    case PW_D: if (k.ms == 2) PW(pw_d_kernel<2>, 0); else PW(pw_d_kernel<1>, 0); break;
    case PW_C: if (k.ms == 2) PW((pw_c_kernel<1, 2>), 0); else PW((pw_c_kernel<1, 1>), 0); break;
    case PW_E:
      if (k.ms == 2) { if (lds_bytes > 64 * 1024) VBT_LDS_OPT_IN(pw_e_kernel<2, 4>); PW((pw_e_kernel<2, 4>), lds_bytes); }
      else { if (lds_bytes > 64 * 1024) VBT_LDS_OPT_IN(pw_e_kernel<1, 4>); PW((pw_e_kernel<1, 4>), lds_bytes); }
      break;
    case PW_F:
      if (k.ntl) {   // the pairs of pw_f_tail_built (op_args.h)
        if (a.NB == 2 && k.ntl == 1) PW_F_TAIL(2, 1); else if (a.NB == 2 && k.ntl == 2) PW_F_TAIL(2, 2); else if (a.NB == 2 && k.ntl == 3) PW_F_TAIL(2, 3);
        else if (a.NB == 2) PW_F_TAIL(2, 4); else if (a.NB == 4) PW_F_TAIL(4, 1); else PW_F_TAIL(6, 2);
      }
      else if (a.NB == 2) PW_F_NB(2); else if (a.NB == 3) PW_F_NB(3); else if (a.NB == 4) PW_F_NB(4); else if (a.NB == 5) PW_F_NB(5); else PW_F_NB(6);
      break;
    case PW_B:
      if (k.nbt == 1) PW(pw_b_kernel<1>, 0); else if (k.nbt == 2) PW(pw_b_kernel<2>, 0); else if (k.nbt == 3) PW(pw_b_kernel<3>, 0); else PW(pw_b_kernel<4>, 0);
      break;
  }
#undef PW_F_TAIL
#undef PW_F_NB
#undef PW_A
#undef PW
  return VBT_OK;
}

int launch_pw_multi(const PwMulti& pm, unsigned grid, int lds_bytes, hipStream_t st) {
  if (pm.n < 1 || pm.n > PW_MERGE_MAX) { set_error("pw_multi: %d convs in one launch, it takes 1 to %d", pm.n, PW_MERGE_MAX); return VBT_ERR_ARG; }
  pw_multi_kernel<<<dim3(grid), 256, lds_bytes, st>>>(pm);
  return VBT_OK;
}

}  // namespace vbt
