// The small single-op kernels of the int8 detector, one graph op per launch: stem conv, depthwise convs (row / column walkers), integer
// ADD, max pool, nearest-neighbour resize - and their launchers (launchers.h; argument structs: op_args.h).  The only unit that sees
// these kernels.
#include "launchers.h"
#include "dev_common.h"

namespace vbt {

// ------------------------------------------------------------------------------------------
// stem: 3x3 stride-2 conv on the uint8 frame as one 16x16x32 MFMA K-step.  The 27 taps are
// laid out per lane group g: g<3 -> the first 8 bytes (px0 RGB, px1 RGB, px2 RG) of kernel row g,
// g==3 -> the B byte of px2 of rows 0..2 (+5 zero weights).  QUANTIZE u8 -> s8 is the XOR 0x80.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stem_kernel(const uint8_t* __restrict__ frames, const long* __restrict__ wp, Epi e,
                                                   int8_t* __restrict__ out, long M, int H, int W, int OH, int OW,
                                                   int N, int pad_t, int pad_l, int zx) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const long m0 = ((long)blockIdx.x * 4 + wave) * 16;
  if (m0 >= M) return;
  long m = min(m0 + r, M - 1);
  int ox = (int)(m % OW);
  long t = m / OW;
  int oy = (int)(t % OH);
  long b = t / OH;
  const uint8_t* f = frames + b * (long)H * W * 3;
  const int ix0 = 2 * ox - pad_l, iy0 = 2 * oy - pad_t;
  const unsigned padb = (unsigned)(zx & 255);
  unsigned char by[8];
  if (g < 3) {
    int iy = iy0 + g;
    bool rowok = iy >= 0 && iy < H;
    if (rowok && ix0 >= 0 && ix0 + 2 < W) {
      unsigned long long v;
      __builtin_memcpy(&v, f + ((long)iy * W + ix0) * 3, 8);
      v ^= 0x8080808080808080ull;
      __builtin_memcpy(by, &v, 8);
    } else {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        int ix = ix0 + j / 3;
        bool ok = rowok && ix >= 0 && ix < W;
        by[j] = ok ? (unsigned char)(f[((long)iy * W + ix) * 3 + j % 3] ^ 0x80) : (unsigned char)padb;
      }
    }
  } else {
    int ix = ix0 + 2;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      int iy = iy0 + j;
      bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
      by[j] = ok ? (unsigned char)(f[((long)iy * W + ix) * 3 + 2] ^ 0x80) : (unsigned char)padb;
    }
#pragma unroll
    for (int j = 3; j < 8; j++) by[j] = 0;
  }
  long av;
  __builtin_memcpy(&av, by, 8);
  v4i acc[4];
#pragma unroll
  for (int t4 = 0; t4 < 4; t4++) {
    acc[t4] = (v4i){0, 0, 0, 0};
    acc[t4] = __builtin_amdgcn_mfma_i32_16x16x32_i8(wp[t4 * 64 + lane], av, acc[t4], 0, 0, 0);
  }
  if (m0 + r < M) store_tile(acc, e, out, m, N, 0, g);
}

// ------------------------------------------------------------------------------------------
// depthwise conv: lane = 4 channels x R=4 consecutive output columns.
// acc = sum u*w with u = x_q + 128 (cvt_f32_ubyte), exact in fp32; folded bias restores (x_q - z_x).
// ------------------------------------------------------------------------------------------
template <int KK, int S>
__global__ __launch_bounds__(256) void dw_kernel(const int8_t* __restrict__ x, const float* __restrict__ wf, Epi e,
                                                 int8_t* __restrict__ out, long total, int H, int W, int C, int OH,
                                                 int OW, int pad_t, int pad_l, unsigned pad4) {
  constexpr int R = 4;
  constexpr int IW = S * (R - 1) + KK;
  long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int C4 = C >> 2;
  const int XR = (OW + R - 1) / R;
  int c4 = (int)(idx % C4);
  long t = idx / C4;
  int xr = (int)(t % XR);
  t /= XR;
  int oy = (int)(t % OH);
  long b = t / OH;
  const int ox0 = xr * R;
  float acc[R][4];
#pragma unroll
  for (int o = 0; o < R; o++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[o][j] = 0.0f;
  const int8_t* xb = x + b * (long)H * W * C + 4 * c4;
#pragma unroll
  for (int ky = 0; ky < KK; ky++) {
    int iy = oy * S + ky - pad_t;
    bool rowok = iy >= 0 && iy < H;
    float4 wr[KK];
#pragma unroll
    for (int kx = 0; kx < KK; kx++) wr[kx] = *(const float4*)(wf + (long)(ky * KK + kx) * C + 4 * c4);
#pragma unroll
    for (int j = 0; j < IW; j++) {
      int ix = ox0 * S + j - pad_l;
      bool ok = rowok && ix >= 0 && ix < W;
      unsigned u = pad4;
      if (ok) u = *(const unsigned*)(xb + ((long)iy * W + ix) * C) ^ 0x80808080u;
      float f0 = (float)(u & 255u), f1 = (float)((u >> 8) & 255u), f2 = (float)((u >> 16) & 255u), f3 = (float)(u >> 24);
#pragma unroll
      for (int kx = 0; kx < KK; kx++) {
        if ((j - kx) >= 0 && (j - kx) % S == 0 && (j - kx) / S < R) {
          const int o = (j - kx) / S;
          acc[o][0] = __builtin_fmaf(f0, wr[kx].x, acc[o][0]);
          acc[o][1] = __builtin_fmaf(f1, wr[kx].y, acc[o][1]);
          acc[o][2] = __builtin_fmaf(f2, wr[kx].z, acc[o][2]);
          acc[o][3] = __builtin_fmaf(f3, wr[kx].w, acc[o][3]);
        }
      }
    }
  }
  int4 bq = *(const int4*)(e.bias + 4 * c4);
  float4 mu = *(const float4*)(e.mult + 4 * c4);
  int8_t* ob = out + ((b * OH + oy) * (long)OW) * C + 4 * c4;
#pragma unroll
  for (int o = 0; o < R; o++) {
    int ox = ox0 + o;
    if (ox < OW) {
      v4i ai = {(int)acc[o][0], (int)acc[o][1], (int)acc[o][2], (int)acc[o][3]};
      unsigned d = rq_pack_i(ai, bq, mu, e.rq);
      *(unsigned*)(ob + (long)ox * C) = d;
    }
  }
}

// ------------------------------------------------------------------------------------------
// depthwise conv, column walker: a lane owns 4 channels x 4 output columns and walks DOWN a segment of
// output rows.  The k*k*4 weights stay in registers for the whole walk; every input row is loaded and
// converted once and scattered into the (at most ceil(k/s)) output rows still in flight, which live in a
// statically indexed accumulator ring (the row loop is unrolled by the ring period).
// ------------------------------------------------------------------------------------------
constexpr int cmod(int a, int n) { return ((a % n) + n) % n; }
constexpr int cfloordiv(int a, int n) { return (a - cmod(a, n)) / n; }

template <int KK, int S>
__global__ __launch_bounds__(256) void dw_col_kernel(const int8_t* __restrict__ x, const float* __restrict__ wf, Epi e,
                                                     int8_t* __restrict__ out, long total, int H, int W, int C, int OH, int OW,
                                                     int pad_t, int pad_l, unsigned pad4, int rows, int nseg) {
  constexpr int IW = 3 * S + KK;
  constexpr int NS = (KK + S - 1) / S;
  constexpr int P = NS * S;
  long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int C4 = C >> 2, XR = (OW + 3) >> 2;
  const int c4 = (int)(idx % C4);
  long t = idx / C4;
  const int xr = (int)(t % XR);
  t /= XR;
  const int seg = (int)(t % nseg);
  const long b = t / nseg;
  const int oy_b = seg * rows;
  const int nrows = min(rows, OH - oy_b);
  if (nrows <= 0) return;
  const int ox0 = xr * 4;
  const int iy_b = oy_b * S - pad_t, ix_b = ox0 * S - pad_l;
  const int n_in = (nrows - 1) * S + KK;
  float4 w[KK][KK];
#pragma unroll
  for (int ky = 0; ky < KK; ky++)
#pragma unroll
    for (int kx = 0; kx < KK; kx++) w[ky][kx] = *(const float4*)(wf + (long)(ky * KK + kx) * C + 4 * c4);
  const int4 bq = *(const int4*)(e.bias + 4 * c4);
  const float4 mu = *(const float4*)(e.mult + 4 * c4);
  float acc[NS][4][4];
#pragma unroll
  for (int sl = 0; sl < NS; sl++)
#pragma unroll
    for (int o = 0; o < 4; o++)
#pragma unroll
      for (int j = 0; j < 4; j++) acc[sl][o][j] = 0.0f;
  unsigned colmask = 0;
#pragma unroll
  for (int j = 0; j < IW; j++)
    if (ix_b + j >= 0 && ix_b + j < W) colmask |= 1u << j;
  const int8_t* xb = x + b * (long)H * W * C + 4 * c4;
  int8_t* ob = out + b * (long)OH * OW * C + 4 * c4;
  for (int i0 = 0; i0 < n_in; i0 += P) {
#pragma unroll
    for (int r = 0; r < P; r++) {
      const int i = i0 + r;
      if (i >= n_in) break;
      const int iy = iy_b + i;
      const bool rowok = iy >= 0 && iy < H;
      const int8_t* rp = xb + ((long)iy * W + ix_b) * C;
      bool kyok[KK];
#pragma unroll
      for (int ky = 0; ky < KK; ky++) kyok[ky] = (i - ky) >= 0 && (i - ky) / S < nrows;
#pragma unroll
      for (int j = 0; j < IW; j++) {
        unsigned u = pad4;
        if (rowok && ((colmask >> j) & 1u)) u = *(const unsigned*)(rp + (long)j * C) ^ 0x80808080u;
        const float f0 = (float)(u & 255u), f1 = (float)((u >> 8) & 255u), f2 = (float)((u >> 16) & 255u), f3 = (float)(u >> 24);
#pragma unroll
        for (int ky = 0; ky < KK; ky++) {
          if (cmod(r - ky, S) == 0) {
            constexpr int dummy = 0;
            (void)dummy;
            const int sl = cmod(cfloordiv(r - ky, S), NS);
            if (kyok[ky]) {
#pragma unroll
              for (int kx = 0; kx < KK; kx++) {
                if ((j - kx) >= 0 && (j - kx) % S == 0 && (j - kx) / S < 4) {
                  const int o = (j - kx) / S;
                  acc[sl][o][0] = __builtin_fmaf(f0, w[ky][kx].x, acc[sl][o][0]);
                  acc[sl][o][1] = __builtin_fmaf(f1, w[ky][kx].y, acc[sl][o][1]);
                  acc[sl][o][2] = __builtin_fmaf(f2, w[ky][kx].z, acc[sl][o][2]);
                  acc[sl][o][3] = __builtin_fmaf(f3, w[ky][kx].w, acc[sl][o][3]);
                }
              }
            }
          }
        }
      }
      // the output row whose last input row this was
      if (cmod(r - (KK - 1), S) == 0) {
        const int sl = cmod(cfloordiv(r - (KK - 1), S), NS);
        const int od = (i - (KK - 1)) / S;
        if (i - (KK - 1) >= 0 && od < nrows) {
          int8_t* orow = ob + ((long)(oy_b + od) * OW) * C;
#pragma unroll
          for (int o = 0; o < 4; o++) {
            const v4i ai = {(int)acc[sl][o][0], (int)acc[sl][o][1], (int)acc[sl][o][2], (int)acc[sl][o][3]};
            if (ox0 + o < OW) *(unsigned*)(orow + (long)(ox0 + o) * C) = rq_pack_i(ai, bq, mu, e.rq);
          }
        }
#pragma unroll
        for (int o = 0; o < 4; o++)
#pragma unroll
          for (int j = 0; j < 4; j++) acc[sl][o][j] = 0.0f;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// elementwise binary int8 ADD: 16 bytes per lane
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_kernel(const int8_t* __restrict__ xa, const int8_t* __restrict__ xb, AddQ q,
                                                  int8_t* __restrict__ out, long n4) {
  long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  const bool al16 = ((((unsigned long)xa) | ((unsigned long)xb) | ((unsigned long)out)) & 15ul) == 0;   // (sub-batch offsets may break it)
  if (al16 && i + 4 <= n4) {
    const uint4 va = *(const uint4*)(xa + 4 * i), vb = *(const uint4*)(xb + 4 * i);
    *(uint4*)(out + 4 * i) = make_uint4(addq4(va.x, vb.x, q), addq4(va.y, vb.y, q), addq4(va.z, vb.z, q), addq4(va.w, vb.w, q));
  } else {
    for (long e = i + 4; i < n4 && i < e; i++) ((unsigned*)out)[i] = addq4(((const unsigned*)xa)[i], ((const unsigned*)xb)[i], q);
  }
}

__global__ __launch_bounds__(256) void maxpool_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ out, long total,
                                                      int H, int W, int C, int OH, int OW, int pad_t, int pad_l) {
  long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int C4 = C >> 2;
  int c4 = (int)(idx % C4);
  long t = idx / C4;
  int ox = (int)(t % OW);
  t /= OW;
  int oy = (int)(t % OH);
  long b = t / OH;
  unsigned best = 0x80808080u;  // -128 x4
  for (int ky = 0; ky < 3; ky++) {
    int iy = oy * 2 + ky - pad_t;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < 3; kx++) {
      int ix = ox * 2 + kx - pad_l;
      if (ix < 0 || ix >= W) continue;
      unsigned v = *(const unsigned*)(x + ((b * H + iy) * (long)W + ix) * C + 4 * c4);
      best = max4_s8(best, v);
    }
  }
  *(unsigned*)(out + ((b * OH + oy) * (long)OW + ox) * C + 4 * c4) = best;
}

__global__ __launch_bounds__(256) void resize_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ out, long total,
                                                     int H, int W, int C, int OH, int OW) {
  long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int C4 = C >> 2;
  int c4 = (int)(idx % C4);
  long t = idx / C4;
  int ox = (int)(t % OW);
  t /= OW;
  int oy = (int)(t % OH);
  long b = t / OH;
  int iy = (oy * H) / OH, ix = (ox * W) / OW;
  *(unsigned*)(out + ((b * OH + oy) * (long)OW + ox) * C + 4 * c4) =
      *(const unsigned*)(x + ((b * H + iy) * (long)W + ix) * C + 4 * c4);
}

// ---- launchers ----
int launch_stem(const StemArgs& a, hipStream_t st) {
  stem_kernel<<<dim3((unsigned)((a.M + 63) / 64)), 256, 0, st>>>(a.frames, a.wp, a.e, a.out, a.M, a.H, a.W, a.OH, a.OW, a.N, a.pad_t, a.pad_l, a.zx);
  return VBT_OK;
}

int launch_dw(const DwArgs& a, int k, int stride, dim3 grid, hipStream_t st) {
  if ((k != 3 && k != 5) || (stride != 1 && stride != 2)) { set_error("dw_conv: no kernel for %d x %d taps, stride %d", k, k, stride); return VBT_ERR_ARG; }
#define DW_LAUNCH(KK, S)                                                                                                                          \
  do {                                                                                                                                            \
    if (a.rows == 0) dw_kernel<KK, S><<<grid, 256, 0, st>>>(a.x, a.wf, a.e, a.out, a.total, a.H, a.W, a.C, a.OH, a.OW, a.pad_t, a.pad_l, a.pad4);  \
    else dw_col_kernel<KK, S><<<grid, 256, 0, st>>>(a.x, a.wf, a.e, a.out, a.total, a.H, a.W, a.C, a.OH, a.OW, a.pad_t, a.pad_l, a.pad4, a.rows,  \
                                                    a.nseg);                                                                                      \
  } while (0)
  if (k == 3 && stride == 1) DW_LAUNCH(3, 1);
  else if (k == 3 && stride == 2) DW_LAUNCH(3, 2);
  else if (k == 5 && stride == 1) DW_LAUNCH(5, 1);
  else DW_LAUNCH(5, 2);
#undef DW_LAUNCH
  return VBT_OK;
}

int launch_add(const int8_t* xa, const int8_t* xb, const AddQ& q, int8_t* out, long n4, hipStream_t st) {
  add_kernel<<<dim3((unsigned)((n4 + 1023) / 1024)), 256, 0, st>>>(xa, xb, q, out, n4);
  return VBT_OK;
}

int launch_maxpool(const MapArgs& a, hipStream_t st) {
  maxpool_kernel<<<dim3((unsigned)((a.total + 255) / 256)), 256, 0, st>>>(a.x, a.out, a.total, a.H, a.W, a.C, a.OH, a.OW, a.pad_t, a.pad_l);
  return VBT_OK;
}

int launch_resize_nn(const MapArgs& a, hipStream_t st) {
  resize_kernel<<<dim3((unsigned)((a.total + 255) / 256)), 256, 0, st>>>(a.x, a.out, a.total, a.H, a.W, a.C, a.OH, a.OW);
  return VBT_OK;
}

}  // namespace vbt
