// Fused network entry: stem 3x3/2 conv on the uint8 frame -> depthwise 3x3/1 -> project 1x1, one kernel.
//
// The two largest activation tensors of the network (stem output 160x160x32 and the first depthwise output) never
// reach HBM: a workgroup reads a 37x37 RGB patch and writes a 16x16x16 output tile.  Bit-identical to the three
// graph ops run one by one (same int32 accumulations, same float requantisation).
//
//   R  [37][120]    raw uint8 rows of the patch (dword-aligned start, out-of-image dwords = input zero point)
//   P  [336][32]    per stem pixel of the 18x18 halo: kernel row 0|1|2 as 8 bytes each (px0 RGB px1 RGB px2 RG)
//                   + the three px2-B bytes: exactly the K=32 operand of one 16x16x32 int8 MFMA
//   S  [324][48]    stem output on the halo, int8 x 32 channels (out-of-map pixels = its zero point: the
//                   depthwise pads ITS input); 48-byte rows: 16-byte aligned channel groups, conflict-free b128 reads
//   D  [256][40]    depthwise output, int8 x 32 channels
// stem / project: weights are the MFMA A operand so a lane ends with consecutive output channels of one pixel;
// depthwise: diagonal-embedded weights on the 16x16x64 MFMA, tap (row m, column g) per instruction m and lane group g
// (three instructions for 3x3, every LDS address = lane base + immediate; see DW64 in fused_block.h).
#pragma once
#include "dev_common.h"
#include "stem_block_args.h"

namespace vbt {

constexpr int SB_HW = 18, SB_NPH = SB_HW * SB_HW, SB_NPG = (SB_NPH + 15) / 16;
constexpr int SB_RROWS = 37, SB_RDW = 30, SB_RST = SB_RDW * 4, SB_PST = 32, SB_SST = 48, SB_DST = 40;

// MODE 1: all three requantisations clamp at the int8 limits (the saturating flavour, no per-element branch); MODE 3: and all
// three convs' accumulators are proven to stay inside +-2^22 (Rq::kb: accumulators start at bias + RQ_KBIAS); MODE 0: read at run time
template <int MODE>
__global__ __launch_bounds__(256) void stem_block_kernel(StemBlockArgs a) {
  constexpr int FK = MODE == 0 ? -1 : MODE;
  constexpr int KB = MODE >= 2 ? RQ_KBIAS : 0;
  // R is dead once P is built and P once S is built: R shares S's storage, D shares P's (23.8 KB -> 6 workgroups / CU)
  __shared__ __attribute__((aligned(16))) unsigned char SR[SB_NPH * SB_SST + 64];
  __shared__ __attribute__((aligned(16))) unsigned char PD[SB_NPG * 16 * SB_PST];
  static_assert(SB_RROWS * SB_RST <= SB_NPH * SB_SST && 256 * SB_DST <= SB_NPG * 16 * SB_PST, "aliased LDS regions");
  unsigned char* const R = SR;
  unsigned char* const S = SR;
  unsigned char* const P = PD;
  unsigned char* const D = PD;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x;
  const int trow = fdiv_small(tile, frcp(a.tiles_x));
  const int tx = tile - trow * a.tiles_x;
  const int bimg = fdiv_small(trow, frcp(a.tiles_y));
  const int ty = trow - bimg * a.tiles_y;
  const long b = bimg;
  const int oy0 = ty * 16, ox0 = tx * 16;
  const int sy0 = oy0 - 1, sx0 = ox0 - 1;                      // depthwise 3x3/1 SAME: one halo pixel
  const int iy0 = 2 * sy0 - a.spad_t, ix0 = 2 * sx0 - a.spad_l;
  const int rb0 = ix0 * 3;
  const int al = rb0 & 3;                                        // two's complement: also right for negative rb0
  const int rstart = rb0 - al;                                   // multiple of 4
  const int rowbytes = a.W * 3;                                  // multiple of 4 (planner)

  // ---- 1a: raw patch rows -> R (aligned dwords) ----
  {
    const uint8_t* f = a.frames + b * (long)a.H * rowbytes;
    for (int idx = tid; idx < SB_RROWS * SB_RDW; idx += 256) {
      const int row = idx / SB_RDW, d = idx - row * SB_RDW;
      const int iy = iy0 + row, off = rstart + 4 * d;
      unsigned v = a.in_pad4;
      if (iy >= 0 && iy < a.H && off >= 0 && off < rowbytes) v = *(const unsigned*)(f + (long)iy * rowbytes + off);
      *(unsigned*)(R + row * SB_RST + 4 * d) = v;
    }
  }
  __syncthreads();
  // ---- 1b: MFMA operand slots: (stem pixel, kernel row) -> 9 bytes, u8 -> s8 by XOR 0x80 ----
  for (int slot = tid; slot < SB_NPH * 3; slot += 256) {
    const int p = slot / 3, ky = slot - 3 * p;
    const int hy = p / SB_HW, hx = p - hy * SB_HW;
    const int o = al + 6 * hx;
    const unsigned char* src = R + (2 * hy + ky) * SB_RST + (o & ~3);
    const unsigned d0 = *(const unsigned*)src, d1 = *(const unsigned*)(src + 4), d2 = *(const unsigned*)(src + 8);
    const unsigned sh = (unsigned)(o & 3);
    const unsigned w0 = __builtin_amdgcn_alignbyte(d1, d0, sh) ^ 0x80808080u;
    const unsigned w1 = __builtin_amdgcn_alignbyte(d2, d1, sh) ^ 0x80808080u;
    const unsigned b8 = ((d2 >> (8 * sh)) & 255u) ^ 0x80u;
    *(uint2*)(P + p * SB_PST + 8 * ky) = make_uint2(w0, w1);
    P[p * SB_PST + 24 + ky] = (unsigned char)b8;
  }
  __syncthreads();
  // ---- 2: stem conv on the 18x18 halo, 2 MFMAs per 16 pixels (32 output channels) ----
  {
    const long wa0 = a.ws[lane], wa1 = a.ws[64 + lane];
    const int4 b0 = int4_plus(*(const int4*)(a.bs + 8 * g), KB), b1 = int4_plus(*(const int4*)(a.bs + 8 * g + 4), KB);
    const float4 m0 = *(const float4*)(a.ms + 8 * g), m1 = *(const float4*)(a.ms + 8 * g + 4);
    // halo pixels outside the stem's output map (tiles on the map border only): bit i <-> pixel group wave + 4i
    unsigned oob_mask = 0;
    if (sy0 < 0 || sx0 < 0 || sy0 + SB_HW > a.SH || sx0 + SB_HW > a.SW) {
      for (int i = 0, pg = wave; pg < SB_NPG; pg += 4, i++) {
        const int pc = min(pg * 16 + r, SB_NPH - 1);
        const int hy = pc / SB_HW, hx = pc - hy * SB_HW;
        const int sy = sy0 + hy, sx = sx0 + hx;
        if (!(sy >= 0 && sy < a.SH && sx >= 0 && sx < a.SW)) oob_mask |= 1u << i;
      }
    }
    for (int i = 0, pg = wave; pg < SB_NPG; pg += 4, i++) {
      const int p = pg * 16 + r;
      const int pc = min(p, SB_NPH - 1);
      const long bv = *(const long*)(P + pc * SB_PST + 8 * g);
      v4i a0 = v4i_from(b0), a1 = v4i_from(b1);
      a0 = __builtin_amdgcn_mfma_i32_16x16x32_i8(wa0, bv, a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_i32_16x16x32_i8(wa1, bv, a1, 0, 0, 0);
      unsigned q0 = rq_pack_b<FK>(a0, m0, a.rqs), q1 = rq_pack_b<FK>(a1, m1, a.rqs);
      if ((oob_mask >> i) & 1u) { q0 = a.zs4; q1 = a.zs4; }
      if (p < SB_NPH) *(uint2*)(S + p * SB_SST + 8 * g) = make_uint2(q0, q1);
    }
  }
  __syncthreads();
  // ---- 3: depthwise 3x3/1 on the 16x16x64 MFMA: wave -> channel group (wave & 1), output rows 8(wave>>1).. ----
  {
    const int cg = wave & 1;
    v4i wreg[3];
#pragma unroll
    for (int mi = 0; mi < 3; mi++) wreg[mi] = a.wd64[(cg * 3 + mi) * 64 + lane];
    const int4 bqm = int4_plus(*(const int4*)(a.bdm + 16 * cg + 4 * g), KB);
    const float4 mum = *(const float4*)(a.mdm + 16 * cg + 4 * g);
    // lane (r = output column, g = tap column): B operand of instruction m for output row py = 16 channels of halo pixel
    // (py + m, r + g); g = 3 carries zero weights (it reads one pixel past the window: still inside S)
    const unsigned char* lane_base = S + (r + g) * SB_SST + 16 * cg + (wave >> 1) * 8 * SB_HW * SB_SST;
#pragma unroll
    for (int i = 0; i < 8; i += 2) {   // two output rows at a time: independent accumulate chains
      v4i dqa = v4i_from(bqm), dqb = v4i_from(bqm);
#pragma unroll
      for (int mi = 0; mi < 3; mi++) {
        dqa = __builtin_amdgcn_mfma_i32_16x16x64_i8(wreg[mi], *(const v4i*)(lane_base + (i + mi) * SB_HW * SB_SST), dqa, 0, 0, 0);
        dqb = __builtin_amdgcn_mfma_i32_16x16x64_i8(wreg[mi], *(const v4i*)(lane_base + (i + 1 + mi) * SB_HW * SB_SST), dqb, 0, 0, 0);
      }
      const int py = (wave >> 1) * 8 + i;
      *(unsigned*)(D + (py * 16 + r) * SB_DST + 16 * cg + 4 * g) = rq_pack_b<FK>(dqa, mum, a.rqd);
      *(unsigned*)(D + ((py + 1) * 16 + r) * SB_DST + 16 * cg + 4 * g) = rq_pack_b<FK>(dqb, mum, a.rqd);
    }
  }
  __syncthreads();
  // ---- 4: project 32 -> Cout (<= 16): one MFMA per 16 pixels, lane -> 4 consecutive channels of pixel r ----
  {
    const long wa = a.wp[lane];
    const int4 bb = int4_plus(*(const int4*)(a.bp + 4 * g), KB);
    const float4 mm = *(const float4*)(a.mp + 4 * g);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int py = wave * 4 + i;
      const long bv = *(const long*)(D + (py * 16 + r) * SB_DST + 8 * g);
      v4i acc = v4i_from(bb);
      acc = __builtin_amdgcn_mfma_i32_16x16x32_i8(wa, bv, acc, 0, 0, 0);
      const unsigned q = rq_pack_b<FK>(acc, mm, a.rqp);
      const int oy = oy0 + py, ox = ox0 + r;
      if (oy < a.SH && ox < a.SW && 4 * g < a.Cout) *(unsigned*)(a.out + ((b * a.SH + oy) * (long)a.SW + ox) * a.Cout + 4 * g) = q;
    }
  }
}

// The direct form (plan variant 1): no im2col tile and no depthwise tile.
//   R  [37][120]    the same raw rows, already int8 (XOR 0x80 once per loaded dword; out-of-image dwords = in_pad4s)
//   S  [324][48]    as above; R and S are both live in the stem stage, so they do not share storage (20.1 KB -> 8 workgroups / CU)
// stem: the K = 27 of a halo pixel goes to one 16x16x64 MFMA as it lies in R: lane (r, g < 3) takes kernel row g of pixel r as the three
// aligned dwords that cover its 9 bytes, funnel-shifted to the pixel's first byte.  K slots 9..15 of the lane group hold the bytes
// that follow in the row (or zero), lane group 3 repeats kernel row 2: all of these meet zero weights (pack_stem_block_stem64).
// depthwise + project: wave w owns output rows 4w..4w+3 for BOTH channel groups, so lane (r, g) ends with channels 4g..4g+3 and
// 16+4g..16+4g+3 of pixel r: those two dwords are the B operand of the projection's 16x16x32 MFMA with the weights packed in that
// K order (pack_stem_block_proj_chain; the chained form of band_block.h).  Two barriers: fill | stem | depthwise + project.
// 20.1 KB of LDS admit 8 workgroups per CU; the register allocator is held to the 64 VGPRs of 8 waves per SIMD.  MODE 1 / 3 pay one
// spilled VGPR for it (one scratch store after the first barrier, one reload in the last stage); at 6 waves per SIMD nothing spills and
// the launch is 10 % slower (profiles/r11_stem_direct_ab.md section 3).
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void stem_block_direct_kernel(StemBlockArgs a) {
  constexpr int FK = MODE == 0 ? -1 : MODE;
  constexpr int KB = MODE >= 2 ? RQ_KBIAS : 0;
  __shared__ __attribute__((aligned(16))) unsigned char R[SB_RROWS * SB_RST];
  __shared__ __attribute__((aligned(16))) unsigned char S[SB_NPH * SB_SST + 64];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x;
  const int trow = fdiv_small(tile, frcp(a.tiles_x));
  const int tx = tile - trow * a.tiles_x;
  const int bimg = fdiv_small(trow, frcp(a.tiles_y));
  const int ty = trow - bimg * a.tiles_y;
  const long b = bimg;
  const int oy0 = ty * 16, ox0 = tx * 16;
  const int sy0 = oy0 - 1, sx0 = ox0 - 1;
  const int iy0 = 2 * sy0 - a.spad_t, ix0 = 2 * sx0 - a.spad_l;
  const int rb0 = ix0 * 3;
  const int al = rb0 & 3;
  const int rstart = rb0 - al;
  const int rowbytes = a.W * 3;

  // ---- 1: raw patch rows -> R, 32 lanes per row (30 live), 8 rows per round ----
  {
    const int d = tid & 31, off = rstart + 4 * d;
    const bool live = d < SB_RDW, in_x = off >= 0 && off < rowbytes;
    const uint8_t* f = a.frames + b * (long)a.H * rowbytes + off;
#pragma unroll
    for (int row = tid >> 5; row < SB_RROWS; row += 8) {
      const int iy = iy0 + row;
      unsigned v = a.in_pad4s;
      if (in_x && iy >= 0 && iy < a.H) v = *(const unsigned*)(f + (long)iy * rowbytes) ^ 0x80808080u;
      if (live) *(unsigned*)(R + row * SB_RST + 4 * d) = v;
    }
  }
  __syncthreads();
  // ---- 2: stem conv on the 18x18 halo straight from R, 2 MFMAs per 16 pixels (32 output channels) ----
  {
    const v4i wa0 = a.ws64[lane], wa1 = a.ws64[64 + lane];
    const int4 b0 = int4_plus(*(const int4*)(a.bs + 8 * g), KB), b1 = int4_plus(*(const int4*)(a.bs + 8 * g + 4), KB);
    const float4 m0 = *(const float4*)(a.ms + 8 * g), m1 = *(const float4*)(a.ms + 8 * g + 4);
    const bool border = sy0 < 0 || sx0 < 0 || sy0 + SB_HW > a.SH || sx0 + SB_HW > a.SW;   // halo pixels outside the stem's output map
    const unsigned char* lane_row = R + min(g, 2) * SB_RST;
    for (int pg = wave; pg < SB_NPG; pg += 4) {
      const int p = pg * 16 + r;
      const int pc = min(p, SB_NPH - 1);
      const int hy = pc / SB_HW, hx = pc - hy * SB_HW;
      const int o = al + 6 * hx;
      const unsigned char* src = lane_row + hy * (2 * SB_RST) + (o & ~3);
      const unsigned d0 = *(const unsigned*)src, d1 = *(const unsigned*)(src + 4), d2 = *(const unsigned*)(src + 8);
      const unsigned sh = (unsigned)(o & 3);
      const v4i bv = {(int)__builtin_amdgcn_alignbyte(d1, d0, sh), (int)__builtin_amdgcn_alignbyte(d2, d1, sh), (int)__builtin_amdgcn_alignbyte(d2, d2, sh), 0};
      v4i a0 = v4i_from(b0), a1 = v4i_from(b1);
      a0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa0, bv, a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa1, bv, a1, 0, 0, 0);
      unsigned q0 = rq_pack_b<FK>(a0, m0, a.rqs), q1 = rq_pack_b<FK>(a1, m1, a.rqs);
      if (border && !((unsigned)(sy0 + hy) < (unsigned)a.SH && (unsigned)(sx0 + hx) < (unsigned)a.SW)) { q0 = a.zs4; q1 = a.zs4; }
      if (p < SB_NPH) *(uint2*)(S + p * SB_SST + 8 * g) = make_uint2(q0, q1);
    }
  }
  __syncthreads();
  // ---- 3: depthwise 3x3/1 on the 16x16x64 MFMA (wave -> output rows 4 wave.., both channel groups), project from its registers ----
  {
    // lane (r = output column, g = tap column): B operand of instruction m for output row py = 16 channels of halo pixel
    // (py + m, r + g); g = 3 carries zero weights (it reads one pixel past the window: still inside S)
    const unsigned char* lane_base = S + (wave * 4 * SB_HW + r + g) * SB_SST;
    unsigned dq[2][4];
#pragma unroll
    for (int cg = 0; cg < 2; cg++) {
      v4i wreg[3];
#pragma unroll
      for (int mi = 0; mi < 3; mi++) wreg[mi] = a.wd64[(cg * 3 + mi) * 64 + lane];
      const int4 bqm = int4_plus(*(const int4*)(a.bdm + 16 * cg + 4 * g), KB);
      const float4 mum = *(const float4*)(a.mdm + 16 * cg + 4 * g);
#pragma unroll
      for (int i = 0; i < 4; i += 2) {   // two output rows at a time: independent accumulate chains on four halo rows
        v4i rows[4];
#pragma unroll
        for (int j = 0; j < 4; j++) rows[j] = *(const v4i*)(lane_base + (i + j) * SB_HW * SB_SST + 16 * cg);
        v4i dqa = v4i_from(bqm), dqb = v4i_from(bqm);
#pragma unroll
        for (int mi = 0; mi < 3; mi++) {
          dqa = __builtin_amdgcn_mfma_i32_16x16x64_i8(wreg[mi], rows[mi], dqa, 0, 0, 0);
          dqb = __builtin_amdgcn_mfma_i32_16x16x64_i8(wreg[mi], rows[mi + 1], dqb, 0, 0, 0);
        }
        dq[cg][i] = rq_pack_b<FK>(dqa, mum, a.rqd);
        dq[cg][i + 1] = rq_pack_b<FK>(dqb, mum, a.rqd);
      }
    }
    const long wa = a.wpc[lane];
    const int4 bb = int4_plus(*(const int4*)(a.bp + 4 * g), KB);
    const float4 mm = *(const float4*)(a.mp + 4 * g);
    const int ox = ox0 + r;
    int8_t* const op = a.out + ((b * a.SH + oy0 + wave * 4) * (long)a.SW + ox) * a.Cout + 4 * g;
    const bool col_ok = ox < a.SW && 4 * g < a.Cout;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const long bv = (long)(((unsigned long)dq[1][i] << 32) | dq[0][i]);
      v4i acc = v4i_from(bb);
      acc = __builtin_amdgcn_mfma_i32_16x16x32_i8(wa, bv, acc, 0, 0, 0);
      const unsigned q = rq_pack_b<FK>(acc, mm, a.rqp);
      if (col_ok && oy0 + wave * 4 + i < a.SH) *(unsigned*)(op + (long)i * a.SW * a.Cout) = q;
    }
  }
}

}  // namespace vbt
