// Plain types the kernel argument structs embed (op_args.h, the *_args.h of the fused families): the vector type of an MFMA operand,
// the requantisation record of a conv, the parameters of the integer ADD.  Host units see these through launchers.h; the device
// helpers that work on them are in dev_common.h, which includes this header.
#pragma once
#include "common.h"

namespace vbt {

typedef int v4i __attribute__((ext_vector_type(4)));

// The requantisation in 5 VALU ops + 1 pack op per element (rq_u8 / rq_pack_b, dev_common.h): clamp(rne(t) + zp, lo, hi) ==
// clamp(rne(t), lo - zp, hi - zp) + zp because every quantity after rne() is an exact small integer in
// fp32; the result is produced in the unsigned domain (q + 128 in [0,255]) so v_cvt_pk_u8_f32 can pack
// it, and one XOR 0x80808080 per dword turns the four bytes back into int8.
struct Rq {
  float lo_f, hi_f, off;  // lo - zp, hi - zp, zp + 128
  int full;               // lo == -128 && hi == 127: the clamp is the [0,255] saturation of v_cvt_pk_u8_f32 itself
  int kb;                 // every accumulator of this conv (bias included) lies in (-2^22, 2^22) - proven on the host from the weights
                          // (conv_acc_bound): kernels may start their accumulators at bias + RQ_KBIAS and read them back as floats
};
// int -> float without v_cvt_f32_i32: for -2^22 <= acc < 2^22 the bit pattern 0x4B400000 + acc IS the float 1.5 * 2^23 + acc
// (exponent of 2^23, mantissa 0x400000 + acc), and subtracting 1.5 * 2^23 is exact.  The MFMA accumulates on top of the initial
// value, so a conv that starts at bias + RQ_KBIAS ends with that pattern for free; two v_pk_add_f32 then replace four
// v_cvt_f32_i32 per dword of outputs (15 -> 13 vector instructions per four requantised elements, none of them VOP1).
constexpr int RQ_KBIAS = 0x4B400000;
__host__ __device__ inline Rq make_rq(int zp, int lo, int hi, int kb = 0) {
  return Rq{(float)(lo - zp), (float)(hi - zp), (float)(zp + 128), (lo <= -128 && hi >= 127) ? 1 : 0, kb};
}

// ---- int8 ADD, XNNPACK qs8-vadd-minmax: q = clamp(((bias + a*am + b*bm) >> shift) + z_out, lo, hi).  The kernel's
// int16 / int8 saturating packs are monotone and the activation range lies inside int8, so the chain of saturations equals
// one clamp; it is applied before the zero point is added (lo - z_out, hi - z_out), and `off` = z_out + 128 moves the
// result to its u8 image so that four of them pack with shifts (no masks) and one XOR restores int8 (addq4, dev_common.h).
struct AddQ { int bias, am, bm, shift, lo, hi, off; };
static inline AddQ make_addq(const AddParams& p, int z_out, int lo, int hi) {
  return AddQ{p.bias, p.am, p.bm, p.shift, lo - z_out, hi - z_out, z_out + 128};
}

struct Epi {  // requantisation parameters of one conv
  const int* bias;    // folded bias, padded to NB*64
  const float* mult;  // padded to NB*64
  int zp, lo, hi;
  Rq rq;
};

}  // namespace vbt
