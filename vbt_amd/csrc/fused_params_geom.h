// The per-chunk parameter block of the fused MBConv tile kernels (fused_block.h: PLDS).  Plain C++: the kernel reads the geometry at
// compile time, the packer (weight_pack.h: pack_fused_chunk_params), the planner and the host test at run time.
#pragma once

// One block per (MBConv step, chunking, depthwise form, projection panel layout): `nch` chunk records of `chunk` bytes, then once per
// block the projection's bias | multipliers (pb bytes).  A chunk record is three regions of 16-byte pieces, each byte for byte the slice
// of the arrays the kernel without PLDS reads from global memory for that chunk, in the same per-lane order:
//   Pe  expand operands [ks][t][lane] x 8 B (we / we3) | be | me of the chunk's 16 NT channels                 (o_be, o_me: offsets in Pe)
//   Pd  depthwise operands (form 0: wd64c, NT x [lane] x 8 B; form 1: wtz, 4 NT quads x KT2 x [lane] x 4 B; form 2: wdm / wdm3,
//       NT x KT x [lane] x 8 B) | bdm | md of the chunk's channels                                              (o_bd, o_md: offsets in Pd)
//   Pp  the chunk's K-step of the projection panel: 4 NBW + NTL tiles of [lane] x 16 B (NTL > 0: NBW = NBP - 1 blocks of wpt / wpt3 and
//       the NTL live tiles of the tile-major last block; NTL = 0: NBW = NBP blocks of wp / wp3)
enum { FPF_DIAG64 = 0, FPF_TOEPLITZ = 1, FPF_MATRIX = 2 };
struct FusedParamsGeom { int pe, pd, pp, chunk, pb, o_be, o_me, o_bd, o_md; };
constexpr FusedParamsGeom fused_params_geom(int NT, int KSE, int form, int KK, int S, int NBP, int NTL) {
  FusedParamsGeom g{};
  const int CH = 16 * NT;
  g.o_be = KSE * NT * 512;
  g.o_me = g.o_be + 4 * CH;
  g.pe = g.o_me + 4 * CH;
  g.o_bd = form == FPF_DIAG64 ? NT * 512 : form == FPF_TOEPLITZ ? 4 * NT * ((S * (S - 1) + KK + 1) / 2) * 256 : NT * ((KK * KK + 1) / 2) * 512;
  g.o_md = g.o_bd + 4 * CH;
  g.pd = g.o_md + 4 * CH;
  g.pp = (4 * (NTL ? NBP - 1 : NBP) + NTL) * 1024;
  g.chunk = g.pe + g.pd + g.pp;
  g.pb = NBP * 512;
  return g;
}
// LDS bytes of the kernel's parameter area: one chunk record and the bias | multiplier tail
constexpr int fused_params_lds(const FusedParamsGeom& g) { return g.chunk + g.pb; }
