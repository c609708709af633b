"""The direct form of the stem block (stem_block.h: stem_block_direct_kernel, plan variant 1 of fused_stem_block), host side (no GPU):
a stand-alone program includes the two packers of vbt_amd/csrc/weight_pack.h and emulates the two stages they serve, lane by lane.

Stem conv: a random uint8 patch of raw rows (every byte random, the ones no tap reads included) goes through the R fill (XOR 0x80 per
dword); lane (r, g) reads the three aligned dwords that cover the 9 bytes of kernel row min(g, 2) of its halo pixel, funnel-shifts them
to the pixel's first byte and feeds 16 bytes to the 64 K slots of a 16x16x64 MFMA against pack_stem_block_stem64's A operand: the
result must be the direct 3x3/2 convolution for both output tiles, all four values of the row alignment and all 18 halo columns.
Projection: the two depthwise dwords of a lane (channels 4g.. and 16+4g..) as the B operand of a 16x16x32 MFMA against
pack_stem_block_proj_chain's A operand, compared with the direct 32 -> N product for N in {4, 8, 16}.  The program is built twice,
plain and with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from conftest import ROOT

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef int v4i __attribute__((vector_size(16)));
#include "weight_pack.h"

static unsigned rng_state = 2463534242u;
static unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } } } while (0)

constexpr int RST = 120, RROWS = 37, HW = 18;   // SB_RST, SB_RROWS, SB_HW of stem_block.h

static unsigned alignbyte(unsigned hi, unsigned lo, unsigned sh) { return (unsigned)((((unsigned long long)hi << 32) | lo) >> (8 * sh)); }
static unsigned dword_at(const std::vector<uint8_t>& R, size_t off) {
  CHECK(off % 4 == 0 && off + 4 <= R.size(), "dword read at %zu outside R (%zu)", off, R.size());
  if (off + 4 > R.size()) return 0;
  return (unsigned)R[off] | (unsigned)R[off + 1] << 8 | (unsigned)R[off + 2] << 16 | (unsigned)R[off + 3] << 24;
}

static void stem_case(int al, int pg) {
  std::vector<int8_t> w(32 * 27);
  for (auto& v : w) { v = (int8_t)rnd(); if (v == 0) v = -1; }
  std::vector<uint8_t> raw((size_t)RROWS * RST), R(raw.size());
  for (auto& v : raw) v = (uint8_t)rnd();
  for (size_t i = 0; i < raw.size(); i++) R[i] = raw[i] ^ 0x80;   // the R fill: XOR 0x80808080 per dword
  const std::vector<v4i> pk = pack_stem_block_stem64(w.data());
  CHECK(pk.size() == 2 * 64, "stem panel size %zu", pk.size());
  const int8_t* A8 = (const int8_t*)pk.data();
  for (int t = 0; t < 2; t++) {
    int A[16][64], B[64][16], hyv[16], hxv[16];
    for (int lane = 0; lane < 64; lane++) {
      const int r = lane & 15, g = lane >> 4;
      for (int j = 0; j < 16; j++) A[r][16 * g + j] = A8[((size_t)t * 64 + lane) * 16 + j];
      const int p = pg * 16 + r, pc = p < HW * HW ? p : HW * HW - 1;
      const int hy = pc / HW, hx = pc - hy * HW, o = al + 6 * hx;
      hyv[r] = hy; hxv[r] = hx;
      const size_t src = (size_t)(2 * hy + (g < 2 ? g : 2)) * RST + (o & ~3);
      const unsigned d0 = dword_at(R, src), d1 = dword_at(R, src + 4), d2 = dword_at(R, src + 8), sh = o & 3;
      const unsigned bv[4] = {alignbyte(d1, d0, sh), alignbyte(d2, d1, sh), alignbyte(d2, d2, sh), 0u};
      for (int j = 0; j < 16; j++) B[16 * g + j][r] = (int8_t)(bv[j >> 2] >> (8 * (j & 3)));
    }
    for (int i = 0; i < 16; i++)
      for (int n = 0; n < 16; n++) {
        long acc = 0;
        for (int k = 0; k < 64; k++) acc += A[i][k] * B[k][n];
        // lane (n, g) ends with rows 4g..4g+3 of tile t = channels 8g + 4t + j: the dword it stores at S + 8g + 4t
        const int g = i >> 2, co = 8 * g + 4 * t + (i & 3);
        long want = 0;
        for (int ky = 0; ky < 3; ky++)
          for (int kx = 0; kx < 3; kx++)
            for (int c = 0; c < 3; c++)
              want += (long)w[(size_t)co * 27 + (ky * 3 + kx) * 3 + c] * ((int)raw[(size_t)(2 * hyv[n] + ky) * RST + al + 6 * hxv[n] + 3 * kx + c] - 128);
        CHECK(acc == want, "stem al %d group %d tile %d pixel (%d,%d) channel %d: %ld, want %ld", al, pg, t, hyv[n], hxv[n], co, acc, want);
      }
  }
}

static void proj_case(int N) {
  std::vector<int8_t> w((size_t)N * 32), D(16 * 32);
  for (auto& v : w) { v = (int8_t)rnd(); if (v == 0) v = 1; }
  for (auto& v : D) v = (int8_t)rnd();
  const std::vector<long> pk = pack_stem_block_proj_chain(w.data(), N);
  CHECK(pk.size() == 64, "projection panel size %zu", pk.size());
  const int8_t* A8 = (const int8_t*)pk.data();
  int A[16][32], B[32][16];
  for (int lane = 0; lane < 64; lane++) {
    const int r = lane & 15, g = lane >> 4;
    for (int j = 0; j < 8; j++) A[r][8 * g + j] = A8[(size_t)lane * 8 + j];
    // the depthwise leaves lane (r, g) with channels 4g..4g+3 (group 0) and 16+4g..16+4g+3 (group 1) of pixel r: low and high dword of B
    for (int j = 0; j < 4; j++) { B[8 * g + j][r] = D[r * 32 + 4 * g + j]; B[8 * g + 4 + j][r] = D[r * 32 + 16 + 4 * g + j]; }
  }
  for (int i = 0; i < 16; i++)
    for (int n = 0; n < 16; n++) {
      long acc = 0, want = 0;
      for (int k = 0; k < 32; k++) acc += A[i][k] * B[k][n];
      for (int k = 0; k < 32 && i < N; k++) want += (long)w[(size_t)i * 32 + k] * D[n * 32 + k];
      CHECK(acc == want, "projection N %d pixel %d channel %d: %ld, want %ld", N, n, i, acc, want);
    }
}

int main() {
  for (int al = 0; al < 4; al++)
    for (int pg = 0; pg < (HW * HW + 15) / 16; pg++) stem_case(al, pg);   // all 21 pixel groups: every halo column, the last row, the clamped tail
  for (int N : {4, 8, 16}) proj_case(N);
  printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_stem_direct_panels_against_direct_convolution(tmp_path, sanitize):
    src, exe = tmp_path / "stem.cpp", tmp_path / "stem"
    src.write_text(PROGRAM)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", *flags, "-I" + os.path.join(ROOT, "vbt_amd", "csrc"), str(src), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("0 failures") and "runtime error" not in res.stderr, res.stdout[-3000:] + res.stderr[-3000:]
