"""The tile-major part-filled last block of the projection panels, host side (no GPU): a stand-alone program includes the packer
(pack_weights64_tail of vbt_amd/csrc/weight_pack.h) and emulates the 16x16x64 MFMA as the kernels use it - A operand = the packed
weights of a tile (lane (i, g) = row i, K slice g), B operand = 16 bytes of a pixel per lane, lane (r, g) of the result holding rows
4 g .. 4 g + 3 of pixel r - against a direct product.  The full blocks are read block-major (row i of tile t = channel 16 (i >> 2) + 4 t +
(i & 3)), the last block tile-major over its NTL = ceil((N % 64) / 16) tiles (row i of tile t = channel 16 t + i, so lane (r, g) of tile t
holds channels 16 t + 4 g .. + 3: what the epilogues index bias, multipliers, residual and output with).  N in {8, 16, 24, 40, 72, 80, 112,
136} x K in {16, 48, 64, 144, 200}, without a K map (K-steps of 64 channels) and with the 48-channel one of the fused tiles (64 slots per
chunk, the first 48 used; kmap48 itself where K is a multiple of 48).  The activation bytes a kernel reads in unused K slots are random: they
must meet zero weights.  Rows past N are zero, the full blocks are pack_weights64's bytes, and N % 64 == 0 gives exactly pack_weights64.
The program is built twice, plain and with the address and undefined-behaviour sanitizers."""
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
static int8_t rnd8() { rng_state = rng_state * 1664525u + 1013904223u; return (int8_t)(rng_state >> 17); }

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } } } while (0)

// one 16x16x64 MFMA: acc[row i][pixel r] += sum over lane group g, byte j of A(lane (i, g))[j] * B(lane (r, g))[j]
static void mfma(const int8_t* tile, const int8_t B[64][16], long acc[16][16]) {
  for (int i = 0; i < 16; i++)
    for (int r = 0; r < 16; r++)
      for (int g = 0; g < 4; g++)
        for (int j = 0; j < 16; j++) acc[i][r] += (long)tile[((size_t)(16 * g + i)) * 16 + j] * B[16 * g + r][j];
}

static void run_case(int N, int K, bool use_kmap) {
  std::vector<int> kmap;
  if (use_kmap) {   // 64 slots per 48-channel chunk, the first 48 used
    const int nch = (K + 47) / 48;
    kmap.assign((size_t)nch * 64, -1);
    for (int c = 0; c < nch; c++)
      for (int q = 0; q < 48; q++)
        if (48 * c + q < K) kmap[(size_t)c * 64 + q] = 48 * c + q;
    if (K % 48 == 0) CHECK(kmap == kmap48(K), "kmap48(%d)", K);
  }
  const int KS = use_kmap ? (K + 47) / 48 : (K + 63) / 64, NB = (N + 63) / 64, nbl = N / 64, NTL = proj_tail_tiles(N);
  std::vector<int8_t> w((size_t)N * K), X((size_t)16 * K);
  for (auto& v : w) { v = rnd8(); if (v == 0) v = 1; }
  for (auto& v : X) v = rnd8();
  std::vector<v4i> ref, got;
  pack_weights64(w.data(), N, K, KS, NB, ref, use_kmap ? &kmap : nullptr);
  pack_weights64_tail(w.data(), N, K, KS, NB, got, use_kmap ? &kmap : nullptr);
  if (N % 64 == 0) {
    CHECK(got.size() == ref.size() && !memcmp(got.data(), ref.data(), 16 * ref.size()), "N %d K %d: not pack_weights64", N, K);
    return;
  }
  CHECK(NTL == (N % 64 + 15) / 16 && NTL >= 1 && NTL <= 4, "N %d: %d tail tiles", N, NTL);
  const size_t full = (size_t)nbl * KS * 4 * 64;
  CHECK(got.size() == full + (size_t)KS * NTL * 64, "N %d K %d kmap %d: %zu operands", N, K, (int)use_kmap, got.size());
  if (got.size() != full + (size_t)KS * NTL * 64) return;
  CHECK(!memcmp(got.data(), ref.data(), 16 * full), "N %d K %d kmap %d: full blocks differ from pack_weights64", N, K, (int)use_kmap);
  const int8_t* P = (const int8_t*)got.data();
  // rows past N of the last block are zero
  for (int ks = 0; ks < KS; ks++)
    for (int t = 0; t < NTL; t++)
      for (int lane = 0; lane < 64; lane++)
        if (64 * nbl + 16 * t + (lane & 15) >= N)
          for (int j = 0; j < 16; j++) CHECK(P[(full + ((size_t)ks * NTL + t) * 64 + lane) * 16 + j] == 0, "N %d K %d: row past N not zero", N, K);
  // the product, K-step by K-step, as the kernels run it
  std::vector<long> out((size_t)16 * NB * 64, 0);       // [pixel][channel], as the epilogue's indexing assigns it
  std::vector<int> hits((size_t)NB * 64, 0);
  for (int nb = 0; nb < NB; nb++) {
    const bool tail = nb == nbl;
    for (int t = 0; t < (tail ? NTL : 4); t++) {
      long acc[16][16];
      memset(acc, 0, sizeof acc);
      for (int ks = 0; ks < KS; ks++) {
        int8_t B[64][16];
        for (int lane = 0; lane < 64; lane++)
          for (int j = 0; j < 16; j++) {
            const int kp = 64 * ks + 16 * (lane >> 4) + j;
            const int k = use_kmap ? kmap[kp] : (kp < K ? kp : -1);
            B[lane][j] = k >= 0 ? X[(size_t)(lane & 15) * K + k] : rnd8();   // an unused slot: whatever lies behind the row
          }
        const size_t op = tail ? full + ((size_t)ks * NTL + t) * 64 : ((size_t)(nb * KS + ks) * 4 + t) * 64;
        mfma(P + op * 16, B, acc);
      }
      for (int r = 0; r < 16; r++)
        for (int g = 0; g < 4; g++)
          for (int j = 0; j < 4; j++) {
            const int ch = tail ? 64 * nb + 16 * t + 4 * g + j : 64 * nb + 16 * g + 4 * t + j;   // the epilogues' channel of register j of lane (r, g)
            out[(size_t)r * NB * 64 + ch] = acc[4 * g + j][r];
            if (r == 0) hits[ch]++;
          }
    }
  }
  for (int ch = 0; ch < NB * 64; ch++) {
    CHECK(hits[ch] == (ch < 64 * nbl + 16 * NTL ? 1 : 0), "N %d: channel %d produced %d times", N, ch, hits[ch]);
    for (int r = 0; r < 16; r++) {
      long want = 0;
      for (int k = 0; ch < N && k < K; k++) want += (long)w[(size_t)ch * K + k] * X[(size_t)r * K + k];
      CHECK(out[(size_t)r * NB * 64 + ch] == want, "N %d K %d kmap %d pixel %d channel %d: %ld, want %ld", N, K, (int)use_kmap, r, ch, out[(size_t)r * NB * 64 + ch], want);
    }
  }
}

int main() {
  for (int N : {8, 16, 24, 40, 72, 80, 112, 136, 64, 128})
    for (int K : {16, 48, 64, 144, 200})
      for (int km = 0; km < 2; km++) run_case(N, K, km);
  printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_tile_major_tail_against_direct_product(tmp_path, sanitize):
    src, exe = tmp_path / "tail.cpp", tmp_path / "tail"
    src.write_text(PROGRAM)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", *flags, "-I" + os.path.join(ROOT, "vbt_amd", "csrc"), str(src), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("0 failures") and "runtime error" not in res.stderr, res.stdout[-3000:] + res.stderr[-3000:]
