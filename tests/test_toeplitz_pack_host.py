"""The band-Toeplitz depthwise of the fused MBConv tiles, host side (no GPU): a stand-alone program includes the tap packer
(pack_expdw2_taps of vbt_amd/csrc/weight_pack.h) and the LDS geometry (vbt_amd/csrc/tpz_geom.h), lays a random expanded halo out
quad-planar, and emulates the stage as fused_block.h runs it - per wave, channel quad, position group and lane: the 16-byte operand
read at `lane base + immediate`, the A operand rebuilt from the table's four bytes, the integer sum over the 64 K slots of the
16x16x64 MFMA, the D slot of the lane's output dword - against a direct depthwise convolution.  Cases: k in {3, 5} x stride {1, 2} x
chunks of 48 and 64 channels (Ce = 100: the last chunk of either is partial) x 8x8 and 16x8 tiles.  The parts of E the expand stage
never writes (padding columns, the rows past the halo) hold random bytes: they must meet zero weights.  The generalised packer must
also reproduce the bytes of the per-chunk packer it replaces.  The program is built twice, plain and with the address and
undefined-behaviour sanitizers."""
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
#include "tpz_geom.h"

// the per-chunk packer of expdw2_block.h as it was before it took a channel base and a quad count
static std::vector<unsigned> old_pack_expdw2_taps(const int8_t* w, int Ce, int c, int k, int S) {
  const int KT2 = (S * (S - 1) + k + 1) / 2;
  std::vector<unsigned> out((size_t)16 * KT2 * 64, 0);
  for (int q = 0; q < 16; q++)
    for (int mi = 0; mi < KT2; mi++)
      for (int lane = 0; lane < 64; lane++) {
        const int i = lane & 15, g = lane >> 4, qq = i >> 2, cc = i & 3, ch = 64 * c + 4 * q + cc;
        const int dy = S == 2 ? qq >> 1 : 0, dx = S == 2 ? qq & 1 : qq;
        const int ty = 2 * mi + (g >> 1) - S * dy;
        unsigned w4 = 0;
        for (int j = 0; j < 4; j++) {
          const int tx = 4 * (g & 1) + j - S * dx;
          if (ty >= 0 && ty < k && tx >= 0 && tx < k && ch < Ce) w4 |= (unsigned)(uint8_t)w[(size_t)(ty * k + tx) * Ce + ch] << (8 * j);
        }
        out[(q * KT2 + mi) * 64 + lane] = w4;
      }
  return out;
}

static unsigned rng_state = 12345u;
static int8_t rnd8() { rng_state = rng_state * 1664525u + 1013904223u; return (int8_t)(rng_state >> 17); }

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } } } while (0)

static void run_case(int k, int S, int NT, int PPW, int Ce) {
  const int CH = 16 * NT, nch = (Ce + CH - 1) / CH, Cp = nch * CH, TXP = 8 * PPW, FB_DST = 80;
  const int HWX = (TXP - 1) * S + k, HWY = 7 * S + k, KT2 = (S * (S - 1) + k + 1) / 2;
  const TpzGeom G = tpz_geom(k, S, PPW, NT);
  CHECK(G.EQS % 16 == 0 && G.EYS % 16 == 0 && G.EQS >= 4 * HWX && G.EYS >= 4 * NT * G.EQS && G.rows >= HWY && G.rows <= HWY + 2 && G.e_bytes == G.rows * G.EYS,
        "geometry k%d s%d nt%d ppw%d", k, S, NT, PPW);
  CHECK(tpz_read_cycles(S, G.XB, PPW, G.EYS) == 4 * PPW, "operand reads of k%d s%d nt%d ppw%d conflict: %d cycles", k, S, NT, PPW, tpz_read_cycles(S, G.XB, PPW, G.EYS));
  std::vector<int8_t> w((size_t)k * k * Ce), X((size_t)HWY * HWX * Cp);
  for (auto& v : w) { v = rnd8(); if (v == 0) v = 1; }
  for (auto& v : X) v = rnd8();
  const std::vector<unsigned> tab = pack_expdw2_taps(w.data(), Ce, 0, Cp / 4, k, S);
  CHECK(tab.size() == (size_t)(Cp / 4) * KT2 * 64, "table size");
  const int PGE = tpz_e_group(G, S), PGD = tpz_d_group(G, PPW, FB_DST);
  for (int c = 0; c < nch; c++) {
    std::vector<int8_t> E((size_t)G.e_bytes);
    for (auto& v : E) v = rnd8();
    // the expand epilogue: lane (pixel, g) writes quads NT g .. NT g + NT - 1 of halo pixel (hy, hx)
    for (int hy = 0; hy < HWY; hy++)
      for (int hx = 0; hx < HWX; hx++)
        for (int g = 0; g < 4; g++)
          for (int t = 0; t < NT; t++) {
            const size_t off = (size_t)tpz_e_store(G, hy, hx, NT * g + t);
            CHECK(off + 4 <= E.size(), "expand store outside E");
            for (int cc = 0; cc < 4; cc++) E[off + cc] = X[((size_t)hy * HWX + hx) * Cp + c * CH + 4 * (NT * g + t) + cc];
          }
    std::vector<int> hits((size_t)64 * PPW * CH, 0);
    for (int wave = 0; wave < 4; wave++)
      for (int q = 0; q < NT; q++)
        for (int pg = 0; pg < PPW; pg++) {
          const int wq0 = wave * NT;
          int acc[16][16];   // [A row i][position n]
          memset(acc, 0, sizeof acc);
          for (int mi = 0; mi < KT2; mi++) {
            int A[16][64], B[64][16];
            for (int lane = 0; lane < 64; lane++) {
              const int r = lane & 15, g = lane >> 4;
              const unsigned w4 = tab[((size_t)(c * 4 * NT + wq0 + q) * KT2 + mi) * 64 + lane];
              for (int j = 0; j < 16; j++) A[r][16 * g + j] = 0;
              for (int j = 0; j < 4; j++) A[r][16 * g + 4 * j + (r & 3)] = (int8_t)(w4 >> (8 * j));   // toeplitz_operand
              const long off = (long)tpz_e_offset(G, S, r, g, wq0) + q * G.EQS + (long)pg * PGE + mi * 2 * G.EYS;   // as fused_block.h reads
              CHECK(off >= 0 && off % 16 == 0 && off + 16 <= (long)E.size(), "operand read at %ld outside E (%zu)", off, E.size());
              if (off < 0 || off + 16 > (long)E.size()) return;
              for (int j = 0; j < 16; j++) B[16 * g + j][r] = E[off + j];
            }
            for (int i = 0; i < 16; i++)
              for (int n = 0; n < 16; n++)
                for (int kk = 0; kk < 64; kk++) acc[i][n] += A[i][kk] * B[kk][n];
          }
          // lane (n, g) ends with rows 4 g .. 4 g + 3: the 4 channels of output pixel g of position n -> one dword of D
          for (int n = 0; n < 16; n++)
            for (int g = 0; g < 4; g++) {
              const int doff = tpz_d_offset(G, S, PPW, FB_DST, n, g, wq0) + pg * PGD + 4 * q;   // as fused_block.h stores
              // the projection stage reads pixel slot s at tpz_d_slot(s): which slot and channel byte is this store?
              int slot = -1;
              for (int s = 0; s < 64 * PPW; s++)
                if (doff >= tpz_d_slot(G, PPW, FB_DST, s) && doff < tpz_d_slot(G, PPW, FB_DST, s) + 64) slot = s;
              const int cb = slot < 0 ? 0 : doff - tpz_d_slot(G, PPW, FB_DST, slot);
              CHECK(slot >= 0 && cb + 4 <= CH && tpz_d_slot(G, PPW, FB_DST, 64 * PPW - 1) + 64 <= 64 * PPW * FB_DST + 8 * G.DSK, "D store at %d: slot %d byte %d", doff, slot, cb);
              if (slot < 0 || cb + 4 > CH) return;
              const int py = slot / TXP, px = slot % TXP;
              for (int cc = 0; cc < 4; cc++) {
                const int ch = c * CH + cb + cc;
                long want = 0;
                if (ch < Ce)
                  for (int ty = 0; ty < k; ty++)
                    for (int tx = 0; tx < k; tx++) want += (long)w[(size_t)(ty * k + tx) * Ce + ch] * X[((size_t)(py * S + ty) * HWX + px * S + tx) * Cp + ch];
                CHECK(acc[4 * g + cc][n] == want, "k%d s%d nt%d ppw%d chunk %d pixel (%d,%d) channel %d: %d, want %ld", k, S, NT, PPW, c, py, px, ch, acc[4 * g + cc][n], want);
                hits[(size_t)slot * CH + cb + cc]++;
              }
            }
        }
    for (size_t i = 0; i < hits.size(); i++) CHECK(hits[i] == 1, "D element %zu written %d times", i, hits[i]);
  }
}

int main() {
  for (int k : {3, 5})
    for (int S : {1, 2}) {
      for (int NT : {3, 4})
        for (int PPW : {1, 2}) run_case(k, S, NT, PPW, 100);
      // the generalised packer against the per-chunk packer it replaces
      for (int Ce : {100, 144, 480}) {
        std::vector<int8_t> w((size_t)k * k * Ce);
        for (auto& v : w) v = rnd8();
        for (int c = 0; c < (Ce + 63) / 64; c++) {
          const std::vector<unsigned> a = old_pack_expdw2_taps(w.data(), Ce, c, k, S), b = pack_expdw2_taps(w.data(), Ce, 64 * c, 16, k, S);
          CHECK(a.size() == b.size() && !memcmp(a.data(), b.data(), 4 * a.size()), "packer bytes differ: k%d s%d Ce%d chunk %d", k, S, Ce, c);
        }
      }
    }
  printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_toeplitz_tables_against_direct_depthwise(tmp_path, sanitize):
    src, exe = tmp_path / "tpz.cpp", tmp_path / "tpz"
    src.write_text(PROGRAM)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", *flags, "-I" + os.path.join(ROOT, "vbt_amd", "csrc"), str(src), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("0 failures") and "runtime error" not in res.stderr, res.stdout[-3000:] + res.stderr[-3000:]
