"""The per-chunk parameter blocks of the fused MBConv tile kernels, host side (no GPU): a stand-alone program includes the packers of
vbt_amd/csrc/weight_pack.h and the geometry of vbt_amd/csrc/fused_params_geom.h and, for seeded weights of the shapes of b1-b5 of Lite0 and
of Lite2's blocks (24 / 48 / 88 output channels: part-filled last blocks, other chunk counts), builds pack_fused_chunk_params' block for
every chunking (64- and 48-channel chunks), depthwise form (diagonal, Toeplitz, generic matrix pipe) and panel layout (tile-major tail,
block-major) and checks that

  - every region of every chunk holds, at `lane base + immediate`, the bytes the kernels without the form index in the existing packers'
    outputs (pack_weights / pack_expand48, pack_dw64_compact, pack_expdw2_taps, pack_dw_diag, pack_weights64 / pack_weights64_tail, the
    folded biases and the multipliers) - the index expressions are those of fused_block.h;
  - the sizes of the three regions and of a chunk record are those of the plan's launches (the table of the kernel's design note);
  - the last chunk of a width that is no multiple of the chunk (240 channels on 64-channel chunks) is zero past the width, as the source
    arrays are.

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
static int8_t rnd8() { rng_state = rng_state * 1664525u + 1013904223u; int8_t v = (int8_t)(rng_state >> 17); return v ? v : 1; }

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } } } while (0)

struct Block { const char* name; int Cin, Ce, k, S, Cout; };

static void run_block(const Block& b) {
  const int Ce = b.Ce, Cp = (Ce + 63) / 64 * 64, kk = b.k * b.k, KSe = (b.Cin + 31) / 32, NBP = (b.Cout + 63) / 64;
  std::vector<int8_t> we((size_t)Ce * b.Cin), wd((size_t)kk * Ce), wp((size_t)b.Cout * Ce);
  for (auto& v : we) v = rnd8();
  for (auto& v : wd) v = rnd8();
  for (auto& v : wp) v = rnd8();
  std::vector<int32_t> bqe(Ce), bqd(Ce), bqp(b.Cout);
  std::vector<float> mue(Ce), mud(Ce), mup(b.Cout);
  for (auto& v : bqe) v = 1000 + rnd8();
  for (auto& v : bqd) v = -500 + rnd8();
  for (auto& v : bqp) v = 77 + rnd8();
  for (auto& v : mue) v = 0.001f * (200 + rnd8());
  for (auto& v : mud) v = 0.002f * (200 + rnd8());
  for (auto& v : mup) v = 0.003f * (200 + rnd8());
  const std::vector<int> be = fold_bias(bqe.data(), we.data(), Ce, b.Cin, 3, W_ROWS, Cp), bdm = fold_bias(bqd.data(), wd.data(), Ce, kk, -5, W_TAPS, Cp);
  const std::vector<int> bp = fold_bias(bqp.data(), wp.data(), b.Cout, Ce, 9, W_ROWS, NBP * 64);
  const std::vector<float> me = pad_floats(mue.data(), Ce, Cp), md = pad_floats(mud.data(), Ce, Cp), mp = pad_floats(mup.data(), b.Cout, NBP * 64);
  for (int nt3 = 0; nt3 < 2; nt3++) {
    if (nt3 && Ce % 48) continue;
    const int NT = nt3 ? 3 : 4, CH = 16 * NT, nch = nt3 ? Ce / 48 : Cp / 64;
    std::vector<long> wex;
    if (nt3) wex = pack_expand48(we.data(), Ce, b.Cin, KSe);
    else pack_weights(we.data(), Ce, b.Cin, KSe, nch, nullptr, wex);
    const std::vector<int> kmap = nt3 ? kmap48(Ce) : std::vector<int>();
    for (int form = 0; form < 3; form++) {
      const int KT2 = (b.S * (b.S - 1) + b.k + 1) / 2, KT = (kk + 1) / 2;
      const std::vector<long> d64c = pack_dw64_compact(pack_dw64(wd.data(), Ce, b.k, Cp / 16), b.k);
      const std::vector<unsigned> dtz = pack_expdw2_taps(wd.data(), Ce, 0, Cp / 4, b.k, b.S);
      const std::vector<long> ddm = pack_dw_diag(wd.data(), Ce, kk, CH);
      const void* wdw = form == FPF_DIAG64 ? (const void*)d64c.data() : form == FPF_TOEPLITZ ? (const void*)dtz.data() : (const void*)ddm.data();
      for (int tail = 0; tail < 2; tail++) {
        if (tail && b.Cout % 64 == 0) continue;
        const int NTL = tail ? proj_tail_tiles(b.Cout) : 0, NBW = NTL ? NBP - 1 : NBP;
        std::vector<v4i> panel;
        if (tail) pack_weights64_tail(wp.data(), b.Cout, Ce, nch, NBP, panel, nt3 ? &kmap : nullptr);
        else pack_weights64(wp.data(), b.Cout, Ce, nch, NBP, panel, nt3 ? &kmap : nullptr);
        const FusedParamsGeom g = fused_params_geom(NT, KSe, form, b.k, b.S, NBP, NTL);
        const FusedParamsSrc src{wex.data(), be.data(), me.data(), wdw, bdm.data(), md.data(), panel.data(), nch, bp.data(), mp.data()};
        const std::vector<unsigned char> blk = pack_fused_chunk_params(g, NT, NBP, NTL, nch, src);
        const char* tag = b.name;
        CHECK(blk.size() == fused_chunk_params_bytes(g, nch) && blk.size() == (size_t)nch * g.chunk + NBP * 512, "%s: block of %zu bytes", tag, blk.size());
        CHECK(g.pe % 16 == 0 && g.pd % 16 == 0 && g.pp % 16 == 0 && g.pb % 16 == 0 && g.chunk == g.pe + g.pd + g.pp, "%s: regions are not 16-byte pieces", tag);
        CHECK(fused_params_lds(g) == g.chunk + g.pb, "%s: LDS area", tag);
        for (int c = 0; c < nch; c++) {
          const unsigned char* Pe = blk.data() + (size_t)c * g.chunk;
          const unsigned char* Pd = Pe + g.pe;
          const unsigned char* Pp = Pd + g.pd;
          // Pe: wreg[ks][t] = w[(ks * NT + t) * 64], w = we + c * KSe * NT * 64 + lane; eb[t] / em[t] = be / me + c * CH + 4 * NT * g + 4 * t
          for (int ks = 0; ks < KSe; ks++)
            for (int t = 0; t < NT; t++)
              for (int lane = 0; lane < 64; lane++)
                CHECK(!memcmp(Pe + 8 * ((ks * NT + t) * 64 + lane), &wex[(size_t)c * KSe * NT * 64 + lane + (ks * NT + t) * 64], 8), "%s nt3 %d chunk %d: expand operand", tag, nt3, c);
          for (int gq = 0; gq < 4; gq++)
            for (int t = 0; t < NT; t++) {
              CHECK(!memcmp(Pe + g.o_be + 4 * (4 * NT * gq + 4 * t), &be[c * CH + 4 * NT * gq + 4 * t], 16), "%s nt3 %d chunk %d: expand bias", tag, nt3, c);
              CHECK(!memcmp(Pe + g.o_me + 4 * (4 * NT * gq + 4 * t), &me[c * CH + 4 * NT * gq + 4 * t], 16), "%s nt3 %d chunk %d: expand multipliers", tag, nt3, c);
            }
          // Pd: the operands of the form, then bdm / md + c * CH + 16 * wave + 4 * g (diagonal, generic) or + 4 * (wq0 + q) (Toeplitz)
          for (int lane = 0; lane < 64; lane++) {
            if (form == FPF_DIAG64)
              for (int wave = 0; wave < NT; wave++) CHECK(!memcmp(Pd + 8 * (wave * 64 + lane), &d64c[(size_t)(c * NT + wave) * 64 + lane], 8), "%s nt3 %d chunk %d: wd64c", tag, nt3, c);
            else if (form == FPF_TOEPLITZ)
              for (int wq0 = 0; wq0 < 4 * NT; wq0 += NT)
                for (int i = 0; i < NT * KT2; i++)
                  CHECK(!memcmp(Pd + 4 * ((wq0 * KT2 + i) * 64 + lane), &dtz[((size_t)(c * 4 * NT + wq0) * KT2) * 64 + lane + i * 64], 4), "%s nt3 %d chunk %d: wtz", tag, nt3, c);
            else
              for (int wave = 0; wave < NT; wave++)
                for (int mi = 0; mi < KT; mi++)
                  CHECK(!memcmp(Pd + 8 * ((wave * KT + mi) * 64 + lane), &ddm[((size_t)(c * NT + wave) * KT) * 64 + lane + mi * 64], 8), "%s nt3 %d chunk %d: wdm", tag, nt3, c);
          }
          CHECK(!memcmp(Pd + g.o_bd, &bdm[c * CH], 4 * CH) && !memcmp(Pd + g.o_md, &md[c * CH], 4 * CH), "%s nt3 %d chunk %d: depthwise bias / multipliers", tag, nt3, c);
          // Pp: w[t * 64], w = panel + ((nb * KSp + c) * 4) * 64 + lane; the tail: panel + (NBW * KSp * 4 + c * NTL) * 64 + lane
          for (int lane = 0; lane < 64; lane++) {
            for (int nb = 0; nb < NBW; nb++)
              for (int t = 0; t < 4; t++)
                CHECK(!memcmp(Pp + 16 * ((nb * 4 + t) * 64 + lane), &panel[((size_t)(nb * nch + c) * 4) * 64 + lane + t * 64], 16), "%s nt3 %d chunk %d: panel block %d", tag, nt3, c, nb);
            for (int t = 0; t < NTL; t++)
              CHECK(!memcmp(Pp + 16 * ((NBW * 4 + t) * 64 + lane), &panel[((size_t)NBW * nch * 4 + (size_t)c * NTL) * 64 + lane + t * 64], 16), "%s nt3 %d chunk %d: panel tail", tag, nt3, c);
          }
        }
        const unsigned char* Pb = blk.data() + (size_t)nch * g.chunk;
        CHECK(!memcmp(Pb, bp.data(), NBP * 256) && !memcmp(Pb + NBP * 256, mp.data(), NBP * 256), "%s: projection bias / multipliers", tag);
        // a width that is no multiple of the chunk: the last chunk is zero past the width
        if (!nt3 && Ce % 64) {
          const unsigned char* Pe = blk.data() + (size_t)(nch - 1) * g.chunk;
          const int live = Ce - 64 * (nch - 1);
          for (int ch = live; ch < 64; ch++) {
            int z = 0;
            for (int j = 0; j < 4; j++) z |= Pe[g.o_be + 4 * ch + j] | Pe[g.o_me + 4 * ch + j] | Pe[g.pe + g.o_bd + 4 * ch + j] | Pe[g.pe + g.o_md + 4 * ch + j];
            CHECK(z == 0, "%s: channel %d of the last chunk is not zero-padded", tag, 64 * (nch - 1) + ch);
          }
          // expand operands: lane (i, kg) of tile t is channel 64 c + 16 (i >> 2) + 4 t + (i & 3)
          for (int ks = 0; ks < KSe; ks++)
            for (int t = 0; t < 4; t++)
              for (int lane = 0; lane < 64; lane++) {
                const int i = lane & 15, ch = 16 * (i >> 2) + 4 * t + (i & 3);
                long v;
                memcpy(&v, Pe + 8 * ((ks * 4 + t) * 64 + lane), 8);
                if (ch >= live) CHECK(v == 0, "%s: expand row %d of the last chunk is not zero", tag, ch);
              }
          // projection: K slots past the width meet zero weights (byte j of lane group g = K slot 16 g + j)
          const unsigned char* Pp = Pe + g.pe + g.pd;
          for (int t = 0; t < 4 * NBW + NTL; t++)
            for (int lane = 0; lane < 64; lane++)
              for (int j = 0; j < 16; j++)
                if (16 * (lane >> 4) + j >= live) CHECK(Pp[16 * (t * 64 + lane) + j] == 0, "%s: projection K slot past the width is not zero", tag);
        }
      }
    }
  }
}

// region sizes of the launches the pinned plan resolves to (bytes): Pe, Pd, Pp and the chunk count
struct Row { int NT, KSE, form, k, S, NBP, NTL, pe, pd, pp, total, chunks, Ce; };

int main() {
  const Block blocks[] = {{"lite0 b1", 16, 96, 3, 2, 24}, {"lite0 b2", 24, 144, 3, 1, 24}, {"lite0 b3", 24, 144, 5, 2, 40}, {"lite0 b4", 40, 240, 5, 1, 40},
                          {"lite0 b5", 40, 240, 3, 2, 80}, {"lite2 b3", 24, 144, 5, 2, 48}, {"lite2 b5", 48, 288, 5, 1, 48}, {"lite2 b7", 48, 288, 3, 2, 88}};
  for (const Block& b : blocks) run_block(b);
  const Row rows[] = {{3, 1, FPF_DIAG64, 3, 2, 1, 2, 1920, 1920, 2048, 5888, 2, 96},       // b1, variant 9
                      {3, 1, FPF_TOEPLITZ, 3, 1, 1, 2, 1920, 6528, 2048, 10496, 3, 144},    // b2, variant 57
                      {3, 1, FPF_DIAG64, 5, 2, 1, 3, 1920, 1920, 3072, 6912, 3, 144},       // b3, variant 9
                      {3, 2, FPF_TOEPLITZ, 5, 1, 1, 3, 3456, 9600, 3072, 16128, 5, 240},    // b4, variant 57
                      {4, 2, FPF_MATRIX, 3, 2, 2, 1, 4608, 10752, 5120, 20480, 4, 240}};    // b5, variant 1
  for (const Row& r : rows) {
    const FusedParamsGeom g = fused_params_geom(r.NT, r.KSE, r.form, r.k, r.S, r.NBP, r.NTL);
    const int nch = r.NT == 3 ? r.Ce / 48 : (r.Ce + 63) / 64;
    CHECK(g.pe == r.pe && g.pd == r.pd && g.pp == r.pp && g.chunk == r.total && nch == r.chunks, "size table: Pe %d Pd %d Pp %d chunk %d, %d chunks (want %d %d %d %d, %d)",
          g.pe, g.pd, g.pp, g.chunk, nch, r.pe, r.pd, r.pp, r.total, r.chunks);
    CHECK(fused_chunk_params_bytes(g, nch) == (size_t)r.chunks * r.total + 512 * r.NBP, "size table: block bytes");
  }
  printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_chunk_params_against_the_existing_packers(tmp_path, sanitize):
    src, exe = tmp_path / "params.cpp", tmp_path / "params"
    src.write_text(PROGRAM)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", *flags, "-I" + os.path.join(ROOT, "vbt_amd", "csrc"), str(src), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("0 failures") and "runtime error" not in res.stderr, res.stdout[-3000:] + res.stderr[-3000:]
