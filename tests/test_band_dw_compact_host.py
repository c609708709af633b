"""The compact depthwise operands of the chained row-band kernels, host side (no GPU): a stand-alone program includes the packers of
vbt_amd/csrc/weight_pack.h and the geometry of vbt_amd/csrc/band_geom.h and checks that

  - pack_band_dw_compact ([cg][lane], one dword per lane), expanded by the rule of dev_common.h's diag_operand (byte m of the dword,
    shifted to byte position i & 3 of dword i >> 2 of the lane's 16 bytes, i = lane & 15), gives every byte of pack_band_dw's twelve
    16-byte operands: 64 channels with random, all-zero, all -128 and all 127 weights, and 40 and 8 channels (channel groups and channels
    past the width are zero);
  - the bytes of the dword past the last tap (4 m + g > 8) and the dword's top byte are zero;
  - the array is 1 KB and band_lds_bytes gives the LDS of a 240-pixel head band (6 rows of 40) and of a 9-pixel band (3 rows of 3) in
    both forms: T0 | projection panel and tail | 1.5 KB depthwise area for the chained form.

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
#include "band_geom.h"

static unsigned rng_state = 2463534242u;
static int8_t rnd8() { rng_state = rng_state * 1664525u + 1013904223u; int8_t v = (int8_t)(rng_state >> 17); return v ? v : 1; }

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } } } while (0)

// diag_operand (dev_common.h) on the host: the 16 bytes of lane row i from the one byte wb
static void diag_operand_host(unsigned wb, int i, unsigned char out[16]) {
  const unsigned sh = wb << (8 * (i & 3));
  const int d = i >> 2;
  unsigned dw[4];
  for (int k = 0; k < 4; k++) dw[k] = d == k ? sh : 0u;
  memcpy(out, dw, 16);
}

static void run_case(const char* name, int C, int fill) {   // fill: 0 = random, 1 = all zero, 2 = all -128, 3 = all 127
  std::vector<int8_t> w((size_t)9 * C);
  for (auto& v : w) v = fill == 0 ? rnd8() : fill == 1 ? 0 : fill == 2 ? -128 : 127;
  const std::vector<v4i> full = pack_band_dw(w.data(), C);
  const std::vector<unsigned> compact = pack_band_dw_compact(w.data(), C);
  const int NCG = (C + 15) / 16;
  CHECK(compact.size() == 4 * 64 && compact.size() * sizeof(unsigned) == (size_t)BD_WD_COMPACT, "%s: compact array of %zu dwords", name, compact.size());
  CHECK(full.size() == (size_t)NCG * 3 * 64, "%s: full array of %zu operands", name, full.size());
  for (int cg = 0; cg < 4; cg++)
    for (int lane = 0; lane < 64; lane++) {
      const int i = lane & 15, g = lane >> 4;
      const unsigned wc = compact[(size_t)cg * 64 + lane];
      CHECK((wc >> 24) == 0, "%s: top byte of (%d, %d) is %u", name, cg, lane, wc >> 24);
      for (int m = 0; m < 3; m++) {
        const unsigned wb = (wc >> (8 * m)) & 0xffu;
        unsigned char got[16], want[16] = {0};
        diag_operand_host(wb, i, got);
        if (cg < NCG) memcpy(want, &full[((size_t)cg * 3 + m) * 64 + lane], 16);
        CHECK(!memcmp(got, want, 16), "%s: operand (cg %d, m %d, lane %d) differs", name, cg, m, lane);
        const int tap = 4 * m + g, ch = 16 * cg + i;
        const unsigned expect = (tap < 9 && ch < C) ? (unsigned)(uint8_t)w[(size_t)tap * C + ch] : 0u;
        CHECK(wb == expect, "%s: byte %d of (%d, %d) is %u, want %u", name, m, cg, lane, wb, expect);
      }
    }
}

int main() {
  run_case("C 64 random", 64, 0);
  run_case("C 64 zero", 64, 1);
  run_case("C 64 all -128", 64, 2);
  run_case("C 64 all 127", 64, 3);
  run_case("C 40 random", 40, 0);
  run_case("C 8 random", 8, 0);
  run_case("C 40 all -128", 40, 2);
  // LDS of a band, 64-channel maps (CS = 80, KS = 1).  240-pixel head band: 6 rows of a 40 x 40 map; 9-pixel band: the 3 x 3 level.
  CHECK(BD_WD_CHAIN == 1024 + 512 && BD_WP_TAIL == 1024, "depthwise area %d, tail %d", BD_WD_CHAIN, BD_WP_TAIL);
  CHECK(band_lds_bytes(6, 40, 80, 64, 1, true) == 8 * 42 * 80 + 4 * 1024 + 1024 + 1536, "240-pixel band, chained: %d", band_lds_bytes(6, 40, 80, 64, 1, true));
  CHECK(band_lds_bytes(6, 40, 80, 64, 1, true) == 33536, "240-pixel band, chained: %d", band_lds_bytes(6, 40, 80, 64, 1, true));
  CHECK(band_lds_bytes(6, 40, 80, 64, 1, false) == 8 * 42 * 80 + 240 * 80 + 4 * 1024 + 1024, "240-pixel band, two stages: %d", band_lds_bytes(6, 40, 80, 64, 1, false));
  CHECK(band_lds_bytes(6, 40, 80, 36, 1, true) == 8 * 42 * 80 + 3 * 1024 + 1024 + 1536, "240-pixel band, 36 outputs: %d", band_lds_bytes(6, 40, 80, 36, 1, true));
  CHECK(band_lds_bytes(3, 3, 80, 64, 1, true) == 5 * 5 * 80 + 4 * 1024 + 1024 + 1536, "9-pixel band, chained: %d", band_lds_bytes(3, 3, 80, 64, 1, true));
  CHECK(band_lds_bytes(3, 3, 80, 64, 1, true) == 8656, "9-pixel band, chained: %d", band_lds_bytes(3, 3, 80, 64, 1, true));
  CHECK(band_lds_bytes(3, 3, 80, 64, 1, false) == 5 * 5 * 80 + 16 * 80 + 4 * 1024 + 1024, "9-pixel band, two stages: %d", band_lds_bytes(3, 3, 80, 64, 1, false));
  // three 240-pixel chained bands share a CU's 160 KB (the head kernels' six waves per SIMD)
  CHECK(3 * band_lds_bytes(6, 40, 80, 64, 1, true) <= 160 * 1024, "three head bands per CU");
  printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_compact_operands_expand_to_the_full_ones(tmp_path, sanitize):
    src, exe = tmp_path / "dwc.cpp", tmp_path / "dwc"
    src.write_text(PROGRAM)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", *flags, "-I" + os.path.join(ROOT, "vbt_amd", "csrc"), str(src), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("0 failures") and "runtime error" not in res.stderr, res.stdout[-3000:] + res.stderr[-3000:]
