"""Geometry of the expand + depthwise kernel's second form and of its small-map instantiation (vbt_amd/csrc/expdw2_geom.h), host side
(no GPU): a stand-alone program runs expdw2_choose on every expand + depthwise step of Lite0 (b6-b15 at 320 x 320) and Lite2 (448 x 448)
and checks

  - the b12-b15 shapes (10 x 10, 192 -> 1152 channels, 5 x 5 and 3 x 3, stride 1): one band, 3 position columns, 30 positions in two
    position groups, seven input pixel groups = two per wave on 8 waves (one on 16), the LDS layout by hand (E 15 / 13 rows of 64- / 48-byte
    quad planes, D 16 planes of 130 dwords, two parameter areas), and expdw2_small_ok: twice the LDS within a CU's 160 KB;
  - that b6-b11 (20 x 20 maps, and the stride-2 block whose OUTPUT is 10 x 10) and every Lite2 step (28 x 28 in bands, 14 x 14) are
    refused, each for a reason the test names: more than two position groups, more than two pixel groups per wave, or stride 2;
  - for every step, small or not, what the kernel derives at run time from the same arguments - the positions of the tallest band and
    their groups, the input pixel groups against what NW / 2 waves x GPW hold, every depthwise operand read and output offset within E
    and D and within the 16 bits the kernel packs them into - against the numbers of expdw2_geom, and `small` against a recount.

The program is built twice, plain and with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from conftest import ROOT

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include "expdw2_geom.h"

using namespace vbt;

static long fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } } } while (0)

struct Shape { const char* name; int H, W, Cin, OH, OW, k, S, pad_t; bool want_small; const char* why_not; };

// what expdw2_block.h computes from its arguments, per band, against the geometry
static void check_kernel_view(const Shape& s, const ExpDw2Geom& g) {
  const int DY = s.S, KT2 = (s.S * (DY - 1) + s.k + 1) / 2;
  int npg_max = 0, groups_max = 0;
  for (int band = 0; band < g.nbands; band++) {
    const int oy0 = band * g.brows, oy1 = std::min(oy0 + g.brows, s.OH), OHb = oy1 - oy0;
    CHECK(OHb > 0, "%s band %d is empty", s.name, band);
    const int iy_lo = std::max(oy0 * s.S - s.pad_t, 0), iy_hi = std::min(oy0 * s.S - s.pad_t + (OHb - 1) * s.S + s.k, s.H);
    const int HW = (iy_hi - iy_lo) * s.W;
    const int NPOS = ((OHb + DY - 1) / DY) * g.XB, NPGo = (NPOS + 15) >> 4;
    npg_max = std::max(npg_max, NPGo);
    groups_max = std::max(groups_max, (HW + 15) / 16);
    CHECK(NPGo <= XD2_NPG, "%s band %d: %d position groups", s.name, band, NPGo);
    // depthwise operand reads and output dwords of every lane (r, g) and position group, as the kernel packs them into 16 bits each
    for (int pg = 0; pg < NPGo; pg++)
      for (int lane = 0; lane < 64; lane++) {
        const int r = lane & 15, gg = lane >> 4;
        const int n = pg * 16 + r, nc = std::min(n, NPOS - 1), y = nc / g.XB, xk = nc % g.XB;
        const int eofs = s.S * DY * y * g.EYS + xk * 16 + (gg >> 1) * g.EYS + 16 * (gg & 1) + 15 * g.EQS;   // last quad of the chunk
        const int last = eofs + (KT2 - 1) * 2 * g.EYS + 16;                                                  // end of the last MFMA's read
        CHECK(last <= g.e_bytes && eofs < 65536, "%s: operand read ends at %d of %d bytes of E", s.name, last, g.e_bytes);
        const int oy = DY * y + (s.S == 2 ? gg >> 1 : 0), ox = (4 / s.S) * xk + (s.S == 2 ? gg & 1 : gg);
        if (n < NPOS && oy < OHb && ox < s.OW) {
          const int dofs = (oy * s.OW + ox) * 4 + 15 * g.PS;
          CHECK(dofs + 4 <= 16 * g.PS && dofs < 0xffff, "%s: output dword at %d of %d bytes of D", s.name, dofs, 16 * g.PS);
        }
      }
  }
  CHECK(npg_max == g.npg, "%s: %d position groups in the tallest band, the geometry says %d", s.name, npg_max, g.npg);
  if (g.gpw) CHECK(groups_max <= 4 * g.gpw, "%s: %d pixel groups, 4 waves x %d", s.name, groups_max, g.gpw);
  if (g.gpw16) CHECK(groups_max <= 8 * g.gpw16, "%s: %d pixel groups, 8 waves x %d", s.name, groups_max, g.gpw16);
  // the recount of `small`: the kernel's bounds (NPGB, GPW on XD2S_WAVES waves) and two workgroups' LDS
  const bool small = g.ok && s.S == 1 && npg_max <= XD2S_NPG && groups_max <= (XD2S_WAVES / 2) * XD2S_GPW && g.gpw == XD2S_GPW &&
                     2 * g.lds <= 160 * 1024;
  CHECK(small == g.small && g.small == expdw2_small_ok(g, s.S), "%s: small %d, recount %d", s.name, (int)g.small, (int)small);
  CHECK(g.lds == g.pd_off + 16 * (KT2 * 256 + 32) && g.pe_off == g.e_bytes + 16 * g.PS, "%s: LDS layout", s.name);
  CHECK(g.lds <= 100 * 1024, "%s: %d bytes of LDS", s.name, g.lds);
}

int main() {
  const Shape shapes[] = {
      // Lite0 at 320 x 320
      {"lite0 b6", 20, 20, 80, 20, 20, 3, 1, 1, false, "groups"},    {"lite0 b7", 20, 20, 80, 20, 20, 3, 1, 1, false, "groups"},
      {"lite0 b8", 20, 20, 80, 20, 20, 5, 1, 2, false, "groups"},    {"lite0 b9", 20, 20, 112, 20, 20, 5, 1, 2, false, "groups"},
      {"lite0 b10", 20, 20, 112, 20, 20, 5, 1, 2, false, "groups"},  {"lite0 b11", 20, 20, 112, 10, 10, 5, 2, 1, false, "stride"},
      {"lite0 b12", 10, 10, 192, 10, 10, 5, 1, 2, true, ""},         {"lite0 b13", 10, 10, 192, 10, 10, 5, 1, 2, true, ""},
      {"lite0 b14", 10, 10, 192, 10, 10, 5, 1, 2, true, ""},         {"lite0 b15", 10, 10, 192, 10, 10, 3, 1, 1, true, ""},
      // Lite2 at 448 x 448
      {"lite2 28 3x3", 28, 28, 88, 28, 28, 3, 1, 1, false, "groups"},   {"lite2 28 5x5", 28, 28, 88, 28, 28, 5, 1, 2, false, "groups"},
      {"lite2 28 5x5 b", 28, 28, 120, 28, 28, 5, 1, 2, false, "groups"}, {"lite2 28 -> 14", 28, 28, 120, 14, 14, 5, 2, 1, false, "stride"},
      {"lite2 14 5x5", 14, 14, 208, 14, 14, 5, 1, 2, false, "groups"},  {"lite2 14 3x3", 14, 14, 208, 14, 14, 3, 1, 1, false, "groups"}};
  int n_small = 0;
  for (const Shape& s : shapes) {
    const int KS64 = (s.Cin + 63) / 64;
    const ExpDw2Geom g = expdw2_choose(s.H, s.W, s.OH, s.OW, s.k, s.S, s.pad_t, KS64);
    CHECK(g.ok, "%s: the second form does not apply", s.name);
    if (!g.ok) continue;
    check_kernel_view(s, g);
    CHECK(g.small == s.want_small, "%s: small %d", s.name, (int)g.small);
    n_small += g.small;
    if (!s.want_small) {
      // the reason it is refused
      if (s.why_not[0] == 's') CHECK(s.S == 2 && g.gpw == 0, "%s: expected the stride to refuse it", s.name);
      else CHECK(g.npg > XD2S_NPG || g.gpw != XD2S_GPW, "%s: expected its position or pixel groups to refuse it (%d, gpw %d)", s.name, g.npg, g.gpw);
      continue;
    }
    // b12-b15 by hand
    const int KT2 = (s.k + 1) / 2, rows = 9 + 2 * KT2, eqs = (4 * (9 + s.k) + 15) & ~15;   // 10 position rows, the last MFMA of the last one may read a row past the kernel
    CHECK(g.nbands == 1 && g.brows == 10 && g.XB == 3 && g.npg == 2 && g.gpw == 2 && g.gpw16 == 1, "%s: bands %d x %d rows, XB %d, %d position groups, gpw %d / %d",
          s.name, g.nbands, g.brows, g.XB, g.npg, g.gpw, g.gpw16);
    CHECK(g.EQS == eqs && eqs == (s.k == 5 ? 64 : 48) && g.EYS >= 16 * eqs && g.EYS < 16 * eqs + 256 && g.EYS % 16 == 0, "%s: EQS %d EYS %d", s.name, g.EQS, g.EYS);
    CHECK(g.e_bytes == ((rows * g.EYS + 32 + 15) & ~15), "%s: E %d bytes for %d rows", s.name, g.e_bytes, rows);
    CHECK(g.PS == 4 * 130, "%s: PS %d", s.name, g.PS);
    CHECK(g.lds == g.e_bytes + 16 * 520 + 16 * (3 * 256 + 32) + 16 * (KT2 * 256 + 32), "%s: %d bytes of LDS", s.name, g.lds);
    CHECK(g.lds > 36 * 1024 && g.lds < 60 * 1024 && 2 * g.lds <= XD2_CU_LDS, "%s: %d bytes of LDS", s.name, g.lds);
    printf("%s: E %d + D %d + Pe %d + Pd %d = %d bytes of LDS, EYS %d\n", s.name, g.e_bytes, 16 * g.PS, g.pd_off - g.pe_off, g.lds - g.pd_off, g.lds, g.EYS);
  }
  CHECK(n_small == 4, "%d small steps", n_small);
  // the "fits twice" test alone: the same geometry with an LDS size over half a CU's is refused
  {
    ExpDw2Geom g = expdw2_choose(10, 10, 10, 10, 5, 1, 2, 3);
    CHECK(expdw2_small_ok(g, 1), "b12");
    g.lds = XD2_CU_LDS / 2 + 16;
    CHECK(!expdw2_small_ok(g, 1), "an LDS size that does not fit twice is accepted");
    g.lds = XD2_CU_LDS / 2;
    CHECK(expdw2_small_ok(g, 1) && !expdw2_small_ok(g, 2), "fits twice / stride 2");
    g.npg = XD2S_NPG + 1;
    CHECK(!expdw2_small_ok(g, 1), "three position groups accepted");
  }
  printf("%ld failures\n", fails);
  return fails ? 1 : 0;
}
"""


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_small_map_geometry(tmp_path, sanitize):
    src, exe = tmp_path / "xd2geom.cpp", tmp_path / "xd2geom"
    src.write_text(PROGRAM)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", *flags, "-I" + os.path.join(ROOT, "vbt_amd", "csrc"), str(src), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("0 failures") and "runtime error" not in res.stderr, res.stdout[-3000:] + res.stderr[-3000:]
