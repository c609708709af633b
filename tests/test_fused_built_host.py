"""Which fused MBConv instantiations are built, host side (no GPU): vbt_amd/csrc/fused_built.h holds one list per special unit
(k_fused_mbconv_tpz.hip, k_fused_mbconv_tail.hip, k_fused_mbconv_params.hip) and the three predicates resolve_fused asks, computed from the
lists.  A stand-alone program includes the header with plain g++, walks the whole key space - k in {3, 5}, stride in {1, 2}, nbp 1..5, KSe
0..5, nt3, ppw2, dw64, tpz, ntl 0..4 (MBConv on the matrix pipe) - and prints every key a predicate accepts, with the waves per SIMD
fused_params_built returns, and the number of rows of each list.

The expected answers below were generated once, by running the three predicates as they stood before the lists existed - each a
hand-written boolean formula in launchers.h - over the same space.  The row counts are the kernel counts of the three units."""
import os
import subprocess

from conftest import ROOT

PROGRAM = r"""
#include <cstdio>
#include "fused_built.h"
int main() {
  using namespace vbt;
  printf("rows %d %d %d\n", FUSED_TPZ_ROWS, FUSED_TAIL_ROWS, FUSED_PARAMS_ROWS);
  for (int k = 3; k <= 5; k += 2) for (int s = 1; s <= 2; s++) for (int nbp = 1; nbp <= 5; nbp++) for (int kse = 0; kse <= 5; kse++)
    for (int ppw2 = 0; ppw2 < 2; ppw2++) {
      if (fused_tpz_built(k, s, nbp, kse, ppw2)) printf("tpz %d %d %d %d %d\n", k, s, nbp, kse, ppw2);
      for (int nt3 = 0; nt3 < 2; nt3++) for (int dw64 = 0; dw64 < 2; dw64++) for (int tpz = 0; tpz < 2; tpz++) for (int ntl = 0; ntl <= 4; ntl++) {
        FusedLaunch L{};
        L.k = k; L.stride = s; L.nbp = nbp; L.expand = true; L.mdw = true; L.nt3 = nt3; L.ppw2 = ppw2; L.dw64 = dw64; L.tpz = tpz; L.ntl = ntl;
        if (fused_tail_built(L, kse, ntl)) printf("tail %d %d %d %d %d %d %d %d %d\n", k, s, nbp, kse, nt3, ppw2, dw64, tpz, ntl);
        const int w = fused_params_built(L, kse, ntl);
        if (w) printf("params %d %d %d %d %d %d %d %d %d %d\n", k, s, nbp, kse, nt3, ppw2, dw64, tpz, ntl, w);
      }
    }
  return 0;
}
"""

# (k, stride, nbp, KSe, ppw2)
TPZ = [(3, 1, 1, 1, 0), (3, 1, 1, 1, 1), (3, 2, 1, 1, 0), (3, 2, 1, 1, 1), (5, 1, 1, 2, 0), (5, 1, 1, 2, 1), (5, 2, 1, 1, 0)]
# (k, stride, nbp, KSe, nt3, ppw2, dw64, tpz, ntl)
TAIL = [(3, 1, 1, 1, 0, 0, 0, 1, 2), (3, 1, 1, 1, 0, 0, 1, 1, 2), (3, 1, 1, 1, 0, 1, 0, 1, 2), (3, 1, 1, 1, 0, 1, 1, 1, 2),
        (3, 1, 1, 1, 1, 0, 0, 1, 2), (3, 1, 1, 1, 1, 0, 1, 1, 2), (3, 1, 1, 1, 1, 1, 0, 1, 2), (3, 1, 1, 1, 1, 1, 1, 1, 2),
        (3, 2, 1, 1, 0, 0, 0, 1, 2), (3, 2, 1, 1, 0, 0, 1, 1, 2), (3, 2, 1, 1, 0, 1, 0, 1, 2), (3, 2, 1, 1, 0, 1, 1, 1, 2),
        (3, 2, 1, 1, 1, 0, 0, 1, 2), (3, 2, 1, 1, 1, 0, 1, 0, 2), (3, 2, 1, 1, 1, 0, 1, 1, 2), (3, 2, 1, 1, 1, 1, 0, 1, 2),
        (3, 2, 1, 1, 1, 1, 1, 1, 2), (3, 2, 2, 2, 0, 0, 0, 0, 1),
        (5, 1, 1, 2, 0, 0, 0, 1, 3), (5, 1, 1, 2, 0, 0, 1, 1, 3), (5, 1, 1, 2, 0, 1, 0, 1, 3), (5, 1, 1, 2, 0, 1, 1, 1, 3),
        (5, 1, 1, 2, 1, 0, 0, 1, 3), (5, 1, 1, 2, 1, 0, 1, 1, 3), (5, 1, 1, 2, 1, 1, 0, 1, 3), (5, 1, 1, 2, 1, 1, 1, 1, 3),
        (5, 2, 1, 1, 0, 0, 0, 1, 3), (5, 2, 1, 1, 0, 0, 1, 1, 3), (5, 2, 1, 1, 1, 0, 0, 1, 3), (5, 2, 1, 1, 1, 0, 1, 0, 3),
        (5, 2, 1, 1, 1, 0, 1, 1, 3)]
# (k, stride, nbp, KSe, nt3, ppw2, dw64, tpz, ntl, waves per SIMD)
PARAMS = [(3, 1, 1, 1, 1, 1, 1, 1, 2, 4), (3, 2, 1, 1, 1, 0, 1, 0, 0, 4), (3, 2, 1, 1, 1, 0, 1, 0, 2, 4), (5, 1, 1, 2, 1, 1, 1, 1, 0, 3),
          (5, 1, 1, 2, 1, 1, 1, 1, 3, 3), (5, 2, 1, 1, 1, 0, 1, 0, 0, 3), (5, 2, 1, 1, 1, 0, 1, 0, 3, 3)]


def test_predicates_from_the_lists_answer_as_the_formulas_did(tmp_path):
    src, exe = tmp_path / "built.cpp", tmp_path / "built"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "vbt_amd", "csrc"), str(src), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    got = {"rows": [], "tpz": [], "tail": [], "params": []}
    for line in res.stdout.split("\n"):
        if line:
            got[line.split()[0]].append(tuple(int(x) for x in line.split()[1:]))
    assert got["rows"] == [(14, 17, 7)]
    assert sorted(got["tpz"]) == TPZ
    assert sorted(got["tail"]) == TAIL
    assert sorted(got["params"]) == PARAMS
