"""The chained row-band projection panel, host side (no GPU): pack_band_pw_chain of vbt_amd/csrc/weight_pack.h lays the weights out in
the K order the depthwise stage leaves in registers (band_block.h), and holds the same bytes per output-channel row as the natural-order
panel of pack_band_pw, so the int32 sums of the two projections are equal."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PROGRAM = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef int v4i __attribute__((vector_size(16)));
#include "weight_pack.h"
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int N = atoi(argv[1]), C = 64;
  std::vector<int8_t> w((size_t)N * C);
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(w.data(), 1, w.size(), f) != w.size()) return 3;
  fclose(f);
  const std::vector<v4i> chain = pack_band_pw_chain(w.data(), N, C), nat = pack_band_pw(w.data(), N, C);
  FILE* o = fopen(argv[3], "wb");
  if (!o) return 4;
  const unsigned sizes[2] = {(unsigned)(chain.size() * 16), (unsigned)(nat.size() * 16)};
  fwrite(sizes, 4, 2, o);
  fwrite(chain.data(), 16, chain.size(), o);
  fwrite(nat.data(), 16, nat.size(), o);
  fclose(o);
  return 0;
}
"""


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    d = tmp_path_factory.mktemp("band_pack")
    src, exe = d / "pack.cpp", d / "pack"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "vbt_amd", "csrc"), str(src), "-o", str(exe)])

    def run(w):
        wf, of = d / "w.bin", d / "panels.bin"
        wf.write_bytes(w.tobytes())
        subprocess.check_call([str(exe), str(w.shape[0]), str(wf), str(of)])
        raw = of.read_bytes()
        n_chain, n_nat = np.frombuffer(raw, "<u4", 2)
        assert len(raw) == 8 + n_chain + n_nat
        return np.frombuffer(raw, np.int8, n_chain, 8), np.frombuffer(raw, np.int8, n_nat, 8 + n_chain)
    return run


@pytest.mark.parametrize("N", [64, 36, 18])
def test_chained_panel_byte_order_and_permutation(packer, N):
    rng = np.random.Generator(np.random.PCG64(100 + N))
    w = rng.integers(-128, 128, (N, 64), dtype=np.int8)
    w[w == 0] = 1                       # a stray zero could not be told from padding
    chain, nat = packer(w)
    NT = (N + 15) // 16
    assert chain.size == nat.size == NT * 64 * 16
    chain, nat = chain.reshape(NT, 64, 16), nat.reshape(NT, 64, 16)   # [t][lane][byte]
    for t in range(NT):
        for lane in range(64):
            i, g = lane & 15, lane >> 4
            for cg in range(4):
                for j in range(4):
                    want = int(w[16 * t + i, 16 * cg + 4 * g + j]) if 16 * t + i < N else 0
                    assert int(chain[t, lane, 4 * cg + j]) == want, (t, lane, cg, j)
    # the same bytes per (t, i) row as the natural-order panel (lanes i, 16 + i, 32 + i, 48 + i hold the row's 64 weights)
    for t in range(NT):
        for i in range(16):
            row_c = np.sort(chain[t, i::16].reshape(-1))
            row_n = np.sort(nat[t, i::16].reshape(-1))
            assert np.array_equal(row_c, row_n), (t, i)
            if 16 * t + i < N:
                assert np.array_equal(row_n, np.sort(w[16 * t + i]))
            else:
                assert not row_c.any()
