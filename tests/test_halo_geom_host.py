"""The halo bookkeeping of the fused tile kernels' expand stage (vbt_amd/csrc/halo_geom.h), host side (no GPU): a stand-alone program
checks the header's predicate and closed forms against the per-pixel loop they replace in fused_block.h - the loop that built an
out-of-image mask and a tail mask for every tile, with the coordinate test under `if (border)` inside it - for every tile position, wave
and lane of

  - the tiles of b1-b5 of Lite0 at 320 x 320 (halos of 17 x 17, 18 x 10, 19 x 19, 20 x 12 and b5's 41 x 7 on 20 x 3 tiles),
  - Lite2's tile-kernel blocks at 448 x 448 (112- and 56-pixel maps; 56 is three and a half 16-wide tiles),
  - both padding conventions: stride 2 SAME on an even map (3x3: bottom / right only, 5x5: one row more below than above) and stride 1
    (all four sides),
  - a few shapes of its own with part-filled last tiles on both axes and a halo of a multiple of 16 pixels (no tail lane at all).

Checked: halo_border is false exactly where no halo pixel is out of the image (so skipping the mask loop there leaves the mask the old
loop computed: zero); halo_oob_mask equals the old loop's mask on border tiles, with the row taken by integer division and by the
kernel's reciprocal form; halo_outside equals the four signed compares; the old tail mask's bit i is `p >= NPh`, which only the last group
has, on the lanes halo_group_lanes names; halo_wave_groups is the trip count of a wave's walk.

The program is built twice, plain and with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from conftest import ROOT

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include "halo_geom.h"

static long fails = 0, tiles_seen = 0, interior_seen = 0, tail_groups = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } } } while (0)

// the kernels' division through a reciprocal (dev_common.h: fdiv_small)
static int fdiv_small(int n, float rcp_d) { return (int)(((float)n + 0.5f) * rcp_d); }

// H x W: the block's input map; OH x OW its output; TX x TY the output tile
struct Shape { const char* name; int H, W, OH, OW, KK, S, TX, TY, pad_t, pad_l; };

static void run_shape(const Shape& s) {
  const int TXp = (s.TX + 3) & ~3;
  const int HWx = (TXp - 1) * s.S + s.KK, HWy = (s.TY - 1) * s.S + s.KK, NPh = HWx * HWy, NPG = (NPh + 15) >> 4;
  const float rcp_hwx = 1.0f / (float)HWx;
  const int tiles_x = (s.OW + s.TX - 1) / s.TX, tiles_y = (s.OH + s.TY - 1) / s.TY;
  CHECK(halo_groups(NPh) == NPG, "%s: %d groups", s.name, halo_groups(NPh));
  for (int ty = 0; ty < tiles_y; ty++)
    for (int tx = 0; tx < tiles_x; tx++) {
      const int iy0 = ty * s.TY * s.S - s.pad_t, ix0 = tx * s.TX * s.S - s.pad_l;
      // per pixel: is any halo pixel out of the image?
      bool any = false;
      for (int p = 0; p < NPh; p++) {
        const int hy = p / HWx, hx = p % HWx, iy = iy0 + hy, ix = ix0 + hx;
        const bool out = !(iy >= 0 && iy < s.H && ix >= 0 && ix < s.W);
        CHECK(out == halo_outside(iy, ix, s.H, s.W), "%s tile (%d, %d) pixel %d: halo_outside", s.name, ty, tx, p);
        any = any || out;
      }
      const bool border = halo_border(iy0, ix0, HWx, HWy, s.H, s.W);
      CHECK(border == any, "%s tile (%d, %d): border flag %d, out-of-image pixel %d", s.name, ty, tx, (int)border, (int)any);
      tiles_seen++;
      interior_seen += !border;
      for (int wave = 0; wave < 4; wave++) {
        int trips = 0;
        for (int r = 0; r < 16; r++) {
          // the loop the header replaces, as fused_block.h had it (without its `if (border)`: the flag must change nothing)
          unsigned oob_mask = 0, tail_mask = 0;
          trips = 0;
          for (int i = 0, pg = wave; pg < NPG; pg += 4, i++, trips++) {
            int p = pg * 16 + r;
            int pc = std::min(p, NPh - 1);
            int hy = pc / HWx, hx = pc - hy * HWx;
            int iy = iy0 + hy, ix = ix0 + hx;
            if (!(iy >= 0 && iy < s.H && ix >= 0 && ix < s.W)) oob_mask |= 1u << i;
            if (p >= NPh) tail_mask |= 1u << i;
          }
          const unsigned want = border ? oob_mask : 0u;
          CHECK(want == oob_mask, "%s tile (%d, %d) wave %d lane %d: an interior tile has out-of-image bits %x", s.name, ty, tx, wave, r, oob_mask);
          const unsigned got_i = border ? halo_oob_mask(wave, r, NPh, HWx, iy0, ix0, s.H, s.W, [&](int p) { return p / HWx; }) : 0u;
          const unsigned got_f = border ? halo_oob_mask(wave, r, NPh, HWx, iy0, ix0, s.H, s.W, [&](int p) { return fdiv_small(p, rcp_hwx); }) : 0u;
          CHECK(got_i == oob_mask && got_f == oob_mask, "%s tile (%d, %d) wave %d lane %d: mask %x / %x, the per-pixel loop %x", s.name, ty, tx, wave, r, got_i, got_f, oob_mask);
          for (int i = 0, pg = wave; pg < NPG; pg += 4, i++) {
            const bool tail = (tail_mask >> i) & 1u;
            CHECK(tail == !(r < halo_group_lanes(NPh, pg)), "%s wave %d lane %d group %d: tail bit %d", s.name, wave, r, pg, (int)tail);
            CHECK(!tail || pg == NPG - 1, "%s: a tail lane on group %d of %d", s.name, pg, NPG);
            tail_groups += tail;
          }
        }
        CHECK(trips == halo_wave_groups(NPh, wave), "%s wave %d: %d trips, halo_wave_groups %d", s.name, wave, trips, halo_wave_groups(NPh, wave));
      }
    }
}

int main() {
  const Shape shapes[] = {
      // Lite0 at 320 x 320: b1-b4 on the pinned tile kernels (8 x 8 and 16 x 8 tiles), b5 on the generic one (20 x 3)
      {"lite0 b1", 160, 160, 80, 80, 3, 2, 8, 8, 0, 0},   {"lite0 b2", 80, 80, 80, 80, 3, 1, 16, 8, 1, 1},
      {"lite0 b3", 80, 80, 40, 40, 5, 2, 8, 8, 1, 1},     {"lite0 b4", 40, 40, 40, 40, 5, 1, 16, 8, 2, 2},
      {"lite0 b5", 40, 40, 20, 20, 3, 2, 20, 3, 0, 0},
      // Lite2 at 448 x 448
      {"lite2 b1", 224, 224, 112, 112, 3, 2, 8, 8, 0, 0}, {"lite2 b2", 112, 112, 112, 112, 3, 1, 16, 8, 1, 1},
      {"lite2 b4", 112, 112, 56, 56, 5, 2, 8, 8, 1, 1},   {"lite2 b5", 56, 56, 56, 56, 5, 1, 16, 8, 2, 2},
      {"56 -> 28, 14 x 4 tiles", 56, 56, 28, 28, 3, 2, 14, 4, 0, 0},
      // part-filled last tiles on both axes, odd maps, a one-tile map, a halo of 18 x 8 = 144 pixels (no tail lane)
      {"odd 3x3/1", 37, 45, 37, 45, 3, 1, 16, 4, 1, 1},   {"odd 5x5/2", 37, 45, 19, 23, 5, 2, 8, 8, 2, 2},
      {"one tile", 8, 8, 8, 8, 3, 1, 8, 8, 1, 1},          {"no tail", 30, 30, 28, 28, 3, 1, 14, 6, 0, 0},
      {"lite0 b1, stride 1 padding", 160, 160, 80, 80, 3, 2, 8, 8, 1, 1}};
  for (const Shape& s : shapes) run_shape(s);
  // the loops above must have met both kinds of tile and tail lanes
  CHECK(interior_seen > 0 && interior_seen < tiles_seen && tail_groups > 0, "coverage: %ld interior of %ld tiles, %ld tail bits", interior_seen, tiles_seen, tail_groups);
  // the counts the design note quotes: interior tiles of b1-b4 of Lite0
  long n[4];
  for (int b = 0; b < 4; b++) {
    const long before = interior_seen;
    run_shape(shapes[b]);
    n[b] = interior_seen - before;
  }
  CHECK(n[0] == 81 && n[1] == 24 && n[2] == 9 && n[3] == 3, "interior tiles of b1-b4: %ld %ld %ld %ld", n[0], n[1], n[2], n[3]);
  printf("%ld tiles, %ld interior\n%ld failures\n", tiles_seen, interior_seen, fails);
  return fails ? 1 : 0;
}
"""


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_halo_closed_forms_against_the_per_pixel_loop(tmp_path, sanitize):
    src, exe = tmp_path / "halo.cpp", tmp_path / "halo"
    src.write_text(PROGRAM)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", *flags, "-I" + os.path.join(ROOT, "vbt_amd", "csrc"), str(src), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("0 failures") and "runtime error" not in res.stderr, res.stdout[-3000:] + res.stderr[-3000:]
