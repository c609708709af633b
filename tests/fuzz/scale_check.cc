// The host statements of vbt_amd/csrc/scale_core.h as a stand-alone program (built with -fsanitize=address,undefined by
// tests/test_scale_host.py, run as a program): the axis tables and the scaled frames of one case must equal what the numpy statement
// (tests/scale_ref.py) wrote into the case file.
//   case file: int32 fmt, H, W, h, w, B; per table of the handle's layout (plane 0 y, x; for YUV plane 1 y, x) int32 i0[n], int32 a[n];
//   B source frames; B expected frames.
// Exit 0 and "ok" when everything is equal, 1 with the first difference otherwise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vbt_amd/csrc/scale_core.h"

using namespace vbt;

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: scale_check CASE\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t hd[6];
  if (!read_all(f, hd, sizeof(hd))) { fprintf(stderr, "short header\n"); return 2; }
  const int fmt = hd[0], H = hd[1], W = hd[2], h = hd[3], w = hd[4], B = hd[5];
  if (fmt != VBT_PIX_RGB24 && !sc_is_yuv(fmt)) { fprintf(stderr, "bad format\n"); return 2; }
  if (sc_check_side(H, fmt) || sc_check_side(W, fmt) || sc_check_side(h, fmt) || sc_check_side(w, fmt) || B < 1 || B > 64) { fprintf(stderr, "bad size\n"); return 2; }
  const ScTableLayout L = sc_table_layout(h, w, fmt);
  std::vector<ScTap> taps((size_t)L.total);
  sc_build_tables(H, W, h, w, fmt, L, taps.data());
  for (int plane = 0; plane < 2; plane++)
    for (int axis = 0; axis < 2; axis++) {
      const int n = L.n[plane][axis];
      std::vector<int32_t> i0((size_t)n), a((size_t)n);
      if (!read_all(f, i0.data(), (size_t)n * 4) || !read_all(f, a.data(), (size_t)n * 4)) { fprintf(stderr, "short table\n"); return 2; }
      for (int k = 0; k < n; k++) {
        const ScTap t = taps[(size_t)(L.at[plane][axis] + k)];
        if (t.i0 != i0[(size_t)k] || t.a != a[(size_t)k]) {
          printf("table plane %d axis %d entry %d: (%d, %d), want (%d, %d)\n", plane, axis, k, t.i0, t.a, i0[(size_t)k], a[(size_t)k]);
          return 1;
        }
        if (t.a < 0 || t.a > SC_ONE) { printf("weight %d outside 0..2048\n", t.a); return 1; }
      }
    }
  const size_t sb = sc_frame_bytes(H, W, fmt), db = sc_frame_bytes(h, w, fmt);
  std::vector<uint8_t> src(sb * (size_t)B), want(db * (size_t)B), got(db * (size_t)B, 0xA5);
  if (!read_all(f, src.data(), src.size()) || !read_all(f, want.data(), want.size())) { fprintf(stderr, "short frames\n"); return 2; }
  if (fgetc(f) != EOF) { fprintf(stderr, "bytes behind the case\n"); return 2; }
  fclose(f);
  for (int b = 0; b < B; b++)
    sc_scale_frame_host(src.data() + sb * (size_t)b, got.data() + db * (size_t)b, H, W, h, w, fmt, taps.data() + L.at[0][0], taps.data() + L.at[0][1],
                        taps.data() + L.at[1][0], taps.data() + L.at[1][1]);
  for (size_t k = 0; k < got.size(); k++)
    if (got[k] != want[k]) {
      printf("frame %zu byte %zu: %d, want %d\n", k / db, k % db, got[k], want[k]);
      return 1;
    }
  printf("ok\n");
  return 0;
}
