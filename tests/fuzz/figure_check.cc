// Host-only statement of the rep figure (include/vbt_hip.h, "Rep figure"), built with g++ -fsanitize=address,undefined
// (tests/test_figure_host.py): the functions of vbt_amd/csrc/figure_core.h - the ones vbt_figure_set and the kernels of figure.hip
// call - applied to one figure read from a file, one statement after the other.
//   figure_check CASE OUT
// CASE: int32 W, H, scale, thickness, T, P; T rows of 7 doubles; P phases of 6 doubles.
// OUT:  6 doubles (head); int32 T; T points of 5 int32; int32 n; n records of 12 int32; H * W * 3 bytes (the frame).
// Exit 3, naming it, for a row or phase vbt_figure_set refuses.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vbt_amd/csrc/figure_core.h"

using namespace vbt;

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s CASE OUT\n", argv[0]); return 2; }
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int32_t hdr[6];
  if (std::fread(hdr, sizeof(hdr), 1, fp) != 1) { std::fprintf(stderr, "short header\n"); return 2; }
  const int W = hdr[0], H = hdr[1], s = hdr[2], t = hdr[3], T = hdr[4], P = hdr[5];
  if (W < 1 || H < 1 || W > 16384 || H > 16384 || s < 1 || t < 1 || T < 0 || P < 0 || T > FIG_MAX_ROWS || P > FIG_MAX_PHASES) { std::fprintf(stderr, "bad header\n"); return 2; }
  std::vector<double> rows((size_t)T * 7), ph((size_t)P * 6);
  if ((T && std::fread(rows.data(), 56, (size_t)T, fp) != (size_t)T) || (P && std::fread(ph.data(), 48, (size_t)P, fp) != (size_t)P)) { std::fprintf(stderr, "short case\n"); return 2; }
  std::fclose(fp);
  const FigGeom G = fig_geom(W, H, s, t);
  if (G.PW < FIG_MIN_PLOT || G.PH < FIG_MIN_PLOT) { std::fprintf(stderr, "plot rectangle %d x %d too small\n", G.PW, G.PH); return 2; }
  for (int i = 0; i < T; i++)
    if (int code = fig_row_check(rows.data() + (size_t)i * 7, i > 0 ? rows.data() + (size_t)(i - 1) * 7 : nullptr)) { std::printf("row %d: %d\n", i, code); return 3; }
  for (int i = 0; i < P; i++)
    if (int code = ov_hud_phase_check(ph.data() + (size_t)i * 6, i > 0 ? ph.data() + (size_t)(i - 1) * 6 : nullptr)) { std::printf("phase %d: %d\n", i, code); return 3; }

  // exactly the sizes the handle gives a figure: a store that strays is the sanitizer's
  std::vector<double> sm((size_t)4 * T);
  for (int k = 0; k < 4; k++) fig_smooth_series(rows.data(), T, k, sm.data() + (size_t)k * T);
  double ext[4] = {0, 0, 0, 0};                                 // position min, max, velocity min, max
  for (int q = 0; q < 2 && T > 0; q++) {
    ext[2 * q] = ext[2 * q + 1] = sm[(size_t)2 * q * T];
    for (int k = 2 * q; k < 2 * q + 2; k++)
      for (int i = 0; i < T; i++) {
        const double v = sm[(size_t)k * T + i];
        if (v < ext[2 * q]) ext[2 * q] = v;
        if (v > ext[2 * q + 1]) ext[2 * q + 1] = v;
      }
  }
  double head[FIG_HEAD];
  fig_head(T, T ? rows[0] : 0.0, T ? rows[(size_t)(T - 1) * 7] : 0.0, ext[0], ext[1], ext[2], ext[3], head);
  std::vector<int32_t> pts((size_t)T * FIG_PT);
  for (int i = 0; i < T; i++) {
    const double sm4[4] = {sm[i], sm[(size_t)T + i], sm[(size_t)2 * T + i], sm[(size_t)3 * T + i]};
    fig_point(G, head, rows[(size_t)i * 7], sm4, pts.data() + (size_t)i * FIG_PT);
  }
  const int cap = FIG_FIXED_RECS + 4 * P;
  std::vector<int32_t> recs((size_t)cap * FIG_REC, -7);
  const int n = fig_records(G, head, ph.data(), P, recs.data(), cap);

  FigView V{pts.data(), 0, T, recs.data(), n, {}, {}};
  fig_view_unbounded(V);
  std::vector<uint8_t> frame((size_t)H * W * 3);
  for (int py = 0; py < H; py++)
    for (int px = 0; px < W; px += 4) {                          // four pixels at a time, as a lane of the render kernel takes them
      const int m = W - px < 4 ? W - px : 4;
      int seg0, seg1, k0, k1, c[4];
      fig_seg_range(V, 0, T, t, px - G.X0, px + m - 1 - G.X0, &seg0, &seg1, &k0, &k1);
      fig_pixels4(G, V, px, py, m, seg0, seg1, c);
      for (int e = 0; e < m; e++) {
        const uint32_t rgb = fig_rgb(c[e]);
        uint8_t* p = frame.data() + ((size_t)py * W + px + e) * 3;
        p[0] = (uint8_t)rgb; p[1] = (uint8_t)(rgb >> 8); p[2] = (uint8_t)(rgb >> 16);
      }
    }

  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  const int32_t T32 = T, n32 = n;
  std::fwrite(head, sizeof(head), 1, out);
  std::fwrite(&T32, 4, 1, out);
  if (T) std::fwrite(pts.data(), 4, pts.size(), out);
  std::fwrite(&n32, 4, 1, out);
  if (n) std::fwrite(recs.data(), 4, (size_t)n * FIG_REC, out);
  std::fwrite(frame.data(), 1, frame.size(), out);
  std::fclose(out);
  std::printf("ok: %d points, %d records\n", T, n);
  return 0;
}
