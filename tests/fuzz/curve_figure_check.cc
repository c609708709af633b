// Host-only statement of the curve figure (include/vbt_hip.h, "Curve figure"), built with g++ -fsanitize=address,undefined
// (tests/test_curve_figure_host.py): the functions of vbt_amd/csrc/curve_figure_core.h - the ones vbt_curve_figure_set and the kernels
// of curve_figure.hip call - applied to one figure read from a file, one statement after the other.
//   curve_figure_check CASE OUT
// CASE: int32 W, H, scale, thickness, corner, minor_x, minor_y, K, M; x_title[32]; y_title[32]; K series of (int32 n, colour,
//       text[64]); M marks of (int32 series, point, text[16]); the points of all series, two doubles each.
// OUT:  int32 K; K int32 (merged points per series); int32 total; total points of 3 int32; int32 n; n records of 28 int32;
//       H * W * 3 bytes (the frame, from the merged tables).
// Exit 3, naming it, for a series vbt_curve_figure_set refuses.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vbt_amd/csrc/curve_figure_core.h"

using namespace vbt;

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s CASE OUT\n", argv[0]); return 2; }
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int32_t hdr[9];
  CfFigure F{};
  if (std::fread(hdr, sizeof(hdr), 1, fp) != 1 || std::fread(F.x_title, 32, 1, fp) != 1 || std::fread(F.y_title, 32, 1, fp) != 1) { std::fprintf(stderr, "short header\n"); return 2; }
  const int W = hdr[0], H = hdr[1], s = hdr[2], t = hdr[3], K = hdr[7], M = hdr[8];
  if (W < 1 || H < 1 || W > 16384 || H > 16384 || s < 1 || t < 1 || K < 0 || K > CF_MAX_SERIES || M < 0 || M > CF_MAX_MARKS) { std::fprintf(stderr, "bad header\n"); return 2; }
  F.n_series = K; F.n_marks = M; F.corner = hdr[4]; F.minor_x = hdr[5]; F.minor_y = hdr[6];
  std::vector<CfSeries> ser((size_t)K);
  size_t total_in = 0;
  for (int k = 0; k < K; k++) {
    int32_t nc[2];
    if (std::fread(nc, sizeof(nc), 1, fp) != 1 || std::fread(ser[k].text, 64, 1, fp) != 1 || nc[0] < 0 || nc[0] > CF_MAX_POINTS) { std::fprintf(stderr, "short series\n"); return 2; }
    ser[k].n = nc[0]; ser[k].colour = nc[1]; ser[k].off = (int32_t)total_in; ser[k].rev = 0;
    total_in += (size_t)nc[0];
  }
  std::vector<CfMark> marks((size_t)M);
  if (M && std::fread(marks.data(), sizeof(CfMark), (size_t)M, fp) != (size_t)M) { std::fprintf(stderr, "short marks\n"); return 2; }
  std::vector<double> xy(total_in * 2);
  if (total_in && std::fread(xy.data(), 16, total_in, fp) != total_in) { std::fprintf(stderr, "short points\n"); return 2; }
  std::fclose(fp);
  const CfGeom G = cf_geom(W, H, s, t);
  if (G.PW < CF_MIN_PLOT || G.PH < CF_MIN_PLOT) { std::fprintf(stderr, "plot rectangle %d x %d too small\n", G.PW, G.PH); return 2; }
  for (int k = 0; k < K; k++) {
    int rev = 0, bad = -1;
    if (cf_series_check(xy.data() + (size_t)2 * ser[k].off, ser[k].n, &rev, &bad)) { std::printf("series %d, point %d: not monotone\n", k, bad); return 3; }
    ser[k].rev = rev;
  }
  for (int i = 0; i < M; i++)
    if (marks[i].series < 0 || marks[i].series >= K || marks[i].point < 0 || marks[i].point >= ser[marks[i].series].n) { std::printf("mark %d\n", i); return 3; }

  // exactly the sizes the handle gives a figure: a store that strays is the sanitizer's
  std::vector<std::vector<int32_t>> merged((size_t)K);
  std::vector<CfSeriesView> views((size_t)K);
  std::vector<int32_t> counts((size_t)K);
  for (int k = 0; k < K; k++) {
    merged[k].assign((size_t)ser[k].n * CF_PT, -7);
    counts[k] = cf_merge_series(xy.data() + (size_t)2 * ser[k].off, ser[k].n, ser[k].rev, G.PW, G.PH, merged[k].data());
    views[k] = CfSeriesView{merged[k].data(), 0, counts[k], ser[k].colour};
  }
  const int cap = CF_FIXED_RECS + 1 + 2 * K + 3 * M;
  std::vector<int32_t> recs((size_t)cap * CF_REC, -7);
  const int n = cf_records(G, F, ser.data(), marks.data(), xy.data(), recs.data(), cap);

  std::vector<uint8_t> frame((size_t)H * W * 3);
  for (int py = 0; py < H; py++)
    for (int px = 0; px < W; px += 4) {                          // four pixels at a time, as a lane of the render kernel takes them
      const int m = W - px < 4 ? W - px : 4;
      int c[4] = {0, 0, 0, 0};
      cf_pixels4(G, views.data(), K, recs.data(), n, px, py, m, c);
      for (int e = 0; e < m; e++) {
        const uint32_t rgb = cf_rgb(c[e]);
        uint8_t* p = frame.data() + ((size_t)py * W + px + e) * 3;
        p[0] = (uint8_t)rgb; p[1] = (uint8_t)(rgb >> 8); p[2] = (uint8_t)(rgb >> 16);
      }
    }

  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  const int32_t K32 = K, n32 = n;
  int32_t total = 0;
  for (int k = 0; k < K; k++) total += counts[k];
  std::fwrite(&K32, 4, 1, out);
  if (K) std::fwrite(counts.data(), 4, (size_t)K, out);
  std::fwrite(&total, 4, 1, out);
  for (int k = 0; k < K; k++)
    if (counts[k]) std::fwrite(merged[k].data(), 4, (size_t)counts[k] * CF_PT, out);
  std::fwrite(&n32, 4, 1, out);
  if (n) std::fwrite(recs.data(), 4, (size_t)n * CF_REC, out);
  std::fwrite(frame.data(), 1, frame.size(), out);
  std::fclose(out);
  std::printf("ok: %d merged points, %d records\n", total, n);
  return 0;
}
