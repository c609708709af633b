// Host-only statement of the validation figure (include/vbt_hip.h, "Validation figure"), built with g++ -fsanitize=address,undefined
// (tests/test_validation_host.py): the functions of vbt_amd/csrc/validation_core.h - the ones vbt_validation_set and the kernels of
// validation.hip call - applied to one pair read from a file, one statement after the other, and compared with what the numpy
// statement (tests/validation_ref.py) wrote for it: doubles with == (two NaNs are equal), integers exactly.
//   validation_check CASE WANT
// CASE: int32 W, H, scale, thickness, kind, nref, T, 0; double plate, rate; nref x 3 doubles; T x 5 doubles.
// WANT: 8 doubles stats; 6 doubles head; T x 3 doubles; int32 n, 0; n x 5 doubles; 4 int32 counts; int32 total, nrec; total x 3 int32;
//       nrec x 28 int32; int32 npix, 0; npix x (int32 x, y, rgb).
// Exit 1, naming the first difference of each table; exit 3 for a pair vbt_validation_set refuses.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vbt_amd/csrc/validation_core.h"

using namespace vbt;

namespace {

bool same(double a, double b) { return a == b || (a != a && b != b); }

template <class T>
bool read_n(std::FILE* fp, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, fp) == n;
}

int compare_d(const char* what, const double* got, const std::vector<double>& want) {
  for (size_t i = 0; i < want.size(); i++)
    if (!same(got[i], want[i])) { std::printf("%s[%zu]: %.17g, numpy %.17g\n", what, i, got[i], want[i]); return 1; }
  return 0;
}

int compare_i(const char* what, const int32_t* got, const std::vector<int32_t>& want) {
  for (size_t i = 0; i < want.size(); i++)
    if (got[i] != want[i]) { std::printf("%s[%zu]: %d, numpy %d\n", what, i, got[i], want[i]); return 1; }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s CASE WANT\n", argv[0]); return 2; }
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int32_t hdr[8];
  double pr[2];
  if (std::fread(hdr, sizeof(hdr), 1, fp) != 1 || std::fread(pr, sizeof(pr), 1, fp) != 1) { std::fprintf(stderr, "short header\n"); return 2; }
  const int W = hdr[0], H = hdr[1], s = hdr[2], t = hdr[3], kind = hdr[4], nref = hdr[5], T = hdr[6];
  if (W < 1 || H < 1 || W > 16384 || H > 16384 || s < 1 || t < 1 || nref < 0 || T < 0 || nref > VAL_MAX_ROWS || T > VAL_MAX_ROWS || (kind != 0 && kind != 1)) {
    std::fprintf(stderr, "bad header\n");
    return 2;
  }
  std::vector<double> ref, rows;
  if (!read_n(fp, ref, (size_t)nref * 3) || !read_n(fp, rows, (size_t)T * 5)) { std::fprintf(stderr, "short rows\n"); return 2; }
  std::fclose(fp);
  const ValGeom G = val_geom(W, H, s, t);
  if (G.PW < VAL_MIN_PLOT || G.PH < VAL_MIN_PLOT) { std::fprintf(stderr, "panel %d x %d too small\n", G.PW, G.PH); return 2; }
  int series = 0, row = 0;
  if (const int bad = val_pair_check(ref.data(), nref, rows.data(), T, &series, &row)) { std::printf("refused: reason %d, series %d, row %d\n", bad, series, row); return 3; }
  double t_min, t_max;
  int n;
  val_span(ref.data(), nref, rows.data(), T, pr[1], &t_min, &t_max, &n);
  if (!(t_max > t_min) || n < 2 || n > VAL_MAX_ROWS) { std::printf("refused: span %g .. %g, n %d\n", t_min, t_max, n); return 3; }

  // exactly the sizes the handle gives a pair: a store that strays is the sanitizer's
  std::vector<double> sm((size_t)T * 4), traj((size_t)T * 3), grid((size_t)n * VAL_GRID), stats(VAL_STATS), head(VAL_HEAD);
  std::vector<int32_t> ws[VAL_SERIES], pts[VAL_SERIES], cnt(VAL_SERIES, -7), recs((size_t)VAL_FIXED_RECS * CF_REC, -7);
  int32_t nrec = -7;
  ValPairOut O{};
  O.sm = sm.data(); O.traj = traj.data(); O.grid = grid.data(); O.stats = stats.data(); O.head = head.data();
  for (int k = 0; k < VAL_SERIES; k++) { pts[k].assign((size_t)(k & 1 ? T : nref) * CF_PT, -7); ws[k].assign((size_t)(k & 1 ? T : nref) * 2, -7); O.pts[k] = pts[k].data(); O.ws[k] = ws[k].data(); }
  O.cnt = cnt.data(); O.recs = recs.data(); O.nrec = &nrec; O.rec_cap = VAL_FIXED_RECS;
  val_pair(G, kind, pr[0], pr[1], ref.data(), nref, rows.data(), T, O);

  fp = std::fopen(argv[2], "rb");
  if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
  std::vector<double> w_stats, w_head, w_traj, w_grid;
  std::vector<int32_t> w_n, w_cnt, w_tot, w_pts, w_recs, w_npix, w_pix;
  bool ok = read_n(fp, w_stats, VAL_STATS) && read_n(fp, w_head, VAL_HEAD) && read_n(fp, w_traj, (size_t)T * 3) && read_n(fp, w_n, 2);
  ok = ok && w_n[0] >= 0 && w_n[0] <= VAL_MAX_ROWS && read_n(fp, w_grid, (size_t)w_n[0] * VAL_GRID) && read_n(fp, w_cnt, VAL_SERIES) && read_n(fp, w_tot, 2);
  ok = ok && w_tot[0] >= 0 && w_tot[1] >= 0 && w_tot[0] <= 4 * VAL_MAX_ROWS && w_tot[1] <= VAL_FIXED_RECS && read_n(fp, w_pts, (size_t)w_tot[0] * CF_PT) &&
       read_n(fp, w_recs, (size_t)w_tot[1] * CF_REC) && read_n(fp, w_npix, 2);
  ok = ok && w_npix[0] >= 0 && w_npix[0] <= (1 << 24) && read_n(fp, w_pix, (size_t)w_npix[0] * 3);
  std::fclose(fp);
  if (!ok) { std::fprintf(stderr, "short or bad file of expected values\n"); return 2; }

  int bad = 0;
  bad += compare_d("stats", stats.data(), w_stats);
  bad += compare_d("head", head.data(), w_head);
  bad += compare_d("traj", traj.data(), w_traj);
  if (w_n[0] != n) { std::printf("n: %d, numpy %d\n", n, w_n[0]); bad++; }
  else bad += compare_d("grid", grid.data(), w_grid);
  bad += compare_i("counts", cnt.data(), w_cnt);
  if (nrec != w_tot[1]) { std::printf("records: %d, numpy %d\n", nrec, w_tot[1]); bad++; }
  else bad += compare_i("records", recs.data(), w_recs);
  std::vector<int32_t> all;
  CfSeriesView views[VAL_SERIES];
  for (int k = 0; k < VAL_SERIES; k++) {
    if (cnt[k] < 0 || (size_t)cnt[k] * CF_PT > pts[k].size()) { std::printf("count %d of series %d\n", cnt[k], k); return 1; }
    all.insert(all.end(), pts[k].begin(), pts[k].begin() + (size_t)cnt[k] * CF_PT);
    views[k] = CfSeriesView{pts[k].data(), 0, cnt[k], k & 1};
  }
  if (all.size() != w_pts.size()) { std::printf("merged points: %zu, numpy %zu\n", all.size() / CF_PT, w_pts.size() / CF_PT); bad++; }
  else bad += compare_i("points", all.data(), w_pts);
  int bad_pix = 0;
  for (int i = 0; i < w_npix[0] && nrec >= 0 && nrec <= VAL_FIXED_RECS; i++) {
    const int x = w_pix[(size_t)i * 3], y = w_pix[(size_t)i * 3 + 1];
    if (x < 0 || x >= W || y < 0 || y >= H) { std::fprintf(stderr, "pixel (%d, %d) outside the frame\n", x, y); return 2; }
    const int px = x & ~3, m = W - px < 4 ? W - px : 4;            // four pixels at a time, as a lane of the render kernel takes them
    int c[4] = {0, 0, 0, 0};
    val_pixels4(G, views, recs.data(), nrec, px, y, m, c);
    const int32_t rgb = (int32_t)val_rgb(c[x - px]);
    if (rgb != w_pix[(size_t)i * 3 + 2] && bad_pix++ == 0) std::printf("pixel (%d, %d): %06x, numpy %06x\n", x, y, (unsigned)rgb, (unsigned)w_pix[(size_t)i * 3 + 2]);
  }
  if (bad || bad_pix) { std::printf("differs: %d tables, %d pixels\n", bad, bad_pix); return 1; }
  std::printf("ok: n %d, %zu merged points, %d records, %d pixels\n", n, all.size() / CF_PT, nrec, w_npix[0]);
  return 0;
}
