// COCO metrics: vbt_amd/csrc/coco_core.h run on the host, built with -fsanitize=address,undefined and run as a program
// (tests/test_coco_ref_host.py).  It reads a case file the test wrote - images with their detections and ground truth, and what the
// numpy restatement (tests/coco_ref.py) gives for them - and runs coco_evaluate_image, the statements the match kernel runs, on every
// image; the tables and, from the restatement's precision / recall arrays, the twelve stats are compared too.
// Case file, little endian: int32 n_images; per image int32 count, height, width, n_gt, float32 boxes [25][4], float32 scores [25],
// int32 gt [n_gt][4], then the expected int32 nd, float32 score [nd], int32 det [nd], uint64 matched [nd], uint64 ignored [nd],
// int32 npig [4]; after the images float64 iou_thrs [10], rec_thrs [101], precision [10][101][4][3], recall [10][4][3], stats [12].
// Prints "ok" and returns 0, or names the first difference and returns 1; 2: a bad case file.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../vbt_amd/csrc/coco_core.h"

using namespace vbt;

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) { printf("usage: coco_check CASE\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
  int32_t n_images = 0;
  if (!rd(f, &n_images, 1) || n_images < 0 || n_images > (1 << 20)) { printf("bad header\n"); return 2; }
  double iou_thrs[COCO_T], rec_thrs[COCO_R];
  coco_tables(iou_thrs, rec_thrs);
  for (int i = 0; i < n_images; i++) {
    int32_t head[4];
    if (!rd(f, head, 4) || head[3] < 0 || head[3] > COCO_MAXG) { printf("image %d: bad head\n", i); return 2; }
    std::vector<float> boxes(COCO_MAXD * 4), scores(COCO_MAXD);
    std::vector<int32_t> gt((size_t)head[3] * 4);
    int32_t nd = 0;
    if (!rd(f, boxes.data(), boxes.size()) || !rd(f, scores.data(), scores.size()) || !rd(f, gt.data(), gt.size()) || !rd(f, &nd, 1) || nd < 0 ||
        nd > COCO_MAXD) {
      printf("image %d: bad body\n", i);
      return 2;
    }
    std::vector<float> w_score((size_t)nd);
    std::vector<int32_t> w_det((size_t)nd);
    std::vector<uint64_t> w_m((size_t)nd), w_i((size_t)nd);
    int32_t w_npig[COCO_A];
    if (!rd(f, w_score.data(), w_score.size()) || !rd(f, w_det.data(), w_det.size()) || !rd(f, w_m.data(), w_m.size()) ||
        !rd(f, w_i.data(), w_i.size()) || !rd(f, w_npig, COCO_A)) {
      printf("image %d: bad expectation\n", i);
      return 2;
    }
    // exactly as large as the detections kept: a write behind them is the sanitizer's to find
    const int cnt = head[0] < 0 ? 0 : (head[0] > COCO_MAXD ? COCO_MAXD : head[0]);
    std::vector<float> g_score((size_t)cnt);
    std::vector<int32_t> g_det((size_t)cnt);
    std::vector<uint64_t> g_m((size_t)cnt), g_i((size_t)cnt);
    int32_t g_npig[COCO_A];
    const int got = coco_evaluate_image(boxes.data(), scores.data(), head[0], head[1], head[2], gt.data(), head[3], iou_thrs, g_score.data(),
                                        g_det.data(), g_m.data(), g_i.data(), g_npig);
    if (got != nd) { printf("image %d: %d detections, expected %d\n", i, got, nd); return 1; }
    for (int a = 0; a < COCO_A; a++)
      if (g_npig[a] != w_npig[a]) { printf("image %d range %d: %d boxes, expected %d\n", i, a, g_npig[a], w_npig[a]); return 1; }
    for (int k = 0; k < nd; k++) {
      if (memcmp(&g_score[k], &w_score[k], 4) != 0 || g_det[k] != w_det[k]) {
        printf("image %d rank %d: detection %d score %.9g, expected %d score %.9g\n", i, k, g_det[k], g_score[k], w_det[k], w_score[k]);
        return 1;
      }
      if (g_m[k] != w_m[k] || g_i[k] != w_i[k]) {
        printf("image %d rank %d: matched %010llx ignored %010llx, expected %010llx %010llx\n", i, k, (unsigned long long)g_m[k],
               (unsigned long long)g_i[k], (unsigned long long)w_m[k], (unsigned long long)w_i[k]);
        return 1;
      }
    }
  }
  const size_t n_pr = (size_t)COCO_T * COCO_R * COCO_A * COCO_M, n_rc = (size_t)COCO_T * COCO_A * COCO_M;
  std::vector<double> w_iou(COCO_T), w_rec(COCO_R), pr(n_pr), rc(n_rc), w_stats(12);
  if (!rd(f, w_iou.data(), w_iou.size()) || !rd(f, w_rec.data(), w_rec.size()) || !rd(f, pr.data(), n_pr) || !rd(f, rc.data(), n_rc) ||
      !rd(f, w_stats.data(), 12)) {
    printf("bad tail\n");
    return 2;
  }
  fclose(f);
  for (int i = 0; i < COCO_T; i++)
    if (iou_thrs[i] != w_iou[i]) { printf("iou threshold %d: %.17g, expected %.17g\n", i, iou_thrs[i], w_iou[i]); return 1; }
  for (int i = 0; i < COCO_R; i++)
    if (rec_thrs[i] != w_rec[i]) { printf("recall threshold %d: %.17g, expected %.17g\n", i, rec_thrs[i], w_rec[i]); return 1; }
  double stats[12];
  coco_stats(pr.data(), rc.data(), stats);
  for (int i = 0; i < 12; i++)
    if (!(fabs(stats[i] - w_stats[i]) <= 1e-12)) { printf("stat %d: %.17g, expected %.17g\n", i, stats[i], w_stats[i]); return 1; }
  printf("ok\n");
  return 0;
}
