// Host-only statement of the table of a rep panel that follows the live analysis (include/vbt_hip.h, "Rep panel from the live
// analysis"), built with g++ -fsanitize=address,undefined (tests/test_overlay_hud_live_host.py): the per-phase record functions of
// vbt_amd/csrc/overlay_core.h - the ones vbt_overlay_set_hud and overlay_hud_follow_kernel both call - applied to a phase list read
// from a file.
//   overlay_hud_follow_check PHASES FPS CAP
// PHASES holds records of 6 doubles (time_start, time_end, y_start, y_end, rom, type).  Output:
//   phase i: the code of ov_hud_phase_check, then - for code 0 - the code of ov_hud_phase_record
//   rec i: fs fe rom_cm acv_cm type count                                          the table of ov_hud_follow_table
//   status: records, flags
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vbt_amd/csrc/overlay_core.h"

using namespace vbt;

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: %s PHASES FPS CAP\n", argv[0]); return 2; }
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::vector<double> ph;
  double rec[6];
  while (std::fread(rec, sizeof(rec), 1, fp) == 1) ph.insert(ph.end(), rec, rec + 6);
  std::fclose(fp);
  const int n = (int)(ph.size() / 6), cap = std::atoi(argv[3]);
  const double fps = std::atof(argv[2]);
  if (!(fps > 0) || cap < 1) { std::fprintf(stderr, "bad argument\n"); return 2; }
  for (int i = 0; i < n; i++) {
    const double* r = ph.data() + (size_t)i * 6;
    const int code = ov_hud_phase_check(r, i > 0 ? r - 6 : nullptr);
    int32_t t[OV_HUD_REC] = {0, 0, 0, 0, 0, 0};
    if (code) std::printf("phase %d: %d\n", i, code);
    else std::printf("phase %d: 0 %d\n", i, ov_hud_phase_record(r, fps, t));
  }
  // exactly the size vbt_overlay_hud_follow allocates: a record that strays is the sanitizer's
  std::vector<int32_t> tab((size_t)cap * OV_HUD_REC, -7);
  int flags = 0;
  const int m = ov_hud_follow_table(ph.data(), n, cap, fps, tab.data(), &flags);
  for (int i = 0; i < m; i++) {
    std::printf("rec %d:", i);
    for (int k = 0; k < OV_HUD_REC; k++) std::printf(" %d", tab[(size_t)i * OV_HUD_REC + k]);
    std::printf("\n");
  }
  std::printf("status: %d %d\n", m, flags);
  return 0;
}
