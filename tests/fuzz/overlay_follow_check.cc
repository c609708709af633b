// Host-only statement of the overlay's follow mode (include/vbt_hip.h, "Following a device row log"), built with
// g++ -fsanitize=address,undefined (tests/test_overlay_follow_host.py): a loop over ov_follow_row of vbt_amd/csrc/overlay_core.h - the
// per-row step the follow kernel implements 64 rows at a time - over a row log read from a file and cut into updates as asked, then
// what the draw kernel would find through the links: per row its trail, per frame its rows.
//   overlay_follow_check LOG H W FPS TRAIL MAX_FRAME MAX_ROWS_PER_FRAME CUT     CUT: K > 0 rows per update, 0 one update, -1 one per frame
// LOG holds the 64-byte records (int64 id, 7 doubles) in emission order.  Output:
//   row i: frame cx cy xmin ymin xmax ymax trail | cx,cy of the trail's points, the newest first
//   frame f: its accepted rows, the newest first
//   status: rows consumed, flags
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vbt_amd/csrc/overlay_core.h"

using namespace vbt;

// what overlay_follow_kernel does with the counter it reads
static void update(const OvFollow& F, int nrows) {
  const int cur = F.state[OV_STATE_CURSOR];
  const int n = nrows > F.rows_cap ? F.rows_cap : nrows;
  if (n < cur) { F.state[OV_STATE_FLAGS] |= VBT_OVERLAY_FOLLOW_REWOUND; return; }
  for (int i = cur; i < n; i++) F.state[OV_STATE_FLAGS] |= ov_follow_row(F, i);
  F.state[OV_STATE_CURSOR] = n;
}

int main(int argc, char** argv) {
  if (argc != 9) { std::fprintf(stderr, "usage: %s LOG H W FPS TRAIL MAX_FRAME MAX_ROWS_PER_FRAME CUT\n", argv[0]); return 2; }
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::vector<OverlayRow> rows;
  OverlayRow rec;
  while (std::fread(&rec, sizeof(rec), 1, fp) == 1) rows.push_back(rec);
  std::fclose(fp);
  const int n = (int)rows.size(), H = std::atoi(argv[2]), W = std::atoi(argv[3]);
  const double fps = std::atof(argv[4]);
  const int trail = std::atoi(argv[5]), max_frame = std::atoi(argv[6]), mrpf = std::atoi(argv[7]), cut = std::atoi(argv[8]);
  if (n < 1 || H < 1 || W < 1 || !(fps > 0) || trail < 1 || max_frame < 1 || max_frame > (1 << 24) || mrpf < 1 || mrpf > 64) {
    std::fprintf(stderr, "bad argument\n");
    return 2;
  }
  size_t slots = 64;
  while (slots < 2 * (size_t)n) slots <<= 1;
  // exactly the sizes vbt_overlay_follow allocates for rows_cap = n: a step that strays is the sanitizer's
  std::vector<int32_t> geom((size_t)n * OV_GEOM, -7), link((size_t)n * OV_LINK, -7), findex(((size_t)max_frame + 1) * 2, 0), state(OV_STATE, 0);
  std::vector<OvIdSlot> table(slots, OvIdSlot{-1, -1, -1});
  OvFollow F{};
  F.rows = rows.data(); F.geom = geom.data(); F.link = link.data(); F.findex = findex.data(); F.table = table.data(); F.state = state.data();
  F.fps = fps; F.rows_cap = n; F.max_frame = max_frame; F.max_rows_per_frame = mrpf; F.table_mask = (int)(slots - 1);
  F.H = H; F.W = W; F.trail = trail;
  if (cut > 0) {
    for (int k = cut; k < n; k += cut) update(F, k);
  } else if (cut < 0) {
    for (int k = 1; k < n; k++) {                                   // an update in front of every row whose time differs from the row before it
      if (rows[k].time != rows[k - 1].time) update(F, k);
    }
  }
  update(F, n);
  update(F, n);                                                     // an update without a new row changes nothing
  for (int i = 0; i < state[OV_STATE_CURSOR]; i++) {
    const int32_t* g = geom.data() + (size_t)i * OV_GEOM;
    std::printf("row %d:", i);
    for (int k = 0; k < OV_GEOM; k++) std::printf(" %d", g[k]);
    std::printf(" |");
    if (g[OV_TRAIL] > 0) std::printf(" %d,%d", g[OV_CX], g[OV_CY]);
    for (int seg = 0; seg < g[OV_TRAIL] - 1; seg++) {
      int older, newer;
      ov_follow_segment(link.data(), i, seg, &older, &newer);
      std::printf(" %d,%d", geom[(size_t)older * OV_GEOM + OV_CX], geom[(size_t)older * OV_GEOM + OV_CY]);
    }
    std::printf("\n");
  }
  for (int f = 1; f <= max_frame; f++) {
    const int cnt = findex[2 * (size_t)f + 1];
    if (!cnt) continue;
    std::printf("frame %d:", f);
    for (int s = 0; s < cnt; s++) std::printf(" %d", ov_follow_frame_row(findex.data(), link.data(), f, s));
    std::printf("\n");
  }
  std::printf("status: %d %d\n", state[OV_STATE_CURSOR], state[OV_STATE_FLAGS]);
  return 0;
}
