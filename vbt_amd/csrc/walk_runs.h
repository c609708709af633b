// The OC-SORT walk of a block of held-back steps as vbt_run lists, one list per vbt_tracker_update_from_detections_seq call.
// Plain C++ (no HIP, no vbt_pipeline): also built host-only by tests/test_walk_runs_host.py.
//
// A block is a contiguous piece of the detector output ring: slot s = (step in the block) * n + (batch slot).  Per tracker clip the
// caller lists the (slot, frame) pairs the clip has in the block, in step order.  A clip walks ONE run per tracker call: its frames
// at one slot stride and one frame step, which is all of them in a plain block.  Steps that break the pattern (an `active` mask or a
// clip map that changes inside the block, a detector-only step in the middle) continue in a further call.
#pragma once
#include <cstddef>
#include <vector>

#include "../../include/vbt_hip.h"

namespace vbt {

struct WalkFrame {
  int slot, frame;   // slot in the block; 1-based frame number of the clip
};

// Next call of the walk: for every clip with frames left (cur[c] < per[c].size()) the longest run that starts at cur[c] - it extends
// while slot stride and frame step stay what its first two frames set, and only if the frame number increases - and cur[c] behind
// it.  Clips with nothing left are skipped; false (and no runs): the walk is done.  cur starts at all zeros.
inline bool next_walk_call(const std::vector<std::vector<WalkFrame>>& per, const double* fps, std::vector<size_t>& cur, std::vector<vbt_run>& runs) {
  runs.clear();
  for (size_t c = 0; c < per.size(); c++) {
    const std::vector<WalkFrame>& v = per[c];
    const size_t a = cur[c];
    if (a >= v.size()) continue;
    size_t b = a + 1;
    int ss = 1, fs = 1;
    if (b < v.size() && v[b].frame > v[a].frame) {
      ss = v[b].slot - v[a].slot;
      fs = v[b].frame - v[a].frame;
      for (b++; b < v.size() && v[b].slot - v[b - 1].slot == ss && v[b].frame - v[b - 1].frame == fs;) b++;
    }
    runs.push_back(vbt_run{(int32_t)c, v[a].slot, ss, (int32_t)(b - a), v[a].frame, fs, fps[c]});
    cur[c] = b;
  }
  return !runs.empty();
}

}  // namespace vbt
