// Process-wide stream pool, one per device, and the placement of a pipeline's busy streams on distinct hardware queues.
//
// HIP binds a stream to one of GPU_MAX_HW_QUEUES hardware queues when it is created (a zig-zag that also counts streams created by
// others) and the queue cannot be queried, so a pool stream is CLASSIFIED once per process: timed with a spinning wave against one
// representative of every queue group known so far (vbt_streams_share_queue, ~0.3 ms per probe).  Streams are kept for the life of
// the process and handed out again when their owner goes away, so that any number of pipelines created one after the other end up on
// the same few streams.  Host code; included by pipeline.hip only.
#pragma once
#include <algorithm>
#include <map>
#include <mutex>

#include "common.h"

namespace vbt {

inline int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v && *v ? atoi(v) : dflt;
}

struct StreamPool {
  std::vector<hipStream_t> streams;
  std::vector<int> free;          // indices not owned by anybody
  std::map<int, int> group;       // stream index -> hardware-queue group
  std::vector<int> reps;          // one stream index per known group
};
inline std::mutex g_pool_mu;      // held around every use of g_pools
inline StreamPool g_pools[64];

// Takes stream i of the pool (i < 0: the lowest free one, or - none free, or `create` - a new one on `device`) for an owner that
// keeps the indices it holds in `own`.
inline int pool_take(StreamPool& pool, int device, std::vector<int>& own, int i, bool create, int* out) {
  if (i < 0) {
    if (!pool.free.empty() && !create) {
      i = *std::min_element(pool.free.begin(), pool.free.end());
    } else {
      void* h = nullptr;
      PL_CHECK(vbt_stream_create(device, &h));
      pool.streams.push_back((hipStream_t)h);
      i = (int)pool.streams.size() - 1;
      pool.free.push_back(i);
    }
  }
  pool.free.erase(std::find(pool.free.begin(), pool.free.end(), i));
  own.push_back(i);
  *out = i;
  return VBT_OK;
}

inline int streams_shared(StreamPool& pool, int i, int j, bool* shared) {
  // host-timed: a descheduled host thread can make one probe read "shared"; two in a row cannot
  for (int rep = 0; rep < 2; rep++) {
    int sh = 0;
    PL_CHECK(vbt_streams_share_queue((void*)pool.streams[i], (void*)pool.streams[j], 150, &sh));
    if (!sh) { *shared = false; return VBT_OK; }
  }
  *shared = true;
  return VBT_OK;
}

inline int group_of(StreamPool& pool, int i, int* g_out) {
  auto it = pool.group.find(i);
  if (it == pool.group.end()) {
    int g = -1;
    for (int k = 0; k < (int)pool.reps.size() && g < 0; k++) {
      bool sh = false;
      PL_CHECK(streams_shared(pool, i, pool.reps[k], &sh));
      if (sh) g = k;
    }
    if (g < 0) {
      g = (int)pool.reps.size();
      pool.reps.push_back(i);
    }
    it = pool.group.emplace(i, g).first;
  }
  *g_out = it->second;
  return VBT_OK;
}

// The streams that carry kernels side by side (the `busy` roles) must sit on distinct hardware queues: an owner takes its busy streams
// from distinct groups - a stream that once collided is simply left for another role - and only creates streams while some group is
// still unseen.  Roles: 0..7 detector slots, 8 copy, 9 tracker; role_idx[r] is the pool stream of role r (-1: the owner has none) and
// comes back rearranged, `own` with the indices taken and given back.  *placement_ok = false when some busy role had to share a queue:
// a warning on stderr, or - `strict` - VBT_ERR_STATE.
inline int place_streams(StreamPool& pool, int device, const std::vector<int>& busy, bool strict, int role_idx[10], std::vector<int>& own,
                         bool* placement_ok) {
  if (env_int("VBT_PLACE_STREAMS", 1) == 0) return VBT_OK;
  VBT_HIP_CHECK(hipDeviceSynchronize());
  auto is_busy = [&](int r) { return std::find(busy.begin(), busy.end(), r) != busy.end(); };
  const int all_roles[10] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9};
  const int nq = std::max(1, env_int("GPU_MAX_HW_QUEUES", 4));
  std::vector<int> used;
  auto in_used = [&](int g) { return std::find(used.begin(), used.end(), g) != used.end(); };
  bool failed = false;
  for (int role : busy) {
    int cur = role_idx[role], g = 0;
    PL_CHECK(group_of(pool, cur, &g));
    if (in_used(g)) {
      // another stream of a group this owner does not use yet: one it already holds for an idle role, a free pool stream, or -
      // while fewer groups than hardware queues are known, and at most 3 nq times - a new one
      int cand = -1;
      bool from_spare = false;
      for (int r : all_roles) {
        if (role_idx[r] < 0 || is_busy(r)) continue;
        int gr = 0;
        PL_CHECK(group_of(pool, role_idx[r], &gr));
        if (!in_used(gr)) { cand = role_idx[r]; from_spare = true; break; }
      }
      if (cand < 0) {
        std::vector<int> fr = pool.free;
        std::sort(fr.begin(), fr.end());
        for (int i : fr) {
          int gi = 0;
          PL_CHECK(group_of(pool, i, &gi));
          if (!in_used(gi)) { cand = i; break; }
        }
      }
      int created = 0;
      while (cand < 0 && (int)pool.reps.size() < nq && created < 3 * nq) {
        int i = -1, gi = 0;
        PL_CHECK(pool_take(pool, device, own, -1, true, &i));
        created++;
        PL_CHECK(group_of(pool, i, &gi));
        if (!in_used(gi)) {
          cand = i;
        } else {   // stays in the pool for a later owner / another role
          pool.free.push_back(i);
          own.erase(std::find(own.begin(), own.end(), i));
        }
      }
      if (cand < 0) { failed = true; continue; }
      if (std::find(pool.free.begin(), pool.free.end(), cand) != pool.free.end()) {
        int dummy = 0;
        PL_CHECK(pool_take(pool, device, own, cand, false, &dummy));
      }
      if (from_spare)   // swap the two roles' streams
        for (int r : all_roles)
          if (role_idx[r] == cand) { role_idx[r] = cur; break; }
      role_idx[role] = cand;
      cur = cand;
      PL_CHECK(group_of(pool, cur, &g));
    }
    used.push_back(g);
  }
  // streams taken but left without a role go back to the pool
  for (size_t k = 0; k < own.size();) {
    const int i = own[k];
    bool held = false;
    for (int r : all_roles) held = held || role_idx[r] == i;
    if (held) { k++; continue; }
    own.erase(own.begin() + (long)k);
    pool.free.push_back(i);
  }
  if (failed) {
    *placement_ok = false;
    const int depth = (int)std::count_if(busy.begin(), busy.end(), [](int r) { return r < 8; });
    char msg[512];
    snprintf(msg, sizeof(msg),
             "vbt_pipeline: could not give every pipeline stream its own hardware queue: %d busy streams (depth %d%s%s), %d distinct queues seen, "
             "GPU_MAX_HW_QUEUES=%d (too few queues for this configuration, or kernels are being serialised by a profiler); throughput will be lower",
             (int)busy.size(), depth, is_busy(9) ? " + tracker stream" : "", is_busy(8) ? " + copy stream" : "", (int)pool.reps.size(), nq);
    if (strict) { set_error("%s", msg); return VBT_ERR_STATE; }
    fprintf(stderr, "%s\n", msg);
  }
  return VBT_OK;
}

}  // namespace vbt
