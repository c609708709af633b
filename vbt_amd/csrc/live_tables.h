// Live rep analysis (vbt_tracker_live_enable): the per-clip tables and the device helpers that work on them.  Plain structs - the host
// handle embeds LiveBufs / LiveCfg (tracker_host.h) - and device code; the kernels are in tracker_live.hip, the slot reset in tracker.hip.
#pragma once
#include "rep_analysis.h"
#include "tracker_state.h"

namespace vbt {

// ------------------------------------------------------------------------------------------
// live rep analysis (vbt_tracker_live_enable): the VelocityTracker of every id that can still win the export, fed while the clip runs
// ------------------------------------------------------------------------------------------
// Per clip a table of LIVE_ENTRIES entries keyed by row id: an id whose tracker is live (<= MAXT of them) or the best dead id (the
// only dead one that can still win: a dead id's cum never grows, and best_cum only grows).  Every other entry is retired.  Each entry
// carries the state of reference plot.py:90-95 (rolling / expanding means) and of VelocityTracker.py:30-48 after the id's rows so far;
// fed through vt_row, the step of the close-time scan, its phase list IS the list analyze_track would give on those rows.
constexpr int LIVE_ENTRIES = MAXT + 1;
constexpr int LIVE_PATH_FULL = 1, LIVE_PHASES_FULL = 2, LIVE_ROWS_LOST = 4;   // = VBT_LIVE_* (include/vbt_hip.h)
static_assert(LIVE_PATH_FULL == 1 && LIVE_PHASES_FULL == 2, "VtState.full bits");

struct LiveEntry {
  long long id;        // Row.id; -1 = free
  int nrows, pad;      // rows of the id consumed
  RollMean rm[4];      // rolling(5) x, y; expanding h, w
  double ring[5][2];   // raw (x, y) of the id's last 5 rows: what leaves the rolling window
  VtState s;
};

struct LiveClip {
  int cursor, flags;           // rows of the log consumed; LIVE_ROWS_LOST
  long long leader;            // export_id() after the rows consumed (-1: none)
  int leader_ver, pad;         // VtState.ver of the leader's entry when seq was last bumped
  unsigned long long seq;      // bumped whenever the leader or its phase list changes
};

struct LiveCfg {
  VtParams p;                  // preprocess = 1, flush = 0
  int path_cap, phase_cap;
};

struct LiveBufs {
  LiveClip* clips;             // [n_clips]
  LiveEntry* ents;             // [n_clips][LIVE_ENTRIES]
  double* paths;               // [n_clips][LIVE_ENTRIES][5][path_cap]
  double* phases;              // [n_clips][LIVE_ENTRIES][phase_cap][6]
  double* view;                // [n_clips][phase_cap][6]: flush-view scratch of the poll
  // rep metrics (vbt_tracker_rep_metrics_enable); null when they are off
  double* metrics;             // [n_clips][LIVE_ENTRIES][phase_cap][VT_METRICS]: the records of `phases`
  double* mview;               // [n_clips][phase_cap][VT_METRICS]: the records of `view`
};

__device__ inline VtPath live_path(const LiveBufs& b, const LiveCfg& c, int clip, int e) {
  const size_t pc = (size_t)c.path_cap;
  double* base = b.paths + ((size_t)clip * LIVE_ENTRIES + e) * 5 * pc;
  return VtPath{base, base + pc, base + 2 * pc, base + 3 * pc, base + 4 * pc, c.path_cap};
}
__device__ inline double* live_phases(const LiveBufs& b, const LiveCfg& c, int clip, int e) {
  return b.phases + ((size_t)clip * LIVE_ENTRIES + e) * c.phase_cap * 6;
}
__device__ inline double* live_metrics(const LiveBufs& b, const LiveCfg& c, int clip, int e) {
  return b.metrics ? b.metrics + ((size_t)clip * LIVE_ENTRIES + e) * c.phase_cap * VT_METRICS : nullptr;
}

__device__ inline void live_entry_init(LiveEntry& x, long long id) {
  x.id = id;
  x.nrows = 0;
  for (int j = 0; j < 4; j++) x.rm[j].init();
  vt_init(x.s);
}

// One row of the entry's id (the rows of an id are applied in log order).  A full entry is frozen: it only counts rows.
template <bool M>
__device__ inline void live_apply(LiveEntry& x, const Row& r, const LiveBufs& b, const LiveCfg& c, int clip, int e) {
  if (!x.s.full) {
    const int k = x.nrows % 5;   // slot of row nrows - 5, the one leaving the rolling window
    vt_row<M>(x.s, x.rm, c.p, &r.time, x.nrows >= 5, x.ring[k][0], x.ring[k][1], live_path(b, c, clip, e),
           VtPhases{live_phases(b, c, clip, e), M ? live_metrics(b, c, clip, e) : nullptr, c.phase_cap});
    x.ring[k][0] = r.x;
    x.ring[k][1] = r.y;
  }
  x.nrows += 1;
}

// The entry's phase list into out[phase_cap][6], as it stands or - flush - as end_processing() (VelocityTracker.py:224-230) would
// leave it, applied to a COPY of the state: it may append one phase and re-filter.  The live state is not touched.  One wavefront,
// uniform entry; returns the number of phases and ORs the entry's VBT_LIVE_* flags into *flags.  M (rep metrics enabled): mout holds
// room for phase_cap records of VT_METRICS doubles, the metrics of the phases in `out` - those of the appended one included.
template <bool M = false>
__device__ inline int live_view(const LiveEntry& x, const LiveBufs& b, const LiveCfg& c, int clip, int e, bool flush, double* out,
                                int* s_n, int* flags, int lane, double* mout = nullptr) {
  const double* ph = live_phases(b, c, clip, e);
  const int nph = x.s.nph;
  for (int i = lane; i < nph * 6; i += 64) out[i] = ph[i];
  if (M) {
    const double* pm = live_metrics(b, c, clip, e);
    for (int i = lane; i < nph * VT_METRICS; i += 64) mout[i] = pm[i];
  }
  __syncthreads();
  if (lane == 0) {
    int f = x.s.full, m = nph;
    if (flush && x.s.phase != 2 && !f) {
      VtState s = x.s;
      vt_end_phase<M>(s, c.p, live_path(b, c, clip, e), VtPhases{out, mout, c.phase_cap});
      f |= s.full;
      m = s.nph;
    }
    *flags |= f;
    *s_n = m;
  }
  __syncthreads();
  return *s_n;
}

__device__ inline void live_clip_init(LiveClip& L) { L.cursor = 0; L.flags = 0; L.leader = -1; L.leader_ver = -1; L.seq = 0; }
__device__ inline void live_entry_free(LiveEntry& x) { x.id = -1; x.nrows = 0; }

}  // namespace vbt
