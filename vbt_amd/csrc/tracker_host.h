// The tracker handle and the host helpers its three units share (tracker.hip, tracker_analysis.hip, tracker_live.hip).  Host code.
#pragma once
#include <algorithm>

#include "common.h"
#include "dev_mem.h"
#include "live_tables.h"
#include "tracker_state.h"

struct vbt_tracker {
  int n_clips = 0, rows_cap = 0, device = 0;
  vbt::TrackParams p;
  bool sort = false;                     // the step is sort_step.h's (vbt_tracker_create_sort), not ocsort_step.h's
  int id_base = 0;                       // row ids of a fresh clip start at id_base + 1 (SORT only; 0 for OC-SORT)
  double q44 = 0, q66 = 0;
  vbt::DevBuf<vbt::ClipState> states;
  vbt::DevBuf<vbt::Row> rows;
  vbt::DevBuf<double> cols;     // [n_clips][rows_cap][7] gathered rows of the export id
  vbt::DevBuf<double> scratch;  // [n_clips][rows_cap][5]
  vbt::DevBuf<double> phases;   // [n_clips][MAXPH][6]
  vbt::DevBuf<int> nph, T, best;
  bool finished = false;
  hipStream_t finish_stream = nullptr;   // stream vbt_tracker_finish ran on: the close waits for it, not for the device
  vbt::Mirror summary;                   // packed close block (pack_summary_kernel), grown on demand
  vbt::Mirror view;                      // packed read-back block of the one-frame path (tracker_one_kernel)
  int view_clip = -1;                    // clip whose state view.host() mirrors (-1: none: the state changed on another path)
  bool stepped = false;                  // a tracker step was enqueued since creation / the last reset
  // live rep analysis (vbt_tracker_live_enable); off: no allocation, no launch
  bool live = false;
  vbt::DevBuf<vbt::LiveClip> live_clips;   // the tables lb points into
  vbt::DevBuf<vbt::LiveEntry> live_ents;
  vbt::DevBuf<double> live_paths, live_phases, live_view;
  vbt::LiveBufs lb{};
  vbt::LiveCfg lc{};
  vbt::Mirror live_poll;                 // packed poll block (live_pack_kernel), grown on demand
  // rep metrics (vbt_tracker_rep_metrics_enable); off: no allocation, and every kernel gets a null pointer for them
  bool rep_metrics = false;
  vbt::DevBuf<double> metrics;             // [n_clips][MAXPH][VT_METRICS]: the records of `phases`
  vbt::DevBuf<double> live_metrics, live_mview;   // what lb.metrics / lb.mview point into (live analysis on too)
};

namespace vbt {

// live analysis after a tracker launch, on the same stream (so before whatever the caller records there next)
int live_after(vbt_tracker* t, hipStream_t st);
// the live tables as vbt_tracker_live_enable leaves them: one launch on the null stream, enqueue only (live analysis is on)
void live_init(vbt_tracker* t);
// live analysis off, its tables freed
void live_free(vbt_tracker* t);
// The live tables' metrics, when both the live analysis and the rep metrics are on and they are not there yet (whichever of the two
// enables came second calls it).  false: hipMalloc failed, nothing changed.
bool live_metrics_alloc(vbt_tracker* t);

// What a reader of the live tables outside the tracker's units needs (the overlay's rep panel, overlay.hip): the tables as the
// tracker's kernels take them.  on == false: live analysis is not enabled and b holds no pointer.
struct LiveTables {
  LiveBufs b;
  LiveCfg c;
  int n_clips, device;
  bool on;
};
inline LiveTables live_tables(const vbt_tracker* t) { return LiveTables{t->lb, t->lc, t->n_clips, t->device, t->live}; }

// clips[i0 ...) as the argument of one launch (at most CLIP_LIST of them)
inline ClipList clip_list(const int32_t* clips, int i0, int n) {
  ClipList l{};
  l.n = std::min(CLIP_LIST, n - i0);
  for (int i = 0; i < l.n; i++) l.clip[i] = clips[i0 + i];
  return l;
}

// The part of a ClipState the host reads back for its counters: the leading scalars + order + used (not last_out, not the tracks)
struct StateHeader {
  alignas(8) char bytes[offsetof(ClipState, last_out)];
  const ClipState* operator->() const { return (const ClipState*)bytes; }
};
static_assert(sizeof(StateHeader) == offsetof(ClipState, last_out), "one header per stride of the strided copy");
// one clip's, with a blocking copy (the caller has synchronised the device) ...
int fetch_state_header(vbt_tracker* t, int clip, StateHeader* h);
// ... or every clip's, in one strided copy on st and one synchronisation of st
int fetch_state_headers(vbt_tracker* t, std::vector<StateHeader>* h, hipStream_t st);
// VBT_ERR_CAPACITY with the text set when the clip dropped births or rows, or holds more rows than the caller's cap
int check_state_header(const vbt_tracker* t, int clip, const StateHeader& h, int cap);

// n phases of 48 bytes from a packed record into phases6 + c * cap * 6, or VBT_ERR_CAPACITY ("<what> <id>: n phases, buffer holds cap")
int unpack_phases(const char* what, long long id, const unsigned char* src, int n, double* phases6, size_t c, int cap);
// the n <= cap metrics records (64 bytes each) that go with them, into metrics8 + c * cap * 8
inline void unpack_metrics(const unsigned char* src, int n, double* metrics8, size_t c, int cap) {
  if (n > 0) memcpy(metrics8 + c * cap * VT_METRICS, src, (size_t)n * VT_METRICS * sizeof(double));
}

}  // namespace vbt
