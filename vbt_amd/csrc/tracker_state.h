// A tracked clip's state as it sits in device memory - one layout under both trackers, OC-SORT and SORT - and the small pieces every
// unit of the tracker shares: the clip list of a launch, a fresh state, the export rule.  Plain structs and device code (tracker.hip
// holds the step kernels, tracker_analysis.hip the clip close, tracker_live.hip the live rep analysis; the host handle is tracker_host.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vbt_hip.h"
#include "lap.h"

namespace vbt {

constexpr int MAXD = VBT_MAX_DETECTIONS;
constexpr int MAXPH = 512;  // phases kept per clip

struct Trk {
  double x[7];
  double B[3][4];  // covariance blocks (a b; c d) of (cx,vcx) (cy,vcy) (s,vs)
  double Pr;       // variance of r
  double sx[7], sB[3][4], sPr;  // frozen copy (observation-centric re-update)
  double last_z[4];
  double last_obs[5];
  double vel[2];
  double obs[4][5];  // observations keyed by age & 3
  double conf, cls;
  double cum, cum_c, prev_x, prev_y;  // running path length of the emitted rows (export id selection)
  int obs_age[4];
  int has_saved, observed, gap, has_obs, has_vel;
  int time_since_update, id, hits, hit_streak, age, nrows;
};

struct Row {
  long long id;
  double time, x, y, dx, dy, h, w;
};

struct ClipState {
  int ntrk, frame_count, next_id, overflow, nrows, rows_overflow, best_id, last_n;
  double best_cum;
  int order[MAXT];
  unsigned long long used;  // slot bitmap
  double last_out[MAXD][9];  // last update(): x1,y1,x2,y2,id,cls,score,dx,dy
  Trk trk[MAXT];
};

struct TrackParams {
  int max_age, min_hits, delta_t, asso;
  double iou_thr, inertia, det_thresh;
};

// id_base: the first track of the clip gets row id id_base + 1 (0 for OC-SORT; vbt_sort_params.id_base for SORT)
__device__ inline void init_state(ClipState& st, int id_base = 0) {
  st.ntrk = 0; st.frame_count = 0; st.next_id = id_base; st.overflow = 0; st.nrows = 0; st.rows_overflow = 0;
  st.best_id = -1; st.last_n = 0; st.best_cum = -1.0; st.used = 0ull;
}

// A clip list in the kernel arguments (no host-to-device copy): block b works on clip[b]; n == 0 - no list - block b on clip b.  A
// longer list takes several launches of at most CLIP_LIST workgroups.
constexpr int CLIP_LIST = 64;
struct ClipList {
  int n;
  int clip[CLIP_LIST];
};
__device__ inline int listed_clip(const ClipList& l) { return l.n ? l.clip[blockIdx.x] : (int)blockIdx.x; }

// The export rule (reference track.py:107-115) applied to the clip as it stands: the largest cumulative path length among the ids
// with at least 2 rows - the dead ones are summed up in best_cum / best_id, the live ones compete here - ties to the lower id.
// -1: no id qualifies.  The clip close's export id and the live analysis' leader.
__device__ inline int export_id(const ClipState& st) {
  double bc = st.best_cum;
  int bi = st.best_id;
  for (int t = 0; t < st.ntrk; t++) {
    const Trk& k = st.trk[st.order[t]];
    if (k.nrows >= 2 && (k.cum > bc || (k.cum == bc && (bi < 0 || k.id + 1 < bi)))) { bc = k.cum; bi = k.id + 1; }
  }
  return bi;
}
// The same rule at the moment a track leaves the list (step_phases.h: retire): a finished track with at least 2 rows enters the dead
// ids' summary best_cum / best_id.  By ONE lane at a time: the deaths of a frame are serialised.
__device__ inline void finished_track_competes(ClipState& st, const Trk& k) {
  if (k.nrows >= 2 && (k.cum > st.best_cum || (k.cum == st.best_cum && k.id + 1 < st.best_id))) { st.best_cum = k.cum; st.best_id = k.id + 1; }
}

}  // namespace vbt
