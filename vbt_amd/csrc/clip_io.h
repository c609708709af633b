// What a step kernel does around the step itself: a frame's detections - from a detector slot or from the host - into the step's
// detection list (StepShared::det), and the clip state's copy between global memory and LDS.  Device code, included by tracker.hip.
#pragma once
#include "step_phases.h"

namespace vbt {

// One detector slot -> the tracker's detection list, lane i = detection i (the slot's 25 scores / boxes arrive in one
// round trip instead of 25 dependent ones by lane 0): threshold of reference odt.py:70-75 (score >= det_threshold), the
// reorder of odt.py:102-118 and OC-SORT's own gate (score > det_thresh), order kept.  Returns the number of detections
// handed to the tracker, or -1 when run_odt would have returned [] (the frame is skipped, track.py:180-181).  Uniform.
// The slot's count, this lane's score and this lane's box are requested TOGETHER (the count used to gate the score load and the score
// the box load: three dependent round trips at the head of every frame of a walk), and a walk requests frame f + 1's while it steps
// through frame f.
struct RawDet {
  int n;
  float s;
  float4 b;   // ymin,xmin,ymax,xmax
};
__device__ __forceinline__ RawDet fetch_slot_detections(const float* boxes, const float* scores, const int* counts, int slot, int lane) {
  const int l = min(lane, MAXD - 1);   // lanes past the 25 entries re-read the last one (never used)
  RawDet d;
  d.n = counts[slot];
  d.s = scores[slot * MAXD + l];
  d.b = *(const float4*)(boxes + ((size_t)slot * MAXD + l) * 4);
  return d;
}
__device__ __forceinline__ int put_slot_detections(StepShared& sh, const RawDet& d, float det_threshold, double det_thresh, int lane) {
  const int n = min(d.n, MAXD);
  const float s = lane < n ? d.s : 0.0f;
  const bool kept = lane < n && s >= det_threshold;
  const bool used = kept && (double)s > det_thresh;
  const unsigned long long mk = __ballot(kept), mu = __ballot(used);
  if (used) {
    const int m = __popcll(mu & ((1ull << lane) - 1ull));
    sh.det[m][0] = (double)d.b.y; sh.det[m][1] = (double)d.b.x; sh.det[m][2] = (double)d.b.w; sh.det[m][3] = (double)d.b.z;
    sh.det[m][4] = (double)s; sh.det[m][5] = 0.0;
  }
  return mk ? __popcll(mu) : -1;
}
__device__ inline int load_slot_detections(StepShared& sh, const float* boxes, const float* scores, const int* counts, int slot,
                                           float det_threshold, double det_thresh, int lane) {
  return put_slot_detections(sh, fetch_slot_detections(boxes, scores, counts, slot, lane), det_threshold, det_thresh, lane);
}

// Host-provided detections (rows of x1,y1,x2,y2,score,cls) -> the tracker's detection list, by ONE lane: dets = dets[confs > det_thresh],
// order kept.  Returns the number kept (0: the step still runs, on no detections).
__device__ __forceinline__ int put_host_detections(StepShared& sh, const double (*d)[6], int n, double det_thresh) {
  int m = 0;
  for (int i = 0; i < n && i < MAXD; i++)
    if (d[i][4] > det_thresh) { for (int j = 0; j < 6; j++) sh.det[m][j] = d[i][j]; m++; }
  return m;
}
// ... all of them, order kept (SORT has no score gate)
__device__ __forceinline__ int put_host_detections_all(StepShared& sh, const double (*d)[6], int n) {
  const int m = min(n, MAXD);
  for (int i = 0; i < m; i++)
    for (int j = 0; j < 6; j++) sh.det[i][j] = d[i][j];
  return m;
}

static_assert(sizeof(Trk) % 8 == 0 && offsetof(ClipState, trk) % 8 == 0, "8-byte copy granularity");
// The clip state between global memory and its LDS copy, by one wavefront: the header, then the LIVE tracks only.  All loads of a pass
// are in flight together (the header in one round trip, the tracks four words per lane at a time): the per-track loop it replaces
// waited for every 512 bytes - 5.8 us for ten tracks - which only a long run could amortise.  slots = 64 ints of LDS scratch.
template <bool TO_LDS>
__device__ inline void clip_state_copy(ClipState* lst, ClipState* gst, int* slots, int lane) {
  constexpr int HW = (int)(offsetof(ClipState, trk) / 8), HI = (HW + 63) / 64, TW = (int)(sizeof(Trk) / 8);
  unsigned long long* l = (unsigned long long*)lst;
  unsigned long long* g = (unsigned long long*)gst;
  {
    unsigned long long hv[HI];
#pragma unroll
    for (int k = 0; k < HI; k++) { const int i = min(lane + 64 * k, HW - 1); hv[k] = TO_LDS ? g[i] : l[i]; }
#pragma unroll
    for (int k = 0; k < HI; k++) { const int i = lane + 64 * k; if (i < HW) (TO_LDS ? l : g)[i] = hv[k]; }
  }
  __syncthreads();
  const unsigned long long used = lst->used;
  if ((used >> lane) & 1ull) slots[__popcll(used & ((1ull << lane) - 1ull))] = lane;
  __syncthreads();
  const int total = __popcll(used) * TW;
  unsigned long long* lt = (unsigned long long*)&lst->trk[0];
  unsigned long long* gt = (unsigned long long*)&gst->trk[0];
  for (int base = 0; base < total; base += 256) {
    unsigned long long v[4];
    int off[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int i = min(base + lane + 64 * k, total - 1);
      const int ord = i / TW, w = i - ord * TW;
      off[k] = slots[ord] * TW + w;
      v[k] = TO_LDS ? gt[off[k]] : lt[off[k]];
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (base + lane + 64 * k < total) (TO_LDS ? lt : gt)[off[k]] = v[k];
  }
  __syncthreads();
}

}  // namespace vbt
