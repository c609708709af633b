// vbt_pipeline: the clip loop of reference track.py:129-260 as one object behind the C ABI (include/vbt_hip.h, "pipeline").
//
// Host code only - every kernel it enqueues is reached through the library's own entry points (vbt_detect_async,
// vbt_tracker_update_from_*; the slot close through tracker_close_clips, common.h).  What lives here is the scheduling part of the fast
// path: which stream a forward runs on and that the busy streams sit on distinct hardware queues, the ring of output slots and the
// events that order detector(t) -> tracker(t) -> slot reuse, the deferred tracker groups of the small-batch path and the step groups of
// the large-batch path (one forward of G x n images behind G step calls) as one held-back block, clip close.  How a step's frames get
// to the network resolution - the staging ring of the host-fed mode, the upload, the pixel formats, the resize - is the Ingest object
// of pipeline_ingest.h, which this unit only hands the step's sources to; the stream pool is stream_pool.h, the run lists of a block's
// walk walk_runs.h.  Every device buffer, pinned buffer and event is held by an owner (dev_mem.h, hip_handles.h) and goes with the
// handle; the streams are borrowed from the pool.  No framework allocator, no framework streams.
#include <algorithm>
#include <chrono>

#include "common.h"
#include "dev_mem.h"
#include "hip_handles.h"
#include "pipeline_ingest.h"
#include "stream_pool.h"
#include "walk_runs.h"

using namespace vbt;

struct vbt_pipeline {
  vbt_pipeline_params prm{};
  int n = 0, n_trk = 0, depth = 0, ring = 0, defer = 0, device = 0;
  bool trk_inline = false, placement_ok = true;
  bool live = false;               // vbt_pipeline_live_enable succeeded
  bool rep_metrics = false;        // vbt_pipeline_rep_metrics_enable succeeded
  std::vector<double> fps;
  // detector outputs: one array per tensor, [ring slot][batch slot]...: the walk of a block addresses batch slot i of its step g as slot g * n + i
  DevBuf<float> boxes, scores, classes;
  DevBuf<int32_t> counts;
  // What the tracker needs to know about the step in a ring slot.  vbt_pipeline_step (fill_step): per batch slot the tracker clip (-1: none)
  // and the 1-based frame number of that clip; vbt_pipeline_step_runs: the runs to walk, and then clip / frame are not read.
  struct Step {
    int B = 0, fc = 0, track = 1;   // batch slots used; frame_count at the step; 0: detector only, never walked
    bool mapped = false;            // the step came with a clip map: its single-step launch is vbt_tracker_update_from_slots
    std::vector<int32_t> clip, frame;
    std::vector<vbt_run> runs;
  };
  std::vector<Step> meta;
  // The held-back block: `used` steps in ring slots o0 .. o0 + used - 1 whose OC-SORT walk goes out as one time-batched launch (flush_block).
  //  - Step group (G > 1): the steps share ONE forward of detector instance k.  Every call runs the network entry (resize / upload + the
  //    plan steps that read the frames) on its own n images at once, into slice g of the G n-image tensors; the flush enqueues the rest of
  //    the plan at batch used * n, whose decode + NMS fills the block's ring slots.
  //  - Deferred tracker steps (G == 1, defer > 0, plain steps only): every step ran its whole forward on its own stream; k is the
  //    forward slot of the last one.
  struct Block { int o0 = 0, used = 0, k = 0; } blk;
  std::vector<int> pending;        // own-stream tracker: steps whose launch lags the detector, oldest first (never together with a block)
  std::vector<int> own_streams;
  std::vector<double> times;                      // scratch of a single-step launch
  std::vector<std::vector<WalkFrame>> walk_per;   // scratch of flush_block: per tracker clip its frames in the block
  std::vector<size_t> walk_cur;
  std::vector<vbt_run> walk_runs;
  hipStream_t det_streams[8] = {nullptr}, trk_stream = nullptr;
  std::vector<Event> ev_det, ev_trk;
  std::vector<int> trk_ev_of;      // ring slot -> index into ev_trk of the tracker launch that read it last (-1: none)
  int last_trk = -1;               // index into ev_trk of the most recent tracker launch
  Ingest ingest;                   // frames in: staging ring, copy stream, pixel format, resize (pipeline_ingest.h)
  std::vector<int64_t> clip_frames;
  int frame_count = 0, step_idx = 0, last_B = 0;
  bool ever_stepped = false;       // a step was enqueued on this handle (not cleared by a reset): vbt_pipeline_use_sort comes too late
  int G = 1;                      // steps per forward (vbt_pipeline_params.group)
  int next_o = 0, fwd_idx = 0;     // G > 1: ring slot of the next forward's first step (a block never wraps); forwards opened since creation / reset
  int last_o = 0, last_k = 0;      // ring slot / forward slot of the most recent step
  uint64_t step_host_ns = 0, step_calls = 0;
  // slot close (vbt_pipeline_close_clips): per tracker clip its record (pinned, CLOSED_HEAD_BYTES), its rows (device, rows_cap rows) and
  // the event of its close; allocated by vbt_pipeline_close_clips_enable.  fc_base: frame_count when the slot last reopened (plain steps count from it)
  PinnedBuf<unsigned char> closed_head;
  unsigned char* closed_head_dev = nullptr;   // (its device address)
  PinnedBuf<unsigned char> closed_metrics;    // rep metrics on: per tracker clip the metrics of its record's phases (CLOSED_METRICS_BYTES)
  double* closed_metrics_dev = nullptr;
  DevBuf<unsigned char> closed_rows;
  std::vector<Event> ev_closed;
  std::vector<char> closed_unread;
  std::vector<int> fc_base;
  hipStream_t read_stream = nullptr;   // the rows of a closed slot come back on it (a pool stream that carries nothing else)
  // declared last, so destroyed first: the models and the tracker go before the rings and events their launches used
  struct ModelDelete { void operator()(vbt_model* m) const { vbt_model_destroy(m); } };
  struct TrackerDelete { void operator()(vbt_tracker* t) const { vbt_tracker_destroy(t); } };
  std::unique_ptr<vbt_tracker, TrackerDelete> trk;
  std::vector<std::unique_ptr<vbt_model, ModelDelete>> models;
  ~vbt_pipeline();
};

namespace {

// host time of a step call, for vbt_pipeline_info (is the host or the GPU pacing a small-batch run?)
struct StepTimer {
  vbt_pipeline* p;
  std::chrono::steady_clock::time_point t0;
  explicit StepTimer(vbt_pipeline* p_) : p(p_), t0(std::chrono::steady_clock::now()) {}
  ~StepTimer() {
    p->step_host_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    p->step_calls++;
  }
};

// ---- output ring ----
inline float* boxes_of(vbt_pipeline* p, int o) { return p->boxes.get() + (size_t)o * p->n * VBT_MAX_DETECTIONS * 4; }
inline float* scores_of(vbt_pipeline* p, int o) { return p->scores.get() + (size_t)o * p->n * VBT_MAX_DETECTIONS; }
inline float* classes_of(vbt_pipeline* p, int o) { return p->classes.get() + (size_t)o * p->n * VBT_MAX_DETECTIONS; }
inline int32_t* counts_of(vbt_pipeline* p, int o) { return p->counts.get() + (size_t)o * p->n; }

int record_trk(vbt_pipeline* p, int o, hipStream_t T) {
  VBT_HIP_CHECK(hipEventRecord(p->ev_trk[o].get(), T));
  p->trk_ev_of[o] = o;
  p->last_trk = o;
  return VBT_OK;
}

// Work enqueued on the tracker stream T outside a step (the slot close with its reset, the update of a live panel) becomes the most
// recent tracker launch: the event of the last launch is recorded again behind it, so every later tracker launch - each waits for
// ev_trk[last_trk], or runs on the tracker stream itself - and whoever else waits for that event comes after it.
int rerecord_trk(vbt_pipeline* p, hipStream_t T) {
  const int e = p->last_trk >= 0 ? p->last_trk : 0;
  VBT_HIP_CHECK(hipEventRecord(p->ev_trk[(size_t)e].get(), T));
  p->last_trk = e;
  return VBT_OK;
}

// Ring slot and forward slot (model instance, stream) of the next step.  Ungrouped: the ring in order.  Grouped: a block continues
// while one is open, else the next forward starts at next_o.
void next_slots(const vbt_pipeline* p, int* o, int* k) {
  if (p->G == 1) {
    *o = p->step_idx % p->ring;
    *k = *o % p->depth;
  } else if (p->blk.used > 0) {
    *o = p->blk.o0 + p->blk.used;
    *k = p->blk.k;
  } else {
    *o = p->next_o;
    *k = p->fwd_idx % p->depth;
  }
}

// The step record of a vbt_pipeline_step call (frame_count already counts the step)
void fill_step(vbt_pipeline* p, vbt_pipeline::Step& m, const uint8_t* active, const int32_t* clip_map, const int32_t* frame_idx, int track) {
  m.B = p->n;
  m.fc = p->frame_count;
  m.track = track;
  m.mapped = clip_map != nullptr;
  m.runs.clear();
  for (int i = 0; i < p->n; i++) {
    if (clip_map) {
      m.clip[i] = clip_map[i];
      m.frame[i] = frame_idx[i];
    } else if (!active) {   // frame_count / fps (track.py:169), counted from the slot's last reopen; slots past the last clip carry none
      m.clip[i] = i < p->n_trk ? i : -1;
      m.frame[i] = i < p->n_trk ? p->frame_count - p->fc_base[(size_t)i] : 0;
    } else if (active[i]) {
      m.clip[i] = i;
      m.frame[i] = (int)++p->clip_frames[(size_t)i];
    } else {
      m.clip[i] = -1;
    }
  }
}

// The OC-SORT launch of the one step in ring slot o: on the tracker stream after the slot's detections ("own"), or at the end of the
// slot's own stream after the previous tracker launch ("inline": stream order gives "after this slot's detections")
int enqueue_tracker(vbt_pipeline* p, int o) {
  hipStream_t T;
  if (p->trk_inline) {
    T = p->det_streams[o % p->depth];
    if (p->last_trk >= 0) VBT_HIP_CHECK(hipStreamWaitEvent(T, p->ev_trk[p->last_trk].get(), 0));   // tracker steps run in frame order
  } else {
    T = p->trk_stream;
    VBT_HIP_CHECK(hipStreamWaitEvent(T, p->ev_det[o].get(), 0));
  }
  const vbt_pipeline::Step& m = p->meta[o];
  // frame times / clip map / runs of the step travel in the kernel arguments (read during the call, no copy in flight)
  if (!m.runs.empty()) {
    PL_CHECK(vbt_tracker_update_from_detections_seq(p->trk.get(), boxes_of(p, o), scores_of(p, o), counts_of(p, o), m.B, m.runs.data(), (int)m.runs.size(),
                                                    p->prm.detection_threshold, (void*)T));
    return record_trk(p, o, T);
  }
  // time = frame number / fps of the clip; fps cannot have changed since the step: a slot close drains before it sets a new one
  for (int i = 0; i < p->n; i++) p->times[i] = m.clip[i] >= 0 ? (double)m.frame[i] / p->fps[m.clip[i]] : -1.0;
  if (m.mapped) {
    PL_CHECK(vbt_tracker_update_from_slots(p->trk.get(), boxes_of(p, o), scores_of(p, o), counts_of(p, o), m.clip.data(), p->times.data(), p->n,
                                           p->prm.detection_threshold, (void*)T));
  } else {   // (reads the first n_trk slots: slot i is clip i)
    PL_CHECK(vbt_tracker_update_from_detections(p->trk.get(), boxes_of(p, o), scores_of(p, o), counts_of(p, o), p->times.data(), p->prm.detection_threshold,
                                                (void*)T));
  }
  return record_trk(p, o, T);
}

int wait_slot_free(vbt_pipeline* p, int o, hipStream_t S) {
  const bool held = o >= p->blk.o0 && o < p->blk.o0 + p->blk.used;
  if (held || std::find(p->pending.begin(), p->pending.end(), o) != p->pending.end()) {
    set_error("vbt_pipeline: ring slot %d still holds a step whose tracker update has not been enqueued", o);
    return VBT_ERR_STATE;
  }
  if (p->trk_ev_of[o] >= 0) VBT_HIP_CHECK(hipStreamWaitEvent(S, p->ev_trk[p->trk_ev_of[o]].get(), 0));   // the tracker is done with this slot's previous outputs
  return VBT_OK;
}

// Hands the held-back block to the GPU.  A step group first gets the rest of its forward.  Then the walk of the block's tracked steps in
// frame order: one launch of the time-batched walk (walk_runs.h; a further one only where a clip's frames break their pattern), on the
// stream of the block's last forward when the tracker runs inline, else on the tracker stream, after the block's other forwards and the
// previous tracker launch.  A single deferred step is an ordinary single-step launch.
//
// Who calls what.
//  - flush_block: the step that fills the block, a step that cannot join it (step_frames), and whatever launches tracker work of its own,
//    so that tracker launches stay in frame order: vbt_pipeline_step_runs (vbt_track_clip with it), vbt_pipeline_tracker_only_steps.
//  - drain: what reads or replaces tracker state - reset, drain, finish, close, close_clips, rows, rows_all, live_poll.  It also needs the
//    own-stream lag enqueued and, with the inline tracker, the tracker stream behind the last launch.
//  - finish_forward: what only needs the detections or the frame counter of the steps so far - detections, join_detectors, closed_clip,
//    skip_frames, set_frame_count, destroy.  A step group's forward is completed (its walk goes with it).  Deferred steps stay deferred:
//    their detections are in the ring already, and skipped frames between them are a frame step the walk carries (step_frames flushes
//    when the step changes inside a block).
int flush_block(vbt_pipeline* p) {
  const vbt_pipeline::Block b = p->blk;
  if (b.used == 0) return VBT_OK;
  p->blk.used = 0;
  const int n = p->n, o0 = b.o0, used = b.used, o_last = o0 + used - 1;
  const bool grouped = p->G > 1;
  auto fwd_slot = [&](int g) { return grouped ? b.k : (o0 + g) % p->depth; };
  if (grouped) {
    hipStream_t S = p->det_streams[b.k];
    for (int g = 0; g < used; g++) PL_CHECK(wait_slot_free(p, o0 + g, S));
    vbt_model* m = p->models[(size_t)b.k].get();
    PL_CHECK(vbt_detect_range_async(m, nullptr, 0, used * n, vbt_model_entry_steps(m), -1, (void*)S, boxes_of(p, o0), scores_of(p, o0), classes_of(p, o0),
                                    counts_of(p, o0)));
    for (int g = 0; g < used; g++) VBT_HIP_CHECK(hipEventRecord(p->ev_det[o0 + g].get(), S));
  } else if (used == 1) {
    return enqueue_tracker(p, o0);
  }
  bool any = false;
  for (auto& v : p->walk_per) v.clear();
  for (int g = 0; g < used; g++) {
    const vbt_pipeline::Step& sm = p->meta[(size_t)(o0 + g)];
    if (!sm.track) continue;
    for (int i = 0; i < n; i++)
      if (sm.clip[i] >= 0) { p->walk_per[(size_t)sm.clip[i]].push_back(WalkFrame{g * n + i, sm.frame[i]}); any = true; }
  }
  if (!any) return VBT_OK;
  hipStream_t T = p->trk_inline ? p->det_streams[b.k] : p->trk_stream;
  for (int g = 0; g < used; g++) {   // the last forward of every other stream in the block
    bool last = p->det_streams[fwd_slot(g)] != T;
    for (int h = g + 1; h < used && last; h++) last = fwd_slot(h) != fwd_slot(g);
    if (last) VBT_HIP_CHECK(hipStreamWaitEvent(T, p->ev_det[o0 + g].get(), 0));
  }
  if (p->last_trk >= 0) VBT_HIP_CHECK(hipStreamWaitEvent(T, p->ev_trk[p->last_trk].get(), 0));   // tracker launches run in frame order
  // (a slot close drains first: fps and the frame bases are those of the whole block)
  std::fill(p->walk_cur.begin(), p->walk_cur.end(), (size_t)0);
  while (next_walk_call(p->walk_per, p->fps.data(), p->walk_cur, p->walk_runs))
    PL_CHECK(vbt_tracker_update_from_detections_seq(p->trk.get(), boxes_of(p, o0), scores_of(p, o0), counts_of(p, o0), used * n, p->walk_runs.data(),
                                                    (int)p->walk_runs.size(), p->prm.detection_threshold, (void*)T));
  VBT_HIP_CHECK(hipEventRecord(p->ev_trk[o_last].get(), T));
  for (int g = 0; g < used; g++) p->trk_ev_of[o0 + g] = o_last;
  p->last_trk = o_last;
  return VBT_OK;
}

int finish_forward(vbt_pipeline* p) {
  if (p->G == 1 || p->blk.used == 0) return VBT_OK;
  VBT_HIP_CHECK(hipSetDevice(p->device));
  return flush_block(p);
}

// own stream: the tracker stays up to `keep` steps behind the detector
int enqueue_lagging(vbt_pipeline* p, int keep) {
  while ((int)p->pending.size() > keep) {
    const int o = p->pending.front();
    p->pending.erase(p->pending.begin());
    PL_CHECK(enqueue_tracker(p, o));
  }
  return VBT_OK;
}

int drain(vbt_pipeline* p) {
  PL_CHECK(flush_block(p));
  PL_CHECK(enqueue_lagging(p, 0));
  if (p->trk_inline && p->last_trk >= 0)   // clip close / row reads run on the tracker stream
    VBT_HIP_CHECK(hipStreamWaitEvent(p->trk_stream, p->ev_trk[p->last_trk].get(), 0));
  return VBT_OK;
}

// The end of a run: everything held back goes out, then export id + rep analysis of every clip on the tracker stream.  Enqueue only.
int drain_and_finish(vbt_pipeline* p) {
  VBT_HIP_CHECK(hipSetDevice(p->device));
  PL_CHECK(drain(p));
  return vbt_tracker_finish(p->trk.get(), p->prm.plate_diameter, p->prm.diff_threshold, p->prm.min_distance, (void*)p->trk_stream);
}

// The front of every step in ring slot o / forward slot k: the slot's previous outputs are free (`wait`: the step writes the slot now
// - a member of a step group writes it at the flush, flush_block waits there), the counters, B frames at the network resolution.
int begin_step(vbt_pipeline* p, int o, int k, bool wait, bool counts_frame, const Sources& src, const vbt_run* asm_runs, int n_asm, int B,
               void* caller_stream, const uint8_t** frames_dev, int* stage_j) {
  hipStream_t S = p->det_streams[k];
  if (wait) PL_CHECK(wait_slot_free(p, o, S));
  if (p->G > 1) {   // the forward this step opens or joins; a block never wraps
    if (p->blk.used == 0) p->fwd_idx++;
    p->next_o = o + 1 + p->G > p->ring ? 0 : o + 1;
  }
  p->step_idx++;
  p->ever_stepped = true;
  if (counts_frame) p->frame_count++;
  p->last_o = o;
  p->last_k = k;
  p->last_B = B;
  return p->ingest.prepare(k, S, src, asm_runs, n_asm, B, caller_stream, frames_dev, stage_j);
}

// Behind the last kernel that reads the step's frames on S: the detections of ring slot o are complete (o < 0: not yet, the entry of
// a step group), the staging buffer is free again
int end_detect(vbt_pipeline* p, int o, int stage_j, hipStream_t S) {
  if (o >= 0) VBT_HIP_CHECK(hipEventRecord(p->ev_det[o].get(), S));
  return p->ingest.frames_read(stage_j, S);
}

// The tracker launch of a step that is not held back: inline right behind its forward, own stream depth - 1 detector steps behind
int launch_or_lag(vbt_pipeline* p, int o) {
  p->pending.push_back(o);
  return enqueue_lagging(p, p->trk_inline ? 0 : p->depth - 1);
}

// One time-batched step: `asm_runs` say where the sources sit in the batch (assembly), `walk_runs` what the tracker walks.  On a grouped
// pipeline it is a forward of its own between the step groups.
int step_runs_impl(vbt_pipeline* p, const Sources& src, const vbt_run* asm_runs, int n_asm, std::vector<vbt_run>& walk_runs, int B, int track,
                   float* out_boxes, float* out_scores, float* out_classes, int32_t* out_counts, void* caller_stream) {
  PL_CHECK(flush_block(p));
  int o = 0, k = 0;
  next_slots(p, &o, &k);
  hipStream_t S = p->det_streams[k];
  const uint8_t* fd = nullptr;
  int stage_j = -1;
  PL_CHECK(begin_step(p, o, k, true, false, src, asm_runs, n_asm, B, caller_stream, &fd, &stage_j));
  const bool outs = out_boxes != nullptr;
  float* b = outs ? out_boxes : boxes_of(p, o);
  float* s = outs ? out_scores : scores_of(p, o);
  float* c = outs ? out_classes : classes_of(p, o);
  int32_t* cnt = outs ? out_counts : counts_of(p, o);
  PL_CHECK(vbt_detect_async(p->models[k].get(), fd, B, (void*)S, b, s, c, cnt));
  PL_CHECK(end_detect(p, o, stage_j, S));
  vbt_pipeline::Step& m = p->meta[o];
  m.runs.swap(walk_runs);
  m.B = B;
  m.track = track;
  return track ? launch_or_lag(p, o) : VBT_OK;
}

// vbt_pipeline_step (arguments checked by the caller).  Everything that touches the caller's frames happens in the call, stream-ordered: the
// wait for the caller's stream, upload, resize / conversion and - step group - the network entry, else the whole forward; what a step
// group holds back reads the model's own tensors only.  There is no ramp: groups of one for the first `depth` forwards measured slower
// over a 20-step run than full groups from the first step (profiles/r07_step_groups_ab.md).
int step_frames(vbt_pipeline* p, const Sources& src, const uint8_t* active, const int32_t* clip_map, const int32_t* frame_idx, int track,
                void* caller_stream) {
  const int n = p->n;
  const bool grouped = p->G > 1, plain = !clip_map && !active && track;
  if (grouped && clip_map)   // (the walk of a block takes a clip once per step)
    for (int i = 0; i < n; i++)
      for (int j = 0; j < i; j++)
        if (clip_map[i] >= 0 && clip_map[i] == clip_map[j]) { set_error("vbt_pipeline_step: clip %d sits in two slots", clip_map[i]); return VBT_ERR_ARG; }
  int o = 0, k = 0;
  next_slots(p, &o, &k);
  if (!grouped && p->blk.used > 0) {
    // deferred steps go out before a step that cannot join them: another kind of step, a ring wrap, or skip_frames() changed the frame stride
    const int o0 = p->blk.o0, last = o0 + p->blk.used - 1;
    if (!plain || o <= last || (p->blk.used >= 2 && p->frame_count + 1 - p->meta[last].fc != p->meta[o0 + 1].fc - p->meta[o0].fc)) PL_CHECK(flush_block(p));
  }
  hipStream_t S = p->det_streams[k];
  const uint8_t* fd = nullptr;
  int stage_j = -1;
  PL_CHECK(begin_step(p, o, k, !grouped, true, src, nullptr, 0, n, caller_stream, &fd, &stage_j));
  fill_step(p, p->meta[(size_t)o], active, clip_map, frame_idx, track);
  vbt_model* mdl = p->models[(size_t)k].get();
  if (grouped) {   // the entry on slice `used` of the forward; it was the staging buffer's only reader
    PL_CHECK(vbt_detect_range_async(mdl, fd, p->blk.used * n, n, 0, vbt_model_entry_steps(mdl), (void*)S, nullptr, nullptr, nullptr, nullptr));
    PL_CHECK(end_detect(p, -1, stage_j, S));
  } else {
    PL_CHECK(vbt_detect_async(mdl, fd, n, (void*)S, boxes_of(p, o), scores_of(p, o), classes_of(p, o), counts_of(p, o)));
    PL_CHECK(end_detect(p, o, stage_j, S));
  }
  if (grouped || (p->defer && plain)) {   // held back; deferred blocks are aligned to `defer` ring slots, so neither kind wraps
    if (p->blk.used == 0) p->blk.o0 = o;
    p->blk.k = k;
    p->blk.used++;
    if (grouped ? p->blk.used >= p->G : (p->blk.used >= p->defer || o % p->defer == p->defer - 1)) PL_CHECK(flush_block(p));
    return VBT_OK;
  }
  return track ? launch_or_lag(p, o) : VBT_OK;   // (track == 0: detector-only step, measurement splits)
}

}  // namespace

// Also the end of a create that fails half way: streams not taken yet are null, models not made yet are absent.
vbt_pipeline::~vbt_pipeline() {
  (void)hipSetDevice(device);
  (void)finish_forward(this);   // (the models' tensors are released below: nothing half-run stays behind)
  for (int k = 0; k < depth; k++)
    if (det_streams[k]) (void)hipStreamSynchronize(det_streams[k]);
  if (ingest.stream()) (void)hipStreamSynchronize(ingest.stream());
  if (trk_stream) (void)hipStreamSynchronize(trk_stream);
  {
    // streams are never destroyed: they go back to the process-wide pool, classified, for the next pipeline
    std::lock_guard<std::mutex> lock(g_pool_mu);
    StreamPool& pool = g_pools[device];
    for (int i : own_streams) pool.free.push_back(i);
  }
  // the members go in reverse order of declaration: the models and the tracker first, then the slot-close buffers, the rings, the events
}

extern "C" {

void vbt_pipeline_default_params(vbt_pipeline_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->defer = -1;
  p->selfcheck = -1;
  p->strict_placement = -1;
  p->model_flags = VBT_MODEL_DEFAULT_FLAGS;
  p->detection_threshold = 0.5f;
  p->plate_diameter = 0.45;
  p->diff_threshold = 0.6;
  p->min_distance = 0.1;
  p->tracker.max_age = 30;
  p->tracker.min_hits = 3;
  p->tracker.delta_t = 3;
  p->tracker.asso = 1;
  p->tracker.iou_threshold = 0.1;
  p->tracker.inertia = 0.2;
  p->tracker.det_thresh = 0.2;
}

void vbt_pipeline_destroy(vbt_pipeline* p) { delete p; }

int vbt_pipeline_create(const char* container_path, const vbt_pipeline_params* prm, const double* fps_host, vbt_pipeline** out) {
  if (!container_path || !prm || !fps_host || !out) { set_error("vbt_pipeline_create: NULL argument"); return VBT_ERR_ARG; }
  *out = nullptr;
  if (prm->n_slots < 1 || prm->n_clips < 0 || prm->rows_cap < 1 || prm->depth < 0 || prm->depth > 8 || prm->device < 0 || prm->device >= 64 ||
      prm->group < 0 || prm->group > 8) {
    set_error("vbt_pipeline_create: n_slots >= 1, n_clips >= 0, rows_cap >= 1, depth 0..8, group 0..8 required");
    return VBT_ERR_ARG;
  }
  if (int rc = use_device("vbt_pipeline_create", prm->device)) return rc;
  std::unique_ptr<vbt_pipeline> owner(new vbt_pipeline());
  vbt_pipeline* const p = owner.get();
  p->prm = *prm;
  p->n = prm->n_slots;
  p->n_trk = prm->n_clips > 0 ? prm->n_clips : prm->n_slots;
  p->device = prm->device;
  for (int c = 0; c < p->n_trk; c++) {
    if (!(fps_host[c] > 0.0)) { set_error("vbt_pipeline_create: fps of clip %d must be > 0", c); return VBT_ERR_ARG; }
    p->fps.push_back(fps_host[c]);
  }
  p->fc_base.assign((size_t)p->n_trk, 0);
  // forwards in flight: 3 at batch 64 (four hardware queues: three forwards + the copy stream); a batch of one to
  // eight frames is launch latency, where a fourth forward still pays
  p->depth = prm->depth > 0 ? prm->depth : env_int("VBT_PIPELINE_DEPTH", p->n <= 8 ? 4 : 3);
  p->depth = std::max(1, std::min(p->depth, 8));
  int mode = prm->tracker_stream;
  if (mode == 0) {
    const char* ts = getenv("VBT_TRACKER_STREAM");
    if (ts && strcmp(ts, "own") != 0 && strcmp(ts, "inline") != 0) { set_error("VBT_TRACKER_STREAM must be 'own' or 'inline'"); return VBT_ERR_ARG; }
    mode = ts ? (strcmp(ts, "inline") == 0 ? 2 : 1) : (p->depth >= 3 ? 2 : 1);
  }
  p->trk_inline = mode == 2;
  // Deferred tracker steps (small batches): one single-wave tracker launch plus its cross-stream event at the end of EVERY forward
  // costs a fifth of a batch-1 step; with deferral the detections of `depth` consecutive steps stay in a ring of 2 x depth output
  // slots and ONE launch of the time-batched walk follows the group's last forward.  Only plain steps are deferred.
  const bool defer_ok = p->n_trk == p->n && p->depth >= 2 && p->trk_inline;
  int want = prm->defer >= 0 ? prm->defer : env_int("VBT_TRACKER_DEFER", (p->n <= 8 && p->n_trk == p->n && p->depth >= 2) ? 1 : 0);
  p->defer = (want == 1 && defer_ok) ? p->depth : 0;
  // Step groups: at 32..64 images the low-resolution half of the network runs grids too small for the GPU, launch after launch; a forward
  // of 4 x n images runs the same launches once per four steps on grids four times as wide.  Default only where the plan of that batch
  // is at hand - a pinned plan file, or no autotuning - so that no pipeline that reads a pinned plan today tunes a new one at creation.
  {
    int g = prm->group;
    if (g == 0) {
      bool planned = (prm->model_flags & VBT_MODEL_NO_AUTOTUNE) != 0;
      if (const char* pf = getenv("VBT_PLAN_FILE")) {
        char path[1024];
        snprintf(path, sizeof(path), "%s.b%d.f%d", pf, 4 * p->n, prm->model_flags);
        if (FILE* f = fopen(path, "r")) { planned = true; fclose(f); }
      }
      g = (p->n >= 32 && p->n <= 64 && planned) ? 4 : 1;
    }
    g = env_int("VBT_PIPELINE_GROUP", g);
    p->G = p->n_trk == p->n ? std::max(1, std::min(g, 8)) : 1;
  }
  if (p->G > 1) p->defer = 0;
  p->ring = p->G > 1 ? (p->depth + 1) * p->G : p->defer ? 2 * p->depth : p->depth;
  int rc = VBT_OK;
  for (int k = 0; k < p->depth; k++) {
    vbt_model* m = nullptr;
    if ((rc = vbt_model_create_ex(container_path, p->device, p->G * p->n, prm->model_flags, &m)) != VBT_OK) return rc;
    p->models.emplace_back(m);
  }
  int shp[4];
  if ((rc = vbt_model_input_shape(p->models[0].get(), shp)) != VBT_OK) return rc;
  const int size = shp[1];
  {
    vbt_tracker* t = nullptr;
    if ((rc = vbt_tracker_create(p->n_trk, prm->rows_cap, &prm->tracker, p->device, &t)) != VBT_OK) return rc;
    p->trk.reset(t);
  }
  const size_t R = (size_t)p->ring, n = (size_t)p->n, md = VBT_MAX_DETECTIONS;
  if (p->boxes.alloc(R * n * md * 4) != hipSuccess || p->scores.alloc(R * n * md) != hipSuccess || p->classes.alloc(R * n * md) != hipSuccess ||
      p->counts.alloc(R * n) != hipSuccess) {
    set_error("vbt_pipeline_create: hipMalloc of the detector output ring failed");
    return VBT_ERR_HIP;
  }
  (void)hipMemset(p->counts.get(), 0, R * n * 4);
  p->meta.resize(R);
  for (auto& m : p->meta) { m.clip.assign(n, -1); m.frame.assign(n, 0); }
  p->times.assign(n, 0.0);
  p->walk_per.resize((size_t)p->n_trk);
  p->walk_cur.resize((size_t)p->n_trk);
  p->trk_ev_of.assign(R, -1);
  auto new_events = [&](std::vector<Event>& v, size_t cnt) {
    v.resize(cnt);
    for (Event& e : v)
      if (e.create(hipEventDisableTiming) != hipSuccess) return false;
    return true;
  };
  if (!new_events(p->ev_det, R) || !new_events(p->ev_trk, R) || !p->ingest.create(p->depth, p->n, size)) {
    set_error("vbt_pipeline_create: hipEventCreate failed");
    return VBT_ERR_HIP;
  }
  p->clip_frames.assign(n, 0);
  {
    // the pipeline's own HIP streams (detector slots, copy, tracker): each is bound to its hardware queue at creation
    // (vbt_stream_create); then checked pair by pair
    std::lock_guard<std::mutex> lock(g_pool_mu);
    StreamPool& pool = g_pools[p->device];
    int role_idx[10] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    for (int k = 0; k < p->depth && rc == VBT_OK; k++) rc = pool_take(pool, p->device, p->own_streams, -1, false, &role_idx[k]);
    if (rc == VBT_OK) rc = pool_take(pool, p->device, p->own_streams, -1, false, &role_idx[8]);
    if (rc == VBT_OK) rc = pool_take(pool, p->device, p->own_streams, -1, false, &role_idx[9]);
    // busy: the streams that carry kernels side by side - the detector slots, the copy stream (four hardware queues: with four forwards in
    // flight it has to share one, which costs a small batch nothing), the tracker stream unless its step runs inline
    std::vector<int> busy;
    for (int k = 0; k < p->depth; k++) busy.push_back(k);
    if (p->depth < 4) busy.push_back(8);
    if (!p->trk_inline) busy.push_back(9);
    const bool strict = (prm->strict_placement >= 0 ? prm->strict_placement : env_int("VBT_STRICT_PLACEMENT", 0)) == 1;
    if (rc == VBT_OK) rc = place_streams(pool, p->device, busy, strict, role_idx, p->own_streams, &p->placement_ok);
    if (rc == VBT_OK) {
      for (int k = 0; k < p->depth; k++) p->det_streams[k] = pool.streams[role_idx[k]];
      p->ingest.set_stream(pool.streams[role_idx[8]]);
      p->trk_stream = pool.streams[role_idx[9]];
    }
  }
  if (rc != VBT_OK) return rc;
  // Self-check: every slot runs its whole plan on a blank batch before the first real frame, so a plan the kernels reject (LDS
  // budget, tile shape) fails here and not in the middle of a clip; the first real step then also finds code objects, arenas and
  // GPU clocks warm.  Detector only: no tracker state is touched.
  const int n_check = prm->selfcheck >= 0 ? prm->selfcheck : env_int("VBT_PIPELINE_SELFCHECK", 1);
  if (n_check > 0) {
    DevBuf<uint8_t> blank;   // (freed when the block ends, behind the synchronisation of every forward that read it)
    const size_t bytes = (size_t)p->G * n * size * size * 3;   // (a grouped pipeline checks the batch its forwards run at)
    if (blank.alloc(bytes + 64) != hipSuccess) { set_error("vbt_pipeline_create: hipMalloc of the self-check batch failed"); return VBT_ERR_HIP; }
    (void)hipMemset(blank.get(), 0, bytes);
    (void)hipDeviceSynchronize();
    for (int i = 0; i < n_check && rc == VBT_OK; i++)
      for (int k = 0; k < p->depth && rc == VBT_OK; k++)
        rc = vbt_detect_async(p->models[k].get(), blank.get(), p->G * p->n, (void*)p->det_streams[k], boxes_of(p, k * p->G), scores_of(p, k * p->G),
                              classes_of(p, k * p->G), counts_of(p, k * p->G));
    hipError_t e = hipSuccess;
    for (int k = 0; k < p->depth; k++) {
      const hipError_t ek = hipStreamSynchronize(p->det_streams[k]);
      if (e == hipSuccess) e = ek;
    }
    if (rc != VBT_OK) return rc;
    if (e != hipSuccess) { set_error("vbt_pipeline_create: self-check forward failed: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
  }
  *out = owner.release();
  return VBT_OK;
}

int vbt_pipeline_step(vbt_pipeline* p, const uint8_t* frames, int frames_on_device, int src_h, int src_w, int swap_rb, const uint8_t* active,
                      const int32_t* clip_map, const int32_t* frame_idx, int track, void* caller_stream) {
  if (!p || !frames) { set_error("vbt_pipeline_step: NULL argument"); return VBT_ERR_ARG; }
  if ((clip_map != nullptr) != (frame_idx != nullptr)) { set_error("vbt_pipeline_step: clip_map and frame_idx come together"); return VBT_ERR_ARG; }
  PL_CHECK(p->ingest.check_sources("vbt_pipeline_step", src_h, src_w, swap_rb, frames_on_device ? frames : nullptr));
  if (active && p->n_trk != p->n) { set_error("vbt_pipeline_step: `active` needs one clip per slot"); return VBT_ERR_ARG; }
  if (clip_map)
    for (int i = 0; i < p->n; i++)
      if (clip_map[i] >= p->n_trk) { set_error("vbt_pipeline_step: slot %d -> clip %d, the pipeline follows %d clips", i, clip_map[i], p->n_trk); return VBT_ERR_ARG; }
  if (!clip_map && track && p->n_trk > p->n) { set_error("vbt_pipeline_step: %d clips on %d slots needs clip_map / frame_idx (or vbt_pipeline_step_runs)", p->n_trk, p->n); return VBT_ERR_ARG; }
  StepTimer timer(p);
  VBT_HIP_CHECK(hipSetDevice(p->device));
  return step_frames(p, Sources(frames, nullptr, frames_on_device, src_h, src_w, swap_rb), active, clip_map, frame_idx, track, caller_stream);
}

int vbt_pipeline_step_runs(vbt_pipeline* p, const uint8_t* frames, const uint8_t* const* run_sources, int frames_on_device, const vbt_run* runs,
                           int n_runs, int src_h, int src_w, int swap_rb, int track, float* out_boxes, float* out_scores, float* out_classes,
                           int32_t* out_counts, void* caller_stream) {
  if (!p || !runs || n_runs < 1 || ((frames != nullptr) == (run_sources != nullptr))) {
    set_error("vbt_pipeline_step_runs: runs and exactly one of frames / run_sources required");
    return VBT_ERR_ARG;
  }
  const bool outs = out_boxes || out_scores || out_classes || out_counts;
  if (outs && (!out_boxes || !out_scores || !out_classes || !out_counts || track)) {
    set_error("vbt_pipeline_step_runs: out_* come together and are for detector-only steps (track = 0)");
    return VBT_ERR_ARG;
  }
  PL_CHECK(p->ingest.check_sources("vbt_pipeline_step_runs", src_h, src_w, swap_rb, frames_on_device ? frames : nullptr,
                               frames_on_device ? run_sources : nullptr, frames_on_device && run_sources ? n_runs : 0));
  StepTimer timer(p);
  VBT_HIP_CHECK(hipSetDevice(p->device));
  std::vector<vbt_run> ra(runs, runs + n_runs);
  int B = 0;
  for (int i = 0; i < n_runs; i++) {
    vbt_run& r = ra[i];
    if (r.slot_stride == 0) r.slot_stride = 1;
    if (r.frame_step == 0) r.frame_step = 1;
    if (r.clip < 0 || r.clip >= p->n_trk || r.n_frames < 1 || r.slot0 < 0 || r.slot_stride != 1 || (long)r.slot0 + r.n_frames > p->n) {
      set_error("run %d: clip %d, slots %d..%ld outside %d clips / %d slots", i, r.clip, r.slot0, (long)r.slot0 + r.n_frames - 1, p->n_trk, p->n);
      return VBT_ERR_ARG;
    }
    if (!(r.fps > 0.0)) r.fps = p->fps[r.clip];
    if (run_sources && !run_sources[i]) { set_error("run %d: NULL source", i); return VBT_ERR_ARG; }
    B = std::max(B, r.slot0 + r.n_frames);
  }
  if (run_sources) {   // raw pointers base + f * frame_bytes go to the gather kernel / the copies: a hole would be detected on garbage
    std::vector<char> used((size_t)B, 0);
    for (const vbt_run& r : ra)
      for (int f = 0; f < r.n_frames; f++) used[(size_t)r.slot0 + f] = 1;
    for (char u : used)
      if (!u) { set_error("vbt_pipeline_step_runs: the runs leave a hole in the detector batch"); return VBT_ERR_ARG; }
  }
  const Sources src(frames, run_sources, frames_on_device, src_h, src_w, swap_rb);
  std::vector<vbt_run> asm_runs(ra);
  return step_runs_impl(p, src, asm_runs.data(), n_runs, ra, B, track, out_boxes, out_scores, out_classes, out_counts, caller_stream);
}

int vbt_pipeline_set_pixel_format(vbt_pipeline* p, int pix_fmt) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  if (pix_fmt != VBT_PIX_RGB24 && !pix_fmt_is_source_yuv(pix_fmt)) { set_error("vbt_pipeline_set_pixel_format: unknown pixel format %d", pix_fmt); return VBT_ERR_ARG; }
  p->ingest.set_pixel_format(pix_fmt);
  return VBT_OK;
}

int vbt_pipeline_set_colour(vbt_pipeline* p, int matrix, int range) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  if (matrix != VBT_CS_BT601 && matrix != VBT_CS_BT709) { set_error("vbt_pipeline_set_colour: unknown matrix %d", matrix); return VBT_ERR_ARG; }
  if (range != VBT_RANGE_LIMITED && range != VBT_RANGE_FULL) { set_error("vbt_pipeline_set_colour: unknown range %d", range); return VBT_ERR_ARG; }
  p->ingest.set_colour(matrix, range);
  return VBT_OK;
}

int vbt_pipeline_skip_frames(vbt_pipeline* p, int n) {
  if (!p || n < 0) { set_error("vbt_pipeline_skip_frames: bad argument"); return VBT_ERR_ARG; }
  PL_CHECK(finish_forward(p));
  p->frame_count += n;
  return VBT_OK;
}

int vbt_pipeline_set_frame_count(vbt_pipeline* p, int frame_count) {
  if (!p || frame_count < 0) { set_error("vbt_pipeline_set_frame_count: bad argument"); return VBT_ERR_ARG; }
  PL_CHECK(finish_forward(p));
  p->frame_count = frame_count;
  return VBT_OK;
}

int vbt_pipeline_reset(vbt_pipeline* p) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(p->device));
  PL_CHECK(drain(p));
  VBT_HIP_CHECK(hipDeviceSynchronize());
  PL_CHECK(vbt_tracker_reset(p->trk.get()));
  p->frame_count = 0;
  p->step_idx = 0;
  p->next_o = p->fwd_idx = p->last_o = p->last_k = 0;
  std::fill(p->trk_ev_of.begin(), p->trk_ev_of.end(), -1);
  p->last_trk = -1;
  std::fill(p->clip_frames.begin(), p->clip_frames.end(), 0);
  std::fill(p->fc_base.begin(), p->fc_base.end(), 0);
  std::fill(p->closed_unread.begin(), p->closed_unread.end(), 0);   // unread slot-close results are dropped
  p->step_host_ns = p->step_calls = 0;
  return VBT_OK;
}

int vbt_pipeline_join_detectors(vbt_pipeline* p, void* stream) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  PL_CHECK(finish_forward(p));
  for (const Event& e : p->ev_det) VBT_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, e.get(), 0));
  return VBT_OK;
}

int vbt_pipeline_drain(vbt_pipeline* p) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(p->device));
  return drain(p);
}

int vbt_pipeline_finish(vbt_pipeline* p) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  PL_CHECK(drain_and_finish(p));
  VBT_HIP_CHECK(hipStreamSynchronize(p->trk_stream));
  return VBT_OK;
}

// The metrics block of the slot close, once both the slot close and the rep metrics are enabled (whichever came second calls it)
static int closed_metrics_alloc(vbt_pipeline* p) {
  if (!p->rep_metrics || !p->closed_head || p->closed_metrics) return VBT_OK;
  PinnedBuf<unsigned char> m;
  double* dev = nullptr;
  hipError_t e = m.alloc((size_t)p->n_trk * CLOSED_METRICS_BYTES, hipHostMallocMapped | hipHostMallocCoherent);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&dev, m.get(), 0);
  if (e != hipSuccess) { set_error("hipHostMalloc of the close metrics failed: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
  p->closed_metrics = std::move(m);
  p->closed_metrics_dev = dev;
  return VBT_OK;
}

// The slot close's buffers, allocated once so that no close allocates: per tracker clip a pinned record, a device row outbox and an
// event; and the stream the rows come back on.  All or nothing.
int vbt_pipeline_close_clips_enable(vbt_pipeline* p) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  if (p->closed_head) return VBT_OK;
  VBT_HIP_CHECK(hipSetDevice(p->device));
  const size_t nt = (size_t)p->n_trk;
  auto failed = [](const char* what, hipError_t e) {
    set_error("vbt_pipeline_close_clips_enable: %s failed: %s", what, hipGetErrorString(e));
    return VBT_ERR_HIP;
  };
  DevBuf<unsigned char> rows;
  PinnedBuf<unsigned char> head;
  unsigned char* head_dev = nullptr;
  std::vector<Event> evs(nt);
  hipError_t e = rows.alloc(nt * (size_t)p->prm.rows_cap * 64);
  if (e != hipSuccess) return failed("hipMalloc of the row outboxes", e);
  // coherent: the close kernel's stores reach host memory directly, visible once the close's event has completed
  e = head.alloc(nt * CLOSED_HEAD_BYTES, hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) return failed("hipHostMalloc of the close records", e);
  e = hipHostGetDevicePointer((void**)&head_dev, head.get(), 0);
  if (e != hipSuccess) return failed("hipHostGetDevicePointer", e);
  for (Event& ev : evs) {
    e = ev.create(hipEventDisableTiming);
    if (e != hipSuccess) return failed("hipEventCreate", e);
  }
  {
    std::lock_guard<std::mutex> lock(g_pool_mu);
    StreamPool& pool = g_pools[p->device];
    int i = -1;
    const int rc = pool_take(pool, p->device, p->own_streams, -1, false, &i);
    if (rc != VBT_OK) { failed("taking the read stream", hipSuccess); return rc; }
    p->read_stream = pool.streams[(size_t)i];
  }
  p->closed_rows = std::move(rows);
  p->closed_head = std::move(head);
  p->closed_head_dev = head_dev;
  p->ev_closed = std::move(evs);
  p->closed_unread.assign(nt, 0);
  return closed_metrics_alloc(p);
}

// Slot close.  Enqueue only: drain() hands the held-back tracker steps to their streams, the close kernels and the reset follow on the
// tracker stream (in inline mode drain() made it wait for the last tracker launch), and the reset is recorded as the most recent tracker
// launch (rerecord_trk).  The record goes straight into pinned memory (close_pack_kernel), so no copy is enqueued here.
int vbt_pipeline_close_clips(vbt_pipeline* p, const int32_t* clips, int n, const double* next_fps) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  PL_CHECK(check_clip_list("vbt_pipeline_close_clips", clips, n, p->n_trk));
  for (int i = 0; i < n; i++) {
    if (next_fps && !(next_fps[i] > 0.0)) { set_error("vbt_pipeline_close_clips: next_fps[%d] = %g must be > 0", i, next_fps[i]); return VBT_ERR_ARG; }
    if (!p->closed_unread.empty() && p->closed_unread[(size_t)clips[i]]) {
      set_error("vbt_pipeline_close_clips: slot %d still holds an unread result (vbt_pipeline_closed_clip)", clips[i]);
      return VBT_ERR_STATE;
    }
  }
  if (!p->closed_head) {
    set_error("vbt_pipeline_close_clips: the slot close is not enabled (vbt_pipeline_close_clips_enable)");
    return VBT_ERR_STATE;
  }
  VBT_HIP_CHECK(hipSetDevice(p->device));
  PL_CHECK(drain(p));
  hipStream_t T = p->trk_stream;
  PL_CHECK(tracker_close_clips(p->trk.get(), clips, n, p->prm.plate_diameter, p->prm.diff_threshold, p->prm.min_distance, p->closed_head_dev,
                               p->closed_metrics_dev, p->closed_rows.get(), T));
  for (int i = 0; i < n; i++) {
    const int c = clips[i];
    VBT_HIP_CHECK(hipEventRecord(p->ev_closed[(size_t)c].get(), T));
    p->closed_unread[(size_t)c] = 1;
    p->fc_base[(size_t)c] = p->frame_count;                       // the next plain step is frame 1 of the new clip
    if ((size_t)c < p->clip_frames.size()) p->clip_frames[(size_t)c] = 0;
    if (next_fps) p->fps[(size_t)c] = next_fps[i];
  }
  return rerecord_trk(p, T);
}

// vbt_pipeline_closed_clip (metrics8 == nullptr) / vbt_pipeline_closed_clip_ex
static int closed_clip(vbt_pipeline* p, int clip, int wait, int* ready, vbt_closed_clip* rec, double* phases6, double* metrics8, int cap_phases,
                       void* rows_host, int cap_rows) {
  if (clip < 0 || clip >= p->n_trk) { set_error("vbt_pipeline_closed_clip: slot %d outside the %d clips", clip, p->n_trk); return VBT_ERR_ARG; }
  *ready = 0;
  if (p->closed_unread.empty() || !p->closed_unread[(size_t)clip]) { set_error("vbt_pipeline_closed_clip: slot %d has no unread result", clip); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(p->device));
  PL_CHECK(finish_forward(p));
  hipEvent_t ev = p->ev_closed[(size_t)clip].get();
  if (wait) {
    VBT_HIP_CHECK(hipEventSynchronize(ev));
  } else {
    const hipError_t q = hipEventQuery(ev);
    if (q == hipErrorNotReady) return VBT_OK;
    VBT_HIP_CHECK(q);
  }
  const unsigned char* h = p->closed_head.get() + (size_t)clip * CLOSED_HEAD_BYTES;
  const int32_t* hd = (const int32_t*)h;
  rec->clip = clip; rec->best_id = hd[0]; rec->n_rows = hd[1]; rec->n_phases = hd[2]; rec->overflow = hd[3]; rec->reserved = 0;
  if (hd[2] > cap_phases) { set_error("vbt_pipeline_closed_clip: slot %d has %d phases, buffer holds %d", clip, hd[2], cap_phases); return VBT_ERR_CAPACITY; }
  if (rows_host && hd[1] > cap_rows) { set_error("vbt_pipeline_closed_clip: slot %d has %d rows, buffer holds %d", clip, hd[1], cap_rows); return VBT_ERR_CAPACITY; }
  if (hd[2] > 0) memcpy(phases6, h + 16, (size_t)hd[2] * 48);
  if (hd[2] > 0 && metrics8) memcpy(metrics8, p->closed_metrics.get() + (size_t)clip * CLOSED_METRICS_BYTES, (size_t)hd[2] * 64);
  if (rows_host && hd[1] > 0) {
    const unsigned char* src = p->closed_rows.get() + (size_t)clip * p->prm.rows_cap * 64;
    VBT_HIP_CHECK(hipStreamWaitEvent(p->read_stream, ev, 0));   // (done already: the copy waits for this close only)
    VBT_HIP_CHECK(hipMemcpyAsync(rows_host, src, (size_t)hd[1] * 64, hipMemcpyDeviceToHost, p->read_stream));
    VBT_HIP_CHECK(hipStreamSynchronize(p->read_stream));
  }
  p->closed_unread[(size_t)clip] = 0;
  *ready = 1;
  return VBT_OK;
}

int vbt_pipeline_closed_clip(vbt_pipeline* p, int clip, int wait, int* ready, vbt_closed_clip* rec, double* phases6, int cap_phases,
                             void* rows_host, int cap_rows) {
  if (!p || !ready || !rec || cap_phases < 0 || (cap_phases > 0 && !phases6) || (rows_host && cap_rows < 0)) {
    set_error("vbt_pipeline_closed_clip: bad argument");
    return VBT_ERR_ARG;
  }
  return closed_clip(p, clip, wait, ready, rec, phases6, nullptr, cap_phases, rows_host, cap_rows);
}

int vbt_pipeline_closed_clip_ex(vbt_pipeline* p, int clip, int wait, int* ready, vbt_closed_clip* rec, double* phases6, double* metrics8,
                                int cap_phases, void* rows_host, int cap_rows) {
  if (!p || !ready || !rec || cap_phases < 0 || (cap_phases > 0 && (!phases6 || !metrics8)) || (rows_host && cap_rows < 0)) {
    set_error("vbt_pipeline_closed_clip_ex: bad argument");
    return VBT_ERR_ARG;
  }
  if (!p->rep_metrics) { set_error("vbt_pipeline_closed_clip_ex: rep metrics are not enabled (vbt_pipeline_rep_metrics_enable)"); return VBT_ERR_STATE; }
  return closed_clip(p, clip, wait, ready, rec, phases6, cap_phases > 0 ? metrics8 : nullptr, cap_phases, rows_host, cap_rows);
}

int vbt_pipeline_close_ex(vbt_pipeline* p, int32_t* best_ids, int32_t* n_rows, int32_t* n_phases, int32_t* overflow, double* phases6,
                          double* metrics8, int cap) {
  if (!p || !best_ids || !n_rows || !n_phases || !overflow || !phases6 || !metrics8) { set_error("vbt_pipeline_close_ex: NULL argument"); return VBT_ERR_ARG; }
  if (!p->rep_metrics) { set_error("vbt_pipeline_close_ex: rep metrics are not enabled (vbt_pipeline_rep_metrics_enable)"); return VBT_ERR_STATE; }
  PL_CHECK(drain_and_finish(p));
  return vbt_tracker_summary_ex(p->trk.get(), best_ids, n_rows, n_phases, overflow, phases6, metrics8, cap);
}

int vbt_pipeline_close(vbt_pipeline* p, int32_t* best_ids, int32_t* n_rows, int32_t* n_phases, int32_t* overflow, double* phases6, int cap) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  if (!best_ids || !n_rows || !n_phases || !overflow || !phases6) {
    if (best_ids || n_rows || n_phases || overflow || phases6) { set_error("vbt_pipeline_close: the output arrays come together"); return VBT_ERR_ARG; }
    return vbt_pipeline_finish(p);
  }
  PL_CHECK(drain_and_finish(p));
  return vbt_tracker_summary(p->trk.get(), best_ids, n_rows, n_phases, overflow, phases6, cap);
}

int vbt_pipeline_rows_all(vbt_pipeline* p, int32_t* counts, void* rows_host, int cap) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(p->device));
  PL_CHECK(drain(p));
  return vbt_tracker_rows_all(p->trk.get(), counts, rows_host, cap, (void*)p->trk_stream);
}

int vbt_pipeline_rows(vbt_pipeline* p, int clip, int64_t* id, double* cols7, int cap, int* n) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(p->device));
  PL_CHECK(drain(p));
  VBT_HIP_CHECK(hipStreamSynchronize(p->trk_stream));
  return vbt_tracker_rows(p->trk.get(), clip, id, cols7, cap, n);
}

int vbt_pipeline_detections(vbt_pipeline* p, float* boxes, float* scores, float* classes, int32_t* counts, int cap_slots, int* B) {
  if (!p || !boxes || !scores || !classes || !counts || !B) { set_error("vbt_pipeline_detections: NULL argument"); return VBT_ERR_ARG; }
  if (p->step_idx < 1) { set_error("vbt_pipeline_detections: no step yet"); return VBT_ERR_STATE; }
  const int o = p->last_o, nb = p->last_B;
  if (nb > cap_slots) { set_error("vbt_pipeline_detections: %d slots, buffers hold %d", nb, cap_slots); return VBT_ERR_CAPACITY; }
  VBT_HIP_CHECK(hipSetDevice(p->device));
  PL_CHECK(finish_forward(p));   // (the last step's detections are the last slice of its group's forward)
  hipStream_t S = p->det_streams[p->last_k];
  const size_t md = VBT_MAX_DETECTIONS;
  VBT_HIP_CHECK(hipMemcpyAsync(boxes, boxes_of(p, o), nb * md * 16, hipMemcpyDeviceToHost, S));
  VBT_HIP_CHECK(hipMemcpyAsync(scores, scores_of(p, o), nb * md * 4, hipMemcpyDeviceToHost, S));
  VBT_HIP_CHECK(hipMemcpyAsync(classes, classes_of(p, o), nb * md * 4, hipMemcpyDeviceToHost, S));
  VBT_HIP_CHECK(hipMemcpyAsync(counts, counts_of(p, o), (size_t)nb * 4, hipMemcpyDeviceToHost, S));
  VBT_HIP_CHECK(hipStreamSynchronize(S));
  *B = nb;
  return VBT_OK;
}

int vbt_pipeline_tracker_only_steps(vbt_pipeline* p, int count, int slot) {
  if (!p || count < 1 || slot < 0 || slot >= p->ring) { set_error("vbt_pipeline_tracker_only_steps: bad argument"); return VBT_ERR_ARG; }
  if (p->n_trk != p->n) { set_error("vbt_pipeline_tracker_only_steps needs one tracker clip per detector slot"); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(p->device));
  PL_CHECK(flush_block(p));   // (tracker launches stay in frame order)
  hipStream_t T = p->trk_stream;
  VBT_HIP_CHECK(hipStreamWaitEvent(T, p->ev_det[slot].get(), 0));
  if (p->last_trk >= 0) VBT_HIP_CHECK(hipStreamWaitEvent(T, p->ev_trk[p->last_trk].get(), 0));
  std::vector<double> tm((size_t)p->n);
  for (int i = 0; i < count; i++) {
    p->frame_count++;
    for (int c = 0; c < p->n; c++) tm[c] = (double)(p->frame_count - p->fc_base[c]) / p->fps[c];
    PL_CHECK(vbt_tracker_update_from_detections(p->trk.get(), boxes_of(p, slot), scores_of(p, slot), counts_of(p, slot), tm.data(), p->prm.detection_threshold, (void*)T));
  }
  return record_trk(p, slot, T);
}

// Every tracker launch goes through vbt_tracker_update_from_*, which enqueue the live analysis right behind it on the launch's stream -
// before the ev_trk event the pipeline records there - so every site above (plain / slot / run steps, deferred groups, both tracker
// stream modes, tracker-only steps) is covered.
int vbt_pipeline_live_enable(vbt_pipeline* p, int path_cap, int phase_cap) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  if (p->step_idx > 0) { set_error("vbt_pipeline_live_enable: steps were enqueued (enable before the first step, or after a reset)"); return VBT_ERR_STATE; }
  PL_CHECK(vbt_tracker_live_enable(p->trk.get(), path_cap, phase_cap, p->prm.plate_diameter, p->prm.diff_threshold, p->prm.min_distance));
  p->live = true;
  return VBT_OK;
}

int vbt_pipeline_rep_metrics_enable(vbt_pipeline* p) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  if (p->rep_metrics) return VBT_OK;
  if (p->step_idx > 0) { set_error("vbt_pipeline_rep_metrics_enable: steps were enqueued (enable before the first step, or after a reset)"); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(p->device));
  PL_CHECK(vbt_tracker_rep_metrics_enable(p->trk.get()));
  p->rep_metrics = true;
  return closed_metrics_alloc(p);
}

int vbt_pipeline_use_sort(vbt_pipeline* p, const vbt_sort_params* sp) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  PL_CHECK(check_sort_params("vbt_pipeline_use_sort", sp));
  if (p->ever_stepped) { set_error("vbt_pipeline_use_sort: steps were enqueued on this pipeline (choose the tracker before the first step)"); return VBT_ERR_STATE; }
  return tracker_use_sort(p->trk.get(), sp);
}

// vbt_pipeline_live_poll (ex false, metrics8 not read) / vbt_pipeline_live_poll_ex
static int live_poll(vbt_pipeline* p, bool ex, int flush_view, vbt_live_clip* clips, double* phases6, double* metrics8, int cap) {
  if (!p) { set_error("NULL pipeline"); return VBT_ERR_ARG; }
  if (!p->live) { set_error("vbt_pipeline_live_poll%s: live analysis is not enabled", ex ? "_ex" : ""); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(p->device));
  PL_CHECK(drain(p));   // (inline mode: the tracker stream now waits for the last tracker launch)
  if (ex) return vbt_tracker_live_poll_ex(p->trk.get(), flush_view, clips, phases6, metrics8, cap, (void*)p->trk_stream);
  return vbt_tracker_live_poll(p->trk.get(), flush_view, clips, phases6, cap, (void*)p->trk_stream);
}

int vbt_pipeline_live_poll(vbt_pipeline* p, int flush_view, vbt_live_clip* clips, double* phases6, int cap) {
  return live_poll(p, false, flush_view, clips, phases6, nullptr, cap);
}

int vbt_pipeline_live_poll_ex(vbt_pipeline* p, int flush_view, vbt_live_clip* clips, double* phases6, double* metrics8, int cap) {
  return live_poll(p, true, flush_view, clips, phases6, metrics8, cap);
}

// One-pass export.  drain() hands every tracker step still held back to its stream - the block of deferred / grouped steps, the
// own-stream lag - so ev_trk[last_trk] then stands behind every step enqueued so far in all three tracker placements, and each of
// those launches is behind the forward whose preprocess read the frames: drawing into them on `stream` after the event is safe.
int vbt_pipeline_overlay_draw(vbt_pipeline* p, vbt_overlay* o, uint8_t* frames_dev, int B, int frame0, int frame_step, void* stream) {
  if (!p || !o) { set_error("vbt_pipeline_overlay_draw: NULL %s", p ? "overlay" : "pipeline"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(p->device));
  PL_CHECK(drain(p));
  // A panel that follows this tracker's live analysis: its update reads tables the NEXT tracker launch changes in place, and writes
  // the table the handle's previous draw may still read.  It runs on the tracker stream, which drain() has put behind the last
  // tracker launch in every placement, after an event behind that draw, and becomes the most recent tracker launch (rerecord_trk):
  // `stream` (below) comes after the update too.
  const bool panel = overlay_hud_follows(o, p->trk.get());
  if (panel) {
    PL_CHECK(overlay_hud_follow_enqueue(o, p->trk_stream));
    PL_CHECK(rerecord_trk(p, p->trk_stream));
  }
  if (p->last_trk >= 0) VBT_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, p->ev_trk[p->last_trk].get(), 0));
  PL_CHECK(vbt_overlay_follow_update(o, stream));
  PL_CHECK(vbt_overlay_draw(o, frames_dev, B, frame0, frame_step, stream));
  if (panel) PL_CHECK(overlay_hud_follow_drawn(o, (hipStream_t)stream));
  return VBT_OK;
}

int vbt_pipeline_get_info(const vbt_pipeline* p, vbt_pipeline_info* out) {
  if (!p || !out) { set_error("vbt_pipeline_get_info: NULL argument"); return VBT_ERR_ARG; }
  memset(out, 0, sizeof(*out));
  out->n_slots = p->n; out->n_clips = p->n_trk; out->rows_cap = p->prm.rows_cap; out->device = p->device; out->depth = p->depth;
  out->ring = p->ring; out->defer = p->defer; out->tracker_inline = p->trk_inline ? 1 : 0; out->image_size = p->ingest.image_size();
  out->frame_count = p->frame_count; out->steps_enqueued = p->step_idx; out->placement_ok = p->placement_ok ? 1 : 0;
  out->group = p->G;
  int next_o = 0;
  next_slots(p, &next_o, &out->next_slot);
  {
    std::lock_guard<std::mutex> lock(g_pool_mu);
    out->queue_groups_seen = (int)g_pools[p->device].reps.size();
  }
  for (int k = 0; k < p->depth; k++) out->det_streams[k] = (void*)p->det_streams[k];
  out->copy_stream = (void*)p->ingest.stream();
  out->tracker_stream = (void*)p->trk_stream;
  out->h2d_bytes = p->ingest.uploaded();
  out->step_host_ns = p->step_host_ns;
  out->step_calls = p->step_calls;
  return VBT_OK;
}

vbt_model* vbt_pipeline_model(vbt_pipeline* p, int k) { return (p && k >= 0 && k < p->depth) ? p->models[(size_t)k].get() : nullptr; }
vbt_tracker* vbt_pipeline_tracker(vbt_pipeline* p) { return p ? p->trk.get() : nullptr; }

int vbt_track_clip(vbt_pipeline* p, const uint8_t* frames, int frames_on_device, int T, int src_h, int src_w, int swap_rb, int frame_stride,
                   int64_t* id, double* cols7, int cap, int* n_rows) {
  if (!p || !frames || T < 0 || !id || !cols7 || !n_rows || cap < 0) { set_error("vbt_track_clip: bad argument"); return VBT_ERR_ARG; }
  if (p->n_trk != 1) { set_error("vbt_track_clip: the pipeline must follow exactly one clip (n_clips = 1), it follows %d", p->n_trk); return VBT_ERR_ARG; }
  PL_CHECK(p->ingest.check_sources("vbt_track_clip", src_h, src_w, swap_rb, frames_on_device ? frames : nullptr));
  const int stride = std::max(frame_stride, 1);
  const size_t fb = p->ingest.source_frame_bytes(src_h, src_w);
  PL_CHECK(vbt_pipeline_reset(p));
  // frames whose 1-based number is not a multiple of the stride are read and dropped (track.py:161-167): they only advance the time
  const int kept = T / stride, F = p->n;
  for (int i0 = 0; i0 < kept; i0 += F) {
    const int nf = std::min(F, kept - i0);
    const int first = (i0 + 1) * stride;   // 1-based frame number of the chunk's first kept frame
    vbt_run run{0, 0, 1, nf, first, stride, p->fps[0]};
    if (stride == 1) {
      PL_CHECK(vbt_pipeline_step_runs(p, frames + (size_t)(first - 1) * fb, nullptr, frames_on_device, &run, 1, src_h, src_w, swap_rb, 1, nullptr, nullptr,
                                      nullptr, nullptr, nullptr));
    } else {
      // one single-frame run per kept frame: sources `stride` frames apart, assembled by the gather launch / the copy stream
      std::vector<vbt_run> rr((size_t)nf);
      std::vector<const uint8_t*> srcs((size_t)nf);
      for (int f = 0; f < nf; f++) {
        rr[(size_t)f] = vbt_run{0, f, 1, 1, first + f * stride, 1, p->fps[0]};
        srcs[(size_t)f] = frames + (size_t)(first + f * stride - 1) * fb;
      }
      // (the tracker sees ONE run for the clip: assembled from the per-frame sources, walked as the single run)
      VBT_HIP_CHECK(hipSetDevice(p->device));
      const Sources src(nullptr, srcs.data(), frames_on_device, src_h, src_w, swap_rb);
      std::vector<vbt_run> walk(1, run);
      PL_CHECK(step_runs_impl(p, src, rr.data(), nf, walk, nf, 1, nullptr, nullptr, nullptr, nullptr, nullptr));
    }
  }
  PL_CHECK(vbt_pipeline_finish(p));
  return vbt_tracker_rows(p->trk.get(), 0, id, cols7, cap, n_rows);
}

}  // extern "C"
