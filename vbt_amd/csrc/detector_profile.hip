// Diagnostic entry points of the detector (include/vbt_hip_diag.h): per-family accounting and the event / wall-clock timings of the
// plan's launches.  Host code only; the launches themselves are detector.hip's.
#include <chrono>
#include <vector>

#include "detector_model.h"

using namespace vbt;

// `reps` forwards on st, one at a time, with an event before every step and one after the last: per_step(i, ms) for every step i of
// every forward.  The events are freed on every way out.
template <class F>
static int timed_forwards(vbt_model* m, const uint8_t* frames_dev, int B, int reps, hipStream_t st, F per_step) {
  const int ns = (int)m->steps.size();
  std::vector<Event> evs(ns + 1);
  for (Event& e : evs) VBT_HIP_CHECK(e.create(hipEventDefault));
  for (int r = 0; r < reps; r++) {
    const int rc = enqueue_forward(m, frames_dev, B, st, m->out_boxes, m->out_scores, m->out_classes, m->out_counts, evs.data());
    if (rc) return rc;
    if (hipStreamSynchronize(st) != hipSuccess) { set_error("stream sync failed"); return VBT_ERR_HIP; }
    for (int i = 0; i < ns; i++) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, evs[i].get(), evs[i + 1].get());
      per_step(i, ms);
    }
  }
  return VBT_OK;
}

extern "C" {

int vbt_model_kernel_stats(const vbt_model* m, int B, vbt_kernel_stat* out, int cap, int* n) {
  if (!m || !out || !n || cap < F_COUNT) { set_error("bad argument"); return VBT_ERR_ARG; }
  for (int i = 0; i < F_COUNT; i++) {
    memset(&out[i], 0, sizeof(out[i]));
    snprintf(out[i].name, sizeof(out[i].name), "%s", kFamilyName[i]);
  }
  for (const Step& s : m->steps) {
    out[s.family].launches++;
    out[s.family].algorithmic_bytes += s.cost.alg_bytes_per_frame * B + s.cost.weight_bytes;
    out[s.family].macs += s.cost.macs_per_frame * B;
  }
  *n = F_COUNT;
  return VBT_OK;
}

int vbt_model_profile(vbt_model* m, const uint8_t* frames_dev, int B, int reps, void* stream, double* ms_out, int cap) {
  if (!m || !frames_dev || !ms_out || cap < F_COUNT || reps < 1) { set_error("bad argument"); return VBT_ERR_ARG; }
  if (B < 1 || B > m->max_batch) { set_error("bad batch"); return VBT_ERR_CAPACITY; }
  for (int i = 0; i < F_COUNT; i++) ms_out[i] = 0.0;
  const int rc = timed_forwards(m, frames_dev, B, reps, (hipStream_t)stream, [&](int i, float ms) { ms_out[m->steps[i].family] += ms; });
  for (int i = 0; i < F_COUNT; i++) ms_out[i] /= reps;
  return rc;
}

// One bracket per kernel family: all launches of family i of the plan back to back on `stream` (`reps` passes between ONE pair
// of HIP events), so ms_out[i] / launches is an average launch duration without the ~3 us a pair of events around every short
// launch adds - the figure rocprofv3 --kernel-trace reports for the same kernels (profiles/) to within the dispatch gap.
int vbt_model_profile_families(vbt_model* m, int B, int reps, void* stream, double* ms_out, int cap) {
  if (!m || !ms_out || cap < F_COUNT || reps < 1) { set_error("bad argument"); return VBT_ERR_ARG; }
  if (B < 1 || B > m->max_batch) { set_error("bad batch"); return VBT_ERR_CAPACITY; }
  hipStream_t st = (hipStream_t)stream;
  Event e0, e1;
  VBT_HIP_CHECK(e0.create(hipEventDefault));
  VBT_HIP_CHECK(e1.create(hipEventDefault));
  int rc = VBT_OK;
  for (int f = 0; f < F_COUNT && rc == VBT_OK; f++) {
    ms_out[f] = 0.0;
    bool any = false;
    for (const Step& s : m->steps) any |= s.family == f;
    if (!any) continue;
    for (int pass = 0; pass < 2 && rc == VBT_OK; pass++) {   // pass 0: warm (code objects, caches)
      const int n = pass == 0 ? 1 : reps;
      (void)hipEventRecord(e0.get(), st);
      for (int r = 0; r < n && rc == VBT_OK; r++)
        for (const Step& s : m->steps)
          if (s.family == f && rc == VBT_OK) rc = launch_step_staged(m, s, B, st);
      (void)hipEventRecord(e1.get(), st);
      if (hipStreamSynchronize(st) != hipSuccess) { set_error("stream sync failed"); rc = VBT_ERR_HIP; break; }
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, e0.get(), e1.get());
      if (pass == 1) ms_out[f] = (double)ms / reps;
    }
  }
  return rc;
}

// Per-launch timing of the plan (one forward in flight, HIP events around every launch): step i of the execution list ->
// family name, index of the last graph op it covers, kernel variant and milliseconds (average over `reps`).
int vbt_model_profile_steps(vbt_model* m, const uint8_t* frames_dev, int B, int reps, void* stream, vbt_step_time* out, int cap, int* n) {
  if (!m || !frames_dev || !out || !n || reps < 1) { set_error("bad argument"); return VBT_ERR_ARG; }
  if (B < 1 || B > m->max_batch) { set_error("bad batch"); return VBT_ERR_CAPACITY; }
  const int ns = (int)m->steps.size();
  if (cap < ns) { set_error("%d plan steps, buffer holds %d", ns, cap); return VBT_ERR_CAPACITY; }
  for (int i = 0; i < ns; i++) {
    const Step& s = m->steps[i];
    memset(&out[i], 0, sizeof(out[i]));
    snprintf(out[i].family, sizeof(out[i].family), "%s", kFamilyName[s.family]);
    out[i].op = s.op;
    out[i].first_op = s.e_op >= 0 ? s.e_op : (s.sum_op >= 0 ? s.sum_op : (s.d_op >= 0 ? s.d_op : s.op));
    out[i].variant = s.variant;
    out[i].algorithmic_bytes = s.cost.alg_bytes_per_frame * B + s.cost.weight_bytes;
    out[i].macs = s.cost.macs_per_frame * B;
  }
  const int rc = timed_forwards(m, frames_dev, B, reps, (hipStream_t)stream, [&](int i, float ms) { out[i].ms += ms / reps; });
  *n = ns;
  return rc;
}

// Measurement: every plan step launched `reps` times back to back on ONE stream, then `reps` times on each of `nstreams`
// streams at once.  conc_ms[i] (time per launch with the streams racing) against single_ms[i] says how much of step i a
// second and third forward in flight can hide: equal -> the kernel saturates a resource, 1/nstreams -> pure latency.
int vbt_model_profile_overlap(vbt_model* m, int B, int reps, int nstreams, float* single_ms, float* conc_ms, int cap, int* n) {
  if (!m || !single_ms || !conc_ms || !n || reps < 1 || nstreams < 1 || nstreams > 8) { set_error("bad argument"); return VBT_ERR_ARG; }
  if (B < 1 || B > m->max_batch) { set_error("bad batch"); return VBT_ERR_CAPACITY; }
  const int ns = (int)m->steps.size();
  if (cap < ns) { set_error("%d plan steps, buffer holds %d", ns, cap); return VBT_ERR_CAPACITY; }
  std::vector<Stream> ss(nstreams);
  for (Stream& st : ss) VBT_HIP_CHECK(st.create(hipStreamNonBlocking));
  int rc = VBT_OK;
  for (int i = 0; i < ns && rc == VBT_OK; i++) {
    const Step& s = m->steps[i];
    for (int pass = 0; pass < 2 && rc == VBT_OK; pass++) {
      const int k = pass == 0 ? 1 : nstreams;
      for (int j = 0; j < k && rc == VBT_OK; j++) rc = launch_step_staged(m, s, B, ss[j].get());
      if (rc) break;
      VBT_HIP_CHECK(hipDeviceSynchronize());
      auto t0 = std::chrono::steady_clock::now();
      for (int r = 0; r < reps; r++)
        for (int j = 0; j < k; j++) rc = rc ? rc : launch_step_staged(m, s, B, ss[j].get());
      VBT_HIP_CHECK(hipDeviceSynchronize());
      const float ms = (float)(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / (reps * k));
      (pass == 0 ? single_ms : conc_ms)[i] = ms;
    }
  }
  *n = ns;
  return rc;
}

}  // extern "C"
