// Ingest (pipeline_ingest.h): the staging ring, the upload of host frames by the plan of upload_plan.h, the assembly of device runs,
// the resize / conversion to the network resolution.  Host code only.
#include "pipeline_ingest.h"

namespace vbt {

// host frames with more than twice the network's rows travel compact (upload_plan.h)
static bool compact_rows(int H, int size) {
  static const bool off = getenv("VBT_NO_ROW_UPLOAD") != nullptr;
  return !off && H >= 2 && 2 * size < H;
}

bool Ingest::create(int depth, int n_, int size_) {
  n = n_;
  size = size_;
  ev_in.resize((size_t)depth);
  bool ok = true;
  for (Event& e : ev_in) ok = ok && e.create(hipEventDisableTiming) == hipSuccess;
  // host-fed mode: H2D copies run on their own stream into a ring of depth + 2 staging buffers, i.e. up to two steps ahead of the
  // forwards, so that a slot's forward never waits for its own copy
  stage.resize((size_t)depth + 2);
  for (auto& s : stage) ok = ok && s.free_ev.create(hipEventDisableTiming) == hipSuccess && s.copy_ev.create(hipEventDisableTiming) == hipSuccess;
  resized.resize((size_t)depth);
  return ok;
}

// Before an H2D copy into staging buffer j is enqueued the forward that last read the buffer must be done.  The wait is on the
// HOST (the event is depth + 2 steps old: it has completed unless the caller is that many steps ahead of the GPU, and then blocking
// the caller is the back-pressure wanted), NOT a stream wait on the copy stream: a cross-stream event wait in front of a DMA copy
// makes hipMemcpyAsync itself block the calling thread on this stack (profiles/r04_h2d_pinned_order.md).
int Ingest::stage_take(size_t bytes, bool host_gate, hipStream_t S, int* j_out) {
  const int j = stage_idx % (int)stage.size();
  stage_idx++;
  Stage& st = stage[j];
  if (st.bytes < bytes) {
    // a buffer that has to be replaced may still be read by a forward or written by a copy in flight (up to depth + 2 steps)
    if (st.buf) {
      if (st.free_set) VBT_HIP_CHECK(hipEventSynchronize(st.free_ev.get()));
      VBT_HIP_CHECK(hipEventSynchronize(st.copy_ev.get()));
      st.free_set = false;
    }
    st.bytes = 0;
    VBT_HIP_CHECK(st.buf.alloc(bytes + 64));   // (frees the old buffer first)
    st.bytes = bytes;
  }
  if (st.free_set) {
    if (host_gate) VBT_HIP_CHECK(hipEventSynchronize(st.free_ev.get()));
    else VBT_HIP_CHECK(hipStreamWaitEvent(S, st.free_ev.get(), 0));
  }
  *j_out = j;
  return VBT_OK;
}

// nf host frames of H rows -> staging buffer (frame slot0 onwards) on the copy stream
int Ingest::upload(uint8_t* stage_buf, int slot0, const uint8_t* host, int nf, const PixLayout& lay, int H, bool compact) {
  upload_plan(lay.row, lay.chroma_plane, H, size, compact, tab, slot0, nf, plan);
  uint64_t bytes = 0;
  for (const UploadCopy& c : plan) {
    if (c.flat) VBT_HIP_CHECK(hipMemcpyAsync(stage_buf + c.dst_off, host + c.src_off, c.width, hipMemcpyHostToDevice, copy_stream));
    else
      VBT_HIP_CHECK(hipMemcpy2DAsync(stage_buf + c.dst_off, c.dst_pitch, host + c.src_off, c.src_pitch, c.width, c.height, hipMemcpyHostToDevice, copy_stream));
    bytes += (uint64_t)c.width * c.height;
  }
  h2d_bytes += bytes;
  return VBT_OK;
}

int Ingest::check_sources(const char* fn, int src_h, int src_w, int swap_rb, const uint8_t* frames, const uint8_t* const* run_sources,
                          int n_sources) const {
  if ((src_h > 0) != (src_w > 0)) { set_error("%s: src_h and src_w come together", fn); return VBT_ERR_ARG; }
  if (!pix_fmt_is_source_yuv(pix_fmt)) return VBT_OK;
  if (pix_fmt_is_yuv(pix_fmt)) {
    if (src_h <= 0 || src_w <= 0 || (src_h & 1) || (src_w & 1)) {
      set_error("%s: YUV 4:2:0 frames need src_h and src_w, > 0 and even, got %d x %d", fn, src_h, src_w);
      return VBT_ERR_ARG;
    }
  } else if (!pix_fmt_takes(pix_fmt, src_h, src_w)) {
    set_error("%s: %s frames need src_h and src_w in 1..16384, src_w even%s, got %d x %d", fn, pix_fmt_is_422(pix_fmt) ? "YUV 4:2:2" : "P010",
              pix_fmt_is_422(pix_fmt) ? "" : " and src_h even", src_h, src_w);
    return VBT_ERR_ARG;
  }
  if (swap_rb) { set_error("%s: swap_rb does not apply to YUV frames", fn); return VBT_ERR_ARG; }
  if (!pix_fmt_is_yuv(pix_fmt)) {
    bool aligned = ((uintptr_t)frames & 3) == 0;
    for (int i = 0; i < n_sources && aligned; i++) aligned = ((uintptr_t)run_sources[i] & 3) == 0;
    if (!aligned) { set_error("%s: device frames of a 4:2:2 or P010 source must be 4-byte aligned", fn); return VBT_ERR_ARG; }
  }
  return VBT_OK;
}

int Ingest::prepare(int k, hipStream_t S, const Sources& src, const vbt_run* runs, int n_runs, int B, void* caller_stream,
                    const uint8_t** frames_dev, int* stage_j) {
  const bool yuv = pix_fmt_is_source_yuv(pix_fmt);   // (a YUV source at the network resolution is still converted)
  const bool resize = yuv || (src.src_h > 0 && src.src_w > 0 && (src.src_h != size || src.src_w != size || src.swap_rb));
  const int H = src.src_h > 0 ? src.src_h : size, W = src.src_w > 0 ? src.src_w : size;
  const PixLayout lay = pix_layout(pix_fmt, H, W);
  const size_t fb = lay.frame_bytes;
  const bool compact = !src.on_device && resize && compact_rows(H, size);
  if (compact && tab_H != H) {
    row_table(H, size, tab);
    tab_H = H;
  }
  const StagedLayout staged = staged_layout(lay.row, lay.chroma_plane, H, size, compact, tab);   // of what the resize reads
  *stage_j = -1;
  const uint8_t* ptr = src.frames;
  if (src.on_device) {
    // frames are ready once the caller's stream gets here
    VBT_HIP_CHECK(hipEventRecord(ev_in[k].get(), (hipStream_t)caller_stream));
    VBT_HIP_CHECK(hipStreamWaitEvent(S, ev_in[k].get(), 0));
  }
  if (!src.on_device || !src.frames) {
    // host frames are uploaded, one device source per run is assembled: either way into a staging buffer
    int j = 0;
    PL_CHECK(stage_take((size_t)n * staged.frame_bytes, !src.on_device, S, &j));
    uint8_t* st = stage[j].buf.get();
    if (!src.on_device) {
      if (src.frames) PL_CHECK(upload(st, 0, src.frames, B, lay, H, compact));
      else
        for (int i = 0; i < n_runs; i++) PL_CHECK(upload(st, runs[i].slot0, src.run_sources[i], runs[i].n_frames, lay, H, compact));
      VBT_HIP_CHECK(hipEventRecord(stage[j].copy_ev.get(), copy_stream));
      VBT_HIP_CHECK(hipStreamWaitEvent(S, stage[j].copy_ev.get(), 0));
    } else {
      bool aligned = fb % 16 == 0;
      for (int i = 0; i < n_runs && aligned; i++) aligned = ((uintptr_t)src.run_sources[i] & 15) == 0;
      if (aligned) {
        std::vector<const uint8_t*> ptrs((size_t)B, nullptr);
        for (int i = 0; i < n_runs; i++)
          for (int f = 0; f < runs[i].n_frames; f++) ptrs[(size_t)runs[i].slot0 + f] = src.run_sources[i] + (size_t)f * fb;
        PL_CHECK(vbt_gather_frames(st, ptrs.data(), B, fb, (void*)S));
      } else {
        // a frame size that is not a multiple of 16 bytes (any source resolution is allowed): the gather kernel moves 16-byte
        // pieces, so the batch is assembled by one device copy per run instead
        for (int i = 0; i < n_runs; i++)
          VBT_HIP_CHECK(hipMemcpyAsync(st + (size_t)runs[i].slot0 * fb, src.run_sources[i], (size_t)runs[i].n_frames * fb, hipMemcpyDeviceToDevice, S));
      }
    }
    ptr = st;
    *stage_j = j;
  }
  if (resize) {
    if (!resized[k]) VBT_HIP_CHECK(resized[k].alloc((size_t)n * size * size * 3 + 64));
    if (yuv) {
      PL_CHECK(resize_frames_pix_dev(ptr, B, H, W, pix_fmt, cs_matrix, cs_range, staged.frame_bytes, staged.chroma_off, compact ? 1 : 0, resized[k].get(),
                                     size, size, S));
    } else {
      PL_CHECK(resize_frames_dev(ptr, B, H, W, resized[k].get(), size, size, src.swap_rb, compact ? 1 : 0, S));
    }
    ptr = resized[k].get();
  }
  *frames_dev = ptr;
  return VBT_OK;
}

int Ingest::frames_read(int stage_j, hipStream_t S) {
  if (stage_j < 0) return VBT_OK;
  VBT_HIP_CHECK(hipEventRecord(stage[stage_j].free_ev.get(), S));
  stage[stage_j].free_set = true;
  return VBT_OK;
}

}  // namespace vbt
