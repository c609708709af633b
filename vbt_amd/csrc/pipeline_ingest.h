// Frame ingest of vbt_pipeline (pipeline.hip): from what a step call hands over - an assembled batch or one source per run, in host or
// device memory, in the pipeline's pixel format - to B frames at the network resolution on the forward's stream.  It owns the staging
// ring of the host-fed / gathered input with its events, the copy stream, the resized batches and the upload counter; the copies of
// a host-fed step are the plan of upload_plan.h.  Host code; the kernels are reached through resize_frames_dev,
// resize_frames_pix_dev (common.h) and vbt_gather_frames.
#pragma once
#include "common.h"
#include "dev_mem.h"
#include "hip_handles.h"

namespace vbt {

struct Sources {
  const uint8_t* frames;              // assembled batch, or
  const uint8_t* const* run_sources;  // one source per run
  bool on_device;
  int src_h, src_w, swap_rb;
  Sources(const uint8_t* frames_, const uint8_t* const* run_sources_, int frames_on_device, int src_h_, int src_w_, int swap_rb_)
      : frames(frames_), run_sources(run_sources_), on_device(frames_on_device != 0), src_h(src_h_), src_w(src_w_), swap_rb(swap_rb_) {}
};

class Ingest {
 public:
  // Rings and events for `depth` forward slots of n frames at size x size; false: hipEventCreate failed.  The copy stream follows once
  // the pipeline has taken its streams.
  bool create(int depth, int n, int size);
  void set_stream(hipStream_t copy_stream_) { copy_stream = copy_stream_; }
  hipStream_t stream() const { return copy_stream; }
  int image_size() const { return size; }
  uint64_t uploaded() const { return h2d_bytes; }
  // read by the next step call: steps already enqueued carry their own kernels and copies.  The colour is not read while the format
  // is VBT_PIX_RGB24.
  void set_pixel_format(int pix_fmt_) { pix_fmt = pix_fmt_; }
  void set_colour(int matrix, int range) { cs_matrix = matrix; cs_range = range; }
  // bytes of one source frame of src_h x src_w (<= 0: the network size) in the current format
  size_t source_frame_bytes(int src_h, int src_w) const { return pix_layout(pix_fmt, src_h > 0 ? src_h : size, src_w > 0 ? src_w : size).frame_bytes; }

  // What a step may ask for under the current pixel format; checked before anything is enqueued or counted.
  // frames / run_sources[0..n_sources): the step's sources where they are device pointers (else NULL / 0), for the alignment the 4:2:2
  // and P010 kernels need.
  int check_sources(const char* fn, int src_h, int src_w, int swap_rb, const uint8_t* frames = nullptr, const uint8_t* const* run_sources = nullptr,
                    int n_sources = 0) const;
  // Brings B frames to the network resolution on stream S of forward slot k and returns the device pointer the detector reads;
  // *stage_j: the staging buffer they went through (-1: none), for frames_read.
  int prepare(int k, hipStream_t S, const Sources& src, const vbt_run* runs, int n_runs, int B, void* caller_stream, const uint8_t** frames_dev,
              int* stage_j);
  // Behind the last kernel that reads the step's frames on S: staging buffer stage_j is free again (< 0: none was used)
  int frames_read(int stage_j, hipStream_t S);

 private:
  struct Stage {
    DevBuf<uint8_t> buf;
    size_t bytes = 0;              // (0 whenever buf is empty)
    Event free_ev, copy_ev;
    bool free_set = false;
  };
  int stage_take(size_t bytes, bool host_gate, hipStream_t S, int* j_out);
  int upload(uint8_t* stage_buf, int slot0, const uint8_t* host, int nf, const PixLayout& lay, int H, bool compact);

  int n = 0, size = 0;
  hipStream_t copy_stream = nullptr;
  std::vector<Event> ev_in;        // per forward slot: the caller's stream has reached the step call
  std::vector<Stage> stage;
  int stage_idx = 0;
  std::vector<DevBuf<uint8_t>> resized;
  std::vector<int> tab;            // p(d) of the compact upload, for (tab_H, size)
  int tab_H = 0;
  std::vector<UploadCopy> plan;    // scratch of upload
  int pix_fmt = VBT_PIX_RGB24;
  int cs_matrix = VBT_CS_BT601, cs_range = VBT_RANGE_LIMITED;
  uint64_t h2d_bytes = 0;
};

}  // namespace vbt
