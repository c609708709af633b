// Shared host-side declarations for libvbt_hip.so (product code; never includes anything from oracle/).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vbt_hip.h"
#include "../../include/vbt_hip_diag.h"
#include "container_parse.h"
#include "upload_plan.h"   // PixLayout, pix_layout, the pix_fmt_* predicates; the compact layout

namespace vbt {

void set_error(const char* fmt, ...);   // (runtime.hip, with use_device and lds_opt_in below)

// The library's one device check: `device` is a visible HIP device - else VBT_ERR_HIP with "<fn>: HIP device %d not available (%d visible)
// - no CPU fallback" set - and, unless set_current is false, the calling thread's current device from here on.
int use_device(const char* fn, int device, bool set_current = true);

// roctx ranges around the host-side enqueue of the path's three stages (detect incl. decode + NMS, track, clip close): with
// VBT_ROCTX=1 the library loads librocprofiler-sdk-roctx.so at the first use and `rocprofv3 --marker-trace` shows
// "vbt:detect" / "vbt:track" / "vbt:finish" next to the kernels they enqueue; without it every call is one branch.
struct RoctxRange {
  explicit RoctxRange(const char* name);
  ~RoctxRange();
  bool on;
};

// More than 64 KB of dynamic LDS is an opt-in per kernel AND per device (hipFuncSetAttribute acts on the current device's code object).
// Every launch site keeps its own per-device record; a refusal is an error (VBT_ERR_HIP with the text set), not a silent launch failure
// that surfaces at a later synchronisation or inside a stream capture.
struct LdsOptIn { signed char dev[64] = {0}; };
bool lds_opt_in(const void* fn, LdsOptIn* state);
#define VBT_LDS_OPT_IN(...)                                                                          \
  do {                                                                                               \
    static vbt::LdsOptIn lds_state_;                                                                 \
    if (!vbt::lds_opt_in(reinterpret_cast<const void*>(&__VA_ARGS__), &lds_state_)) return VBT_ERR_HIP; \
  } while (0)

#define VBT_HIP_CHECK(expr)                                                              \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      vbt::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return VBT_ERR_HIP;                                                                \
    }                                                                                    \
  } while (0)

// a call that returns a VBT_* code and has set the error text (the pipeline's units)
#define PL_CHECK(expr)            \
  do {                            \
    const int rc_ = (expr);       \
    if (rc_ != VBT_OK) return rc_; \
  } while (0)

// preprocess_image (reference odt.py:10-19) on device memory (frames.hip, with its kernel); compact != 0: src holds only the row pairs the
// resize reads (the compact layout, upload_plan.h)
int resize_frames_dev(const uint8_t* src_dev, int B, int H, int W, uint8_t* dst_dev, int h, int w, int swap_rb, int compact, hipStream_t st);
// the same for VBT_PIX_NV12 / VBT_PIX_I420 sources, conversion fused (yuv_kernels.h): frame b at src_dev + b * frame_stride, its chroma
// plane(s) at chroma_off; compact != 0: the luma part holds only the row pairs.  Whole frames: frame_stride H*W*3/2, chroma_off H*W.
int resize_frames_yuv_dev(const uint8_t* src_dev, int B, int H, int W, int pix_fmt, size_t frame_stride, size_t chroma_off, int compact,
                          uint8_t* dst_dev, int h, int w, hipStream_t st);

// The colour description as the conversion kernels take it (yuv_kernels.h): by value, uniform across the launch
struct YuvColour { int cy, crv, cgu, cgv, cbu, yoff, coff; };
// the table of include/vbt_hip.h; false: an unknown format, matrix or range
bool yuv_colour(int pix_fmt, int matrix, int range, YuvColour* c);
// preprocess_image for any YUV format under a colour description.  Frame b at src_dev + b * frame_stride.  Formats with a chroma plane:
// as resize_frames_yuv_dev (NV12 / I420 under the default description run that very kernel).  4:2:2: whole frames of H rows, or -
// compact - [2h] rows, the row pairs the resize reads, as resize_frames_dev has them; chroma_off is not read.  4:2:2 and P010 sources
// are 4-byte aligned.
int resize_frames_pix_dev(const uint8_t* src_dev, int B, int H, int W, int pix_fmt, int matrix, int range, size_t frame_stride, size_t chroma_off,
                          int compact, uint8_t* dst_dev, int h, int w, hipStream_t st);

// Slot close (vbt_pipeline_close_clips): the per-clip record close_pack_kernel writes, { int best_id, n_rows, n_phases, overflow ;
// double phases[512][6] } (512 = the phases a clip keeps, tracker_state.h MAXPH; tracker.hip asserts the two agree)
constexpr size_t CLOSED_HEAD_BYTES = 16 + 512 * 48;
constexpr size_t CLOSED_METRICS_BYTES = 512 * 64;   // ... and, with rep metrics enabled, double metrics[512][8] in a block of their own
// clips[0..n): each in [0, n_clips), none twice, n >= 1 - else VBT_ERR_ARG with the error text set (fn: the caller's name)
int check_clip_list(const char* fn, const int32_t* clips, int n, int n_clips);
// Device part of vbt_pipeline_close_clips (tracker_analysis.hip), enqueue only, on st: export id + rep analysis of the listed clips (the kernels
// of vbt_tracker_finish on the list), their records into head (pinned, [n_clips][CLOSED_HEAD_BYTES]) and their rows into out_rows
// (device, [n_clips][rows_cap] 64-byte rows), then a fresh clip in every listed slot (vbt_tracker_reset_clips).  mhead (or null; needs
// rep metrics enabled on t): pinned, [n_clips][CLOSED_METRICS_BYTES], the metrics of the records' phases
int tracker_close_clips(vbt_tracker* t, const int32_t* clips, int n, double plate_diameter, double diff_threshold, double min_distance,
                        unsigned char* head, double* mhead, void* out_rows, hipStream_t st);
// The SORT tracker's parameters as vbt_tracker_create_sort takes them (tracker.hip): VBT_ERR_ARG with the text set for what it
// refuses; no device call (who: the caller's name)
int check_sort_params(const char* who, const vbt_sort_params* sp);
// An unstepped tracker becomes a SORT tracker (vbt_pipeline_use_sort): parameters checked, clip states re-initialised with id_base.
// VBT_ERR_STATE when it has been stepped.  Synchronises the device.
int tracker_use_sort(vbt_tracker* t, const vbt_sort_params* sp);

// The pipeline's side of a rep panel that follows the live analysis (overlay.hip; vbt_pipeline_overlay_draw is their one caller).
// Does the handle's panel follow a clip of tracker t?
bool overlay_hud_follows(const vbt_overlay* o, const vbt_tracker* t);
// The handle's vbt_overlay_hud_follow_update, with its vbt_overlay_hud_follow_flush setting, on T - the stream the tracker's launches
// are ordered on - behind the handle's previous pipeline draw (one event wait, none before the first draw).  Enqueue only.
int overlay_hud_follow_enqueue(vbt_overlay* o, hipStream_t T);
// The draw just enqueued on `stream` reads the handle's table: the next overlay_hud_follow_enqueue waits for it
int overlay_hud_follow_drawn(vbt_overlay* o, hipStream_t stream);

// ---- VBTM container records, reader + validator, plan-file reader: container_parse.h (pure C++, also built host-only under
// -fsanitize=address,undefined by tests/test_parser_fuzz.py) ----
// Integer parameters of an int8 ADD exactly as XNNPACK derives them (xnn_create_add_nd_qs8 +
// xnn_init_qs8_add_minmax_*_params of the XNNPACK revision tflite-runtime 2.14 builds; the reference runs that kernel
// through the default delegate, reference odt.py:58-61):  q = clamp(((bias + a*am + b*bm) >> shift) + z_out, lo, hi).
struct AddParams { int32_t bias, am, bm, shift; };
inline bool xnn_add_params(float s_a, float s_b, float s_out, int z_a, int z_b, AddParams* p) {
  const float a_os = s_a / s_out, b_os = s_b / s_out;
  if (!(a_os >= 0x1.0p-10f && a_os < 0x1.0p+8f) || !(b_os >= 0x1.0p-10f && b_os < 0x1.0p+8f)) return false;
  const float mx = a_os > b_os ? a_os : b_os;
  uint32_t bits;
  memcpy(&bits, &mx, 4);
  const int32_t max_exp = (int32_t)(bits >> 23) - 127;
  const uint32_t shift = (uint32_t)(20 - max_exp);
  if (shift < 12 || shift > 30) return false;
  auto scaled = [&](float v) {  // v * 2^shift through the exponent field, then lrintf (round to nearest even)
    uint32_t b;
    memcpy(&b, &v, 4);
    b += shift << 23;
    float f;
    memcpy(&f, &b, 4);
    return (int32_t)lrintf(f);
  };
  p->am = scaled(a_os);
  p->bm = scaled(b_os);
  p->shift = (int32_t)shift;
  p->bias = (int32_t)((1u << (shift - 1)) - (uint32_t)(p->am * z_a) - (uint32_t)(p->bm * z_b));
  return true;
}

}  // namespace vbt
