/*
 * vbt_hip.h - C ABI of libvbt_hip.so, the MI355X (gfx950) drop-in for the hot loop of the
 * reference's track.py (reference track.py:159-247) and plot.py:analyze_df (plot.py:33-47).
 *
 * The reference has no FFI layer of its own: its hot path sits behind duck-typed Python objects
 * (SURVEY.md section 8b).  Each entry point below names the reference interface it replaces;
 * the Python classes in vbt_amd/ bind them with ctypes and keep the reference's call shapes.
 *
 * Conventions: every function returns 0 on success or a negative vbt_status; the message of the
 * last failure on the calling thread is vbt_last_error().  Handles are opaque, owned by the
 * library, used by one host thread at a time.  "dev" pointers are HIP device pointers; `stream`
 * is a hipStream_t passed as void* (NULL = the default stream).  No torch types anywhere.
 */
#ifndef VBT_HIP_H
#define VBT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  VBT_OK = 0,
  VBT_ERR_ARG = -1,      /* bad argument (NULL, out of range, shape mismatch) */
  VBT_ERR_IO = -2,       /* container file missing / malformed */
  VBT_ERR_HIP = -3,      /* a HIP runtime call failed */
  VBT_ERR_CAPACITY = -4, /* batch / row / track capacity exceeded */
  VBT_ERR_STATE = -5     /* call sequence error */
} vbt_status;

#define VBT_MAX_DETECTIONS 25

const char* vbt_last_error(void);
int vbt_device_count(void);

/* ------------------------------------------------------------------ detector ----------------
 * Replaces tflite_runtime.interpreter.Interpreter (reference track.py:93-94, eval.py:167-168):
 *   Interpreter(model_path, num_threads) + allocate_tensors()        -> vbt_model_create
 *   get_input_details()[0]['shape']            (reference odt.py:86-87) -> vbt_model_input_shape
 *   get_signature_runner()(images=uint8[1,H,W,3]) (reference odt.py:58-66) -> vbt_detect
 */
typedef struct vbt_model vbt_model;

/* container_path: a VBTM model container (vbt_amd/container.py); max_batch frames per vbt_detect. */
int vbt_model_create(const char* container_path, int device, int max_batch, vbt_model** out);
/* flags = 0 (VBT_MODEL_DEFAULT_FLAGS): the fused, autotuned execution plan.  The plan-shaping flags used by the parity tests and
 * the tuning tools are lab equipment and live in vbt_hip_diag.h.  vbt_model_create == _ex with flags 0 (or the integer in the
 * environment variable VBT_FUSION_FLAGS). */
#define VBT_MODEL_DEFAULT_FLAGS 0
int vbt_model_create_ex(const char* container_path, int device, int max_batch, int flags, vbt_model** out);
void vbt_model_destroy(vbt_model* m);
/* shape = {max_batch, H, W, 3} */
int vbt_model_input_shape(const vbt_model* m, int shape[4]);
int vbt_model_num_tensors(const vbt_model* m);
int vbt_model_num_ops(const vbt_model* m);
/* shape = {H, W, C} of graph tensor `tensor_id` */
int vbt_model_tensor_shape(const vbt_model* m, int tensor_id, int shape[3]);

/* frames: uint8 [B,H,W,3] RGB (host pointer if frames_on_device == 0, else device pointer).
 * Outputs follow the TFLite_Detection_PostProcess signature read at reference odt.py:64-66:
 *   boxes  float32 [B,25,4]  (ymin,xmin,ymax,xmax) normalised   = output_3
 *   scores float32 [B,25]                                        = output_1
 *   classes float32 [B,25]                                       = output_2
 *   counts int32   [B]                                           = output_0
 * Output pointers are host (outputs_on_device == 0; the call synchronises the stream) or device. */
int vbt_detect(vbt_model* m, const uint8_t* frames, int B, int frames_on_device, void* stream,
               float* boxes, float* scores, float* classes, int32_t* counts, int outputs_on_device);

/* Enqueue only (no copies, no sync): frames and outputs are device pointers. Used by the fused
 * pipeline and by bench.py inside HIP-event brackets. */
int vbt_detect_async(vbt_model* m, const uint8_t* frames_dev, int B, void* stream,
                     float* boxes_dev, float* scores_dev, float* classes_dev, int32_t* counts_dev);

/* A part of the forward: plan steps [step0, step1) (step1 < 0: to the end; vbt_model_num_launches of them) on images
 * [img0, img0 + n_img) of the model's max_batch-image tensors.  The detector is per-image, so a batch may be brought through the
 * network entry a few images at a time and through the rest at once: steps [0, vbt_model_entry_steps) - the stem convolution, with
 * block 0 where the plan fuses the two - on images [g n, (g + 1) n) as they arrive, then steps [entry, end) on images [0, G n).
 * frames_dev = the n_img frames of the range (NULL when step0 >= vbt_model_entry_steps); the output pointers are those of image 0
 * of the batch, as vbt_detect_async takes them (NULL when the range ends before decode + NMS).  Steps behind the entry run from
 * img0 = 0 only (VBT_ERR_ARG otherwise).  Enqueue only; never replayed from a graph. */
int vbt_detect_range_async(vbt_model* m, const uint8_t* frames_dev, int img0, int n_img, int step0, int step1, void* stream,
                           float* boxes_dev, float* scores_dev, float* classes_dev, int32_t* counts_dev);
/* plan steps that form the network entry: every step up to the last one that reads the frames; all tensors behind it are materialised */
int vbt_model_entry_steps(const vbt_model* m);

/* Streams for a pipeline that keeps several forwards in flight (the reference runs one interpreter.invoke() at a time,
 * odt.py:58-61; there is no reference counterpart).  A HIP stream is bound to a hardware queue at its first command,
 * round-robin: the stream returned here has already run one empty launch, so streams created back to back use distinct
 * queues, whatever a framework's stream pool has been used for before. */
int vbt_stream_create(int device, void** stream_out);
int vbt_stream_destroy(void* stream);

/* preprocess_image (reference odt.py:10-19): bilinear resize (half-pixel centres, float32) of
 * uint8 [B,H,W,3] frames to [B,h,w,3] + truncating uint8 cast; swap_rb != 0 also swaps channels 0
 * and 2 (cv2 BGR -> RGB, reference track.py:171).  src/dst are host or device pointers. */
int vbt_resize_frames(const uint8_t* src, int B, int H, int W, int src_on_device, uint8_t* dst, int h, int w,
                      int dst_on_device, int swap_rb, int device, void* stream);

/* Pixel formats of source frames.  VBT_PIX_RGB24 (the default everywhere): packed uint8 [H,W,3].  The two YUV 4:2:0 formats are
 * what a video decoder emits (`ffmpeg -pix_fmt nv12|yuv420p -f rawvideo`); a frame is H*W*3/2 bytes, H and W even, the frames of a
 * clip contiguous:
 *   VBT_PIX_NV12: H*W luma bytes, then H/2 rows of interleaved U,V (W bytes per row);
 *   VBT_PIX_I420: H*W luma bytes, then an H/2 x W/2 U plane, then an H/2 x W/2 V plane.
 * Arithmetic contract.  Source pixel (y, x) has luma Y[y][x] and the chroma sample at (y >> 1, x >> 1), taken nearest (no chroma
 * interpolation).  BT.601 limited range in 20-bit fixed point, all int32, >> arithmetic, clip8 saturating to 0..255:
 *   Yp = max(0, Y - 16);  u = U - 128;  v = V - 128
 *   R = clip8((1220542*Yp             + 1673527*v + (1<<19)) >> 20)
 *   G = clip8((1220542*Yp -  409993*u -  852492*v + (1<<19)) >> 20)
 *   B = clip8((1220542*Yp + 2116026*u             + (1<<19)) >> 20)
 * Those uint8 RGB values go through the arithmetic of vbt_resize_frames unchanged (float32 bilinear, truncating cast), in one
 * kernel: no full-resolution RGB frame is written.  A source already at h x w is still converted. */
#define VBT_PIX_RGB24 0
#define VBT_PIX_NV12 1
#define VBT_PIX_I420 2
/* vbt_resize_frames for YUV 4:2:0 sources: src = B frames of H*W*3/2 bytes, dst = uint8 [B,h,w,3] RGB.  VBT_ERR_ARG, before any
 * device call: H or W odd, an unknown pix_fmt, or VBT_PIX_RGB24 (that is vbt_resize_frames). */
int vbt_resize_frames_yuv(const uint8_t* src, int B, int H, int W, int pix_fmt, int src_on_device, uint8_t* dst, int h, int w,
                          int dst_on_device, int device, void* stream);

/* More source formats, and the colour description of every YUV format.  Codes 3..15 are unknown.
 *   VBT_PIX_YUYV422 (`yuyv422`, UVC / v4l2 webcams): H rows of 2W bytes, Y0 U Y1 V per pixel pair;
 *   VBT_PIX_UYVY422 (`uyvy422`, SDI / HDMI capture cards): H rows of 2W bytes, U Y0 V Y1 per pixel pair;
 *   VBT_PIX_P010 (`p010le`, 10-bit hardware decoders): the NV12 layout in 16-bit little-endian words - H*W luma words, then H/2 rows
 *     of interleaved U,V words (W words per row).  The sample is word >> 6; the low 6 bits are ignored.
 * Sizes: the 4:2:2 formats take any H >= 1 and an even W >= 2, P010 even H and W >= 2; no side above 16384.
 * Chroma, taken nearest: 4:2:2 pixel (y, x) uses the sample of its own pair, (y, x >> 1); P010 uses (y >> 1, x >> 1).
 * Colour description: a matrix (VBT_CS_*) and a range (VBT_RANGE_*); (VBT_CS_BT601, VBT_RANGE_LIMITED) is the default everywhere.
 * It applies to all five YUV formats (ffmpeg's yuvj420p is VBT_PIX_I420 with VBT_RANGE_FULL).
 * Arithmetic contract, all int32, >> arithmetic, clip8 saturating to 0..255:
 *   Yp = max(0, Y - YOFF);  u = U - COFF;  v = V - COFF
 *   R = clip8((CY*Yp            + CRV*v + (1<<19)) >> 20)
 *   G = clip8((CY*Yp - CGU*u    - CGV*v + (1<<19)) >> 20)
 *   B = clip8((CY*Yp + CBU*u            + (1<<19)) >> 20)
 * YOFF / COFF: 8-bit limited 16 / 128, 8-bit full 0 / 128, 10-bit limited 64 / 512, 10-bit full 0 / 512.  The 8-bit BT.601 limited
 * coefficients are those of VBT_PIX_NV12 above (rounded from three decimals), for every 8-bit format.  Every other row is
 * C = floor(x * 2^20 + 0.5) in double precision with CY = 255/ys, CRV = 2(1-Kr)*255/cs, CGU = 2(1-Kb)Kb/Kg*255/cs,
 * CGV = 2(1-Kr)Kr/Kg*255/cs, CBU = 2(1-Kb)*255/cs; (Kr, Kb) = (0.299, 0.114) for BT.601, (0.2126, 0.0722) for BT.709, Kg = 1-Kr-Kb;
 * (ys, cs) = (219, 224) 8-bit limited, (255, 255) 8-bit full, (876, 896) 10-bit limited, (1023, 1023) 10-bit full:
 *   matrix, depth, range      CY      CRV     CGU     CGV     CBU
 *   601,  8, limited     1220542  1673527  409993  852492  2116026
 *   601,  8, full        1048576  1470104  360853  748826  1858077
 *   601, 10, limited      305236   418389  102698  213115   528805
 *   601, 10, full         261375   366448   89949  186658   463157
 *   709,  8, limited     1220945  1879825  223607  558796  2215014
 *   709,  8, full        1048576  1651297  196424  490864  1945738
 *   709, 10, limited      305236   469956   55902  139699   553753
 *   709, 10, full         261375   411614   48962  122356   485008
 * (the largest intermediate is about 5.8e8).  The uint8 RGB then goes through the arithmetic of vbt_resize_frames, in the same
 * kernel, as for VBT_PIX_NV12.  Drawing, scaling and JPEG-encoding frames (overlay, scaler, mjpeg handles below) know neither the
 * new formats nor a colour description: there 16..18 are unknown formats. */
#define VBT_PIX_YUYV422 16
#define VBT_PIX_UYVY422 17
#define VBT_PIX_P010 18
#define VBT_CS_BT601 0
#define VBT_CS_BT709 1
#define VBT_RANGE_LIMITED 0
#define VBT_RANGE_FULL 1
/* Bytes of one H x W frame: H*W*3 (RGB24), H*W*3/2 (NV12, I420), H*W*2 (4:2:2), H*W*3 (P010).  0 for an unknown format or a size the
 * format refuses: H or W < 1, an odd side where the format's chroma needs an even one, a side above 16384 for the 4:2:2 formats and
 * P010.  RGB24, NV12 and I420 have no upper limit here, as they have none in the pipeline.  Host only. */
size_t vbt_pix_frame_bytes(int H, int W, int pix_fmt);
/* vbt_resize_frames for any YUV format under a colour description: src = B frames of vbt_pix_frame_bytes each, dst = uint8
 * [B,h,w,3] RGB.  VBT_ERR_ARG, before any device call, the text naming the argument: an unknown pix_fmt, matrix or range, a size
 * the format refuses or, in any format, a side above 16384, VBT_PIX_RGB24 (that is vbt_resize_frames), or a device source of a 4:2:2 or P010 format that is not 4-byte
 * aligned (the kernel loads a pixel pair as one dword; host sources are staged and may have any alignment). */
int vbt_resize_frames_pix(const void* src, int B, int H, int W, int pix_fmt, int matrix, int range, int src_on_device,
                          uint8_t* dst, int h, int w, int dst_on_device, int device, void* stream);

/* ------------------------------------------------------------------ tracker -----------------
 * Replaces ocsort.OCSort (reference track.py:17,157,186-199), the row assembly of
 * reference track.py:189-234 and the export id selection of track.py:107-115.
 * One handle tracks `n_clips` independent clips in parallel (one wavefront per clip).
 */
typedef struct vbt_tracker vbt_tracker;
typedef struct {
  int32_t max_age;       /* reference track.py:22,157 -> 30 */
  int32_t min_hits;      /* OC-SORT default 3 */
  int32_t delta_t;       /* OC-SORT default 3 (1..3 supported) */
  int32_t asso;          /* second-round association: 0 = iou, 1 = diou (reference track.py:157) */
  double iou_threshold;  /* reference track.py:157 -> 0.1 */
  double inertia;        /* OC-SORT default 0.2 */
  double det_thresh;     /* OC-SORT score gate (detections with score <= det_thresh are dropped) */
} vbt_tracker_params;

/* rows_cap: capacity of the per-clip row log (rows = emitted (id,time,...) records). */
int vbt_tracker_create(int n_clips, int rows_cap, const vbt_tracker_params* p, int device, vbt_tracker** out);
/* The second tracker: sort.tracker.SortTracker, the commented-out alternative of reference track.py:16,156
 * (`SortTracker(max_age=MAX_AGE)`, sort-track 0.0.8), which made the reference's dfs/ result set.  Plain SORT: the same 7-state
 * filter, association on IoU alone (no direction term, no second round, no score gate, no class test), z built with r = w / h
 * (no 1e-6), and rows emitted from the filter's posterior box instead of the observation.  The handle is an ordinary vbt_tracker:
 * every vbt_tracker_* entry below works on it, the row log and everything that reads it are the same.  The fused entries
 * (vbt_tracker_update_from_*) still apply their det_threshold (reference odt.py:70-75); SORT itself drops no detection.
 * id_base: the package's id counter is shared by all trackers of a process (the reference's dfs/ file ids run 1, 3, 7, ..., 94); here
 * it is a parameter - the ids of every clip start at id_base + 1, and vbt_tracker_reset / _reset_clips keep it.
 * VBT_ERR_ARG, before any device call: a NULL pointer, n_clips or rows_cap < 1, max_age < 0, min_hits < 0, iou_threshold not
 * finite, id_base < 0 or above VBT_SORT_MAX_ID_BASE. */
typedef struct {
  int32_t max_age;       /* SortTracker default 1; reference track.py:156 -> 30 */
  int32_t min_hits;      /* SortTracker default 3 */
  int32_t id_base;       /* ids of a clip start at id_base + 1 (0: the first tracker of a process) */
  double iou_threshold;  /* SortTracker default 0.3 */
} vbt_sort_params;
#define VBT_SORT_MAX_ID_BASE 0x3fffffff /* row ids are id_base + 1 + births so far: half of the int32 range is left to the births */
int vbt_tracker_create_sort(int n_clips, int rows_cap, const vbt_sort_params* p, int device, vbt_tracker** out);
void vbt_tracker_destroy(vbt_tracker* t);
int vbt_tracker_reset(vbt_tracker* t);
/* A fresh clip in each of the slots clips[0..n): its OC-SORT state cleared (ids restart at 1), its row log empty, its frame counter 0
 * and - live analysis on - its live record and entries re-initialised, exactly as vbt_tracker_reset leaves a clip; the other clips
 * are untouched.  Enqueue only, on `stream` (the list travels in the kernel arguments).  VBT_ERR_ARG: n < 1, a clip outside
 * 0..n_clips-1 or listed twice. */
int vbt_tracker_reset_clips(vbt_tracker* t, const int32_t* clips, int n, void* stream);

/* OCSort.update for F consecutive frames of every clip (host pointers; synchronous):
 *   dets   float64 [F][n_clips][25][6] = x1,y1,x2,y2,score,cls   (reference odt.py:102-118)
 *   counts int32   [F][n_clips]   (0 = empty frame: the tracker is not stepped, track.py:180-181)
 *   times  float64 [F][n_clips]   (frame_count / fps, reference track.py:169) */
int vbt_tracker_update(vbt_tracker* t, const double* dets, const int32_t* counts, const double* times, int F);

/* Fused path: one frame per clip straight from vbt_detect_async's device outputs; applies the
 * detection threshold of reference odt.py:70-75 (score >= det_threshold). times_host [n_clips]; a negative time marks a
 * clip that has no frame in this step (clips of different lengths batched together): its state is left untouched.
 * The host arrays are read during the call and travel in the kernel arguments (64 slots per launch): no host-to-device
 * copy is enqueued, the caller may reuse them as soon as the call returns. */
int vbt_tracker_update_from_detections(vbt_tracker* t, const float* boxes_dev, const float* scores_dev,
                                       const int32_t* counts_dev, const double* times_host, float det_threshold,
                                       void* stream);
/* The same with fewer detector slots than clips: slot i of the batch carries a frame of clip clip_of_slot_host[i]
 * (-1: none), times_host is per slot.  A slot can move on to the next clip of its queue when one ends, so a corpus of
 * clips of different lengths keeps every slot of the detector batch busy (the reference runs clips one after the other,
 * track.py:85-126).  Export ids / rows / phases stay per clip. */
int vbt_tracker_update_from_slots(vbt_tracker* t, const float* boxes_dev, const float* scores_dev, const int32_t* counts_dev,
                                  const int32_t* clip_of_slot_host, const double* times_host, int n_slots, float det_threshold,
                                  void* stream);

/* Time-batched form.  The reference's unit of work is ONE video (track.py:85-126): `while cap.isOpened()` reads frame
 * after frame of one clip (track.py:159-247).  The detector has no state, so a batch may hold RUNS of consecutive frames of
 * a clip instead of one frame of each of B clips; the tracker then walks every run in frame order inside one launch (one
 * wavefront per run).  Frame f (0-based) of a run sits in detector slot slot0 + f * slot_stride and is the reference's
 * frame number frame_count = frame0 + f * frame_step (track.py:161; frame_step = the `frame_count % 16` stride of
 * track.py:166, normally 1); its time stamp is frame_count / fps (track.py:169), one IEEE double division.  Frames on which
 * run_odt returns [] do not step the tracker (track.py:180-181).  A clip may appear in at most one run per call; calls on
 * one stream are ordered, so consecutive calls continue a clip.  runs_host is read during the call (kernel arguments). */
typedef struct {
  int32_t clip;         /* tracker clip the run belongs to (< 0: descriptor ignored) */
  int32_t slot0;        /* detector slot of the run's first frame */
  int32_t slot_stride;  /* 1: the run's frames are neighbours in the batch */
  int32_t n_frames;     /* frames in the run */
  int32_t frame0;       /* 1-based frame number of the first frame */
  int32_t frame_step;   /* frame-number increment per frame of the run (>= 1) */
  double fps;           /* cap.get(cv2.CAP_PROP_FPS), reference track.py:138 */
} vbt_run;
int vbt_tracker_update_from_detections_seq(vbt_tracker* t, const float* boxes_dev, const float* scores_dev,
                                           const int32_t* counts_dev, int n_slots, const vbt_run* runs_host, int n_runs,
                                           float det_threshold, void* stream);

/* Assemble a detector batch from frames that live elsewhere in device memory (frame runs of different clips, or a clip
 * whose frames are cycled): dst_dev[i] = *src_frames_host[i] for i < n_frames, frame_bytes each (a multiple of 16; all
 * pointers 16-byte aligned).  src_frames_host is an array of DEVICE pointers held in host memory; it is read during the
 * call (kernel arguments).  One launch per 64 frames, enqueued on `stream`. */
int vbt_gather_frames(uint8_t* dst_dev, const uint8_t* const* src_frames_host, int n_frames, size_t frame_bytes, void* stream);

/* What OCSort.update returned for the clip's most recent stepped frame: out7 [M,7] =
 * x1,y1,x2,y2,id(1-based),cls,score (reference track.py:190) and vel2 [M,2] = kf.x[4:6] of the
 * same track (reference track.py:194-199). */
int vbt_tracker_last_output(vbt_tracker* t, int clip, double* out7, double* vel2, int cap, int* M);
/* tracker.trackers: ids (0-based, reference track.py:195) and kf.x (7 values each) in list order */
int vbt_tracker_get_trackers(vbt_tracker* t, int clip, int32_t* ids, double* kfx, int cap, int* n);
int vbt_tracker_status(vbt_tracker* t, int clip, int32_t* n_rows, int32_t* n_trackers, int32_t* overflow,
                       int32_t* rows_overflow, int32_t* frame_count);
/* The clip's row log in emission order = the dict of reference track.py:144-145,227-234:
 * id int64 [n]; cols7 float64 [n,7] = time,x,y,dx,dy,norm_plate_height,norm_plate_width */
int vbt_tracker_rows(vbt_tracker* t, int clip, int64_t* id, double* cols7, int cap, int* n);

/* End of clips: pick each clip's id with the largest cumulative path length (reference
 * track.py:107-115) and run plot.py's preprocessing + VelocityTracker over its rows on device. */
int vbt_tracker_finish(vbt_tracker* t, double plate_diameter, double diff_threshold, double min_distance, void* stream);
/* phases6 [P,6] = time_start,time_end,y_start,y_end,rom,type (reference Phase.py:16-22).  VBT_ERR_CAPACITY, as vbt_tracker_rows,
 * for a clip that dropped births (more than 64 live tracks) or rows (rows_cap): its log is not the reference's. */
int vbt_tracker_phases(vbt_tracker* t, int clip, int32_t* best_id, double* phases6, int cap, int* P);
/* Clip close of every clip at once (arrays of n_clips entries; phases6 is [n_clips][cap][6], rows beyond n_phases[c] are
 * not written): export ids, DataFrame row counts, phase counts and overflow flags are packed on the device into one
 * block, fetched by ONE asynchronous copy into pinned memory and ONE synchronisation of the stream vbt_tracker_finish ran
 * on (not of the device). */
int vbt_tracker_summary(vbt_tracker* t, int32_t* best_ids, int32_t* n_rows, int32_t* n_phases, int32_t* overflow, double* phases6, int cap);
/* DataFrame rows (reference track.py:227-234) of EVERY clip in one strided device-to-host copy on `stream` (which the
 * call synchronises): rows_host = [n_clips][cap] records of 64 bytes {int64 id; double time, x, y, dx, dy,
 * norm_plate_height, norm_plate_width}, all ids in emission order; counts[c] = number of rows of clip c.
 * rows_host may be pinned host memory (one DMA) or pageable. */
int vbt_tracker_rows_all(vbt_tracker* t, int32_t* counts, void* rows_host, int cap, void* stream);
/* The row log of `clip` where it lives, in device memory: *rows_dev = its 64-byte records in emission order (room for *rows_cap),
 * *nrows_dev = the device int32 that counts them (never above *rows_cap; vbt_tracker_reset / _reset_clips set it back to 0).
 * Borrowed pointers, valid until the tracker is destroyed; no device call.  VBT_ERR_ARG: a NULL argument, a clip out of range. */
int vbt_tracker_rows_dev(vbt_tracker* t, int clip, const void** rows_dev, const int32_t** nrows_dev, int* rows_cap);

/* Live rep analysis (off unless enabled): per-rep ROM / ACV while the clips are still being tracked.
 * After every tracker launch one more kernel on the same stream feeds the rows it appended to the log, in emission order, to the
 * preprocessing of reference plot.py:90-95 and a VelocityTracker (VelocityTracker.py:92-158) per id - for every id that can still win
 * the export (a live track, or the best dead id: at most 65 per clip).  Guarantee: the phases of such an id equal reference
 * VelocityTracker(plate_diameter, diff_threshold, min_distance).phases fed the preprocessed rows of the id emitted so far, bit for bit
 * (the close-time scan and the live path share one per-row step); with flush_view, that list after end_processing() - computed on a
 * copy, the live state is not touched.  The clip's leader is the id vbt_tracker_finish would export if the clip closed now
 * (track.py:107-115).  After the last frame, the leader and its flush view are exactly the close's export id and phases.
 * Capacities are reported, never guessed around: an id whose open phase outgrows path_cap samples or whose list outgrows phase_cap
 * phases is frozen and flagged, a clip whose row log overflowed is flagged, and a flagged id / clip reports no phases. */
#define VBT_LIVE_PATH_FULL 1      /* the open phase's bar path outgrew path_cap */
#define VBT_LIVE_PHASES_FULL 2    /* the phase list outgrew phase_cap */
#define VBT_LIVE_ROWS_LOST 4      /* the clip's row log overflowed (rows_cap): rows never reached the analysis */
#define VBT_LIVE_MAX_PATH 65536
#define VBT_LIVE_MAX_PHASES 512
typedef struct {
  int64_t leader_id;              /* the export rule applied to the rows so far (-1: no id has 2 rows yet) */
  int32_t rows_consumed;          /* rows of the clip's log analysed */
  int32_t n_phases;               /* phases of the leader (0 when overflow != 0) */
  int32_t phase_state;            /* the leader's VelocityTracker state: 0 concentric, 1 eccentric, 2 hold */
  int32_t overflow;               /* VBT_LIVE_* bits of the clip and its leader */
  uint64_t seq;                   /* bumped whenever the leader or its phase list changes */
} vbt_live_clip;
/* Before the first update (or after vbt_tracker_reset), else VBT_ERR_STATE; once per tracker.  path_cap in [2, VBT_LIVE_MAX_PATH],
 * phase_cap in [1, VBT_LIVE_MAX_PHASES], else VBT_ERR_ARG.  VelocityTracker parameters as in vbt_tracker_finish.  Allocates
 * n_clips x 65 x (5 path_cap + 6 phase_cap) doubles.  vbt_tracker_reset clears the live state too. */
int vbt_tracker_live_enable(vbt_tracker* t, int path_cap, int phase_cap, double plate_diameter, double diff_threshold, double min_distance);
/* Every clip's record and its leader's phases6 [n_clips][cap][6]: one pack launch on `stream` (which must follow the tracker launches
 * of interest), ONE copy, ONE synchronisation of `stream`.  VBT_ERR_STATE when live analysis is not enabled. */
int vbt_tracker_live_poll(vbt_tracker* t, int flush_view, vbt_live_clip* clips, double* phases6, int cap, void* stream);
/* Every analysed id of one clip (the ids that can still win, with at least one row): ids, rows consumed, phases, VBT_LIVE_* flags;
 * phases6 [cap_tracks][cap_phases][6].  Synchronises the device (tests, clips with several plates). */
int vbt_tracker_live_tracks(vbt_tracker* t, int clip, int flush_view, int64_t* ids, int32_t* n_rows, int32_t* n_phases, int32_t* flags,
                            double* phases6, int cap_tracks, int cap_phases, int* n);

/* Rep metrics (off unless enabled): eight doubles per phase, formed on the device where the phase's bar path is - in the scan, when
 * the phase is appended to its list - from the very samples and step range its rom is summed over (VelocityTracker.py:171-222), in
 * IEEE double without contraction, sequentially in index order i = st+1 .. en (st / en: the path samples the phase starts / ends at;
 * D = plate_diameter; ddx_i, ddy_i: the per-step terms of rom; dt_i = ts[i] - ts[i-1]; v_i = (ddx_i + ddy_i) / dt_i):
 *   VBT_RM_PV       max v_i (initial value 0.0, a strictly greater value replaces it)          peak velocity, m/s
 *   VBT_RM_T_PV     ts[i] of the first maximum of PV; ts[st] if no step qualified               its time stamp, s
 *   VBT_RM_ROM_Y    sum ddy_i                                                                   vertical travel, m
 *   VBT_RM_ROM_X    sum ddx_i                                                                   horizontal travel, m
 *   VBT_RM_PV_Y     max ddy_i / dt_i (as PV)                                                    peak vertical velocity, m/s
 *   VBT_RM_MV       rom / (ts[en] - ts[st]); 0.0 when that duration is <= 0                     the reference's ACV (plot.py:173)
 *   VBT_RM_X_DEV    max |xs[i] - xs[st]| / ((ws[i] + ws[st]) / 2) * D (initial value 0.0)       largest sideways excursion, m
 *   VBT_RM_N_STEPS  (double)(en - st) when en > st, else 0.0
 * A step with dt_i <= 0 adds to the sums but takes no part in the two velocity maxima (a tracker's row log cannot hold one; rows
 * handed to vbt_analyze_metrics can).  The record travels with its phase: a phase the filter drops later takes its metrics along, so
 * metrics8 [P][8] is always in the order of phases6 [P][6].  Enabling metrics changes no other output. */
#define VBT_REP_METRICS 8
#define VBT_RM_PV 0
#define VBT_RM_T_PV 1
#define VBT_RM_ROM_Y 2
#define VBT_RM_ROM_X 3
#define VBT_RM_PV_Y 4
#define VBT_RM_MV 5
#define VBT_RM_X_DEV 6
#define VBT_RM_N_STEPS 7
/* Before the first update (or after vbt_tracker_reset), else VBT_ERR_STATE; before or after vbt_tracker_live_enable; a second call
 * does nothing.  Allocates n_clips x 512 x 8 doubles (32 KB per clip) for the close and, with live analysis on, n_clips x 65 x
 * phase_cap x 8 doubles for the live tables + n_clips x phase_cap x 8 for the poll's view (at the default phase_cap of 128: 65 KB x
 * 66 = 541 KB per clip). */
int vbt_tracker_rep_metrics_enable(vbt_tracker* t);
/* After vbt_tracker_finish: metrics8 [P][8] of the clip's export id, in the order of vbt_tracker_phases.  VBT_ERR_STATE when metrics
 * are not enabled or before the finish; otherwise refused as vbt_tracker_phases refuses. */
int vbt_tracker_rep_metrics(vbt_tracker* t, int clip, double* metrics8, int cap, int* P);
/* vbt_tracker_summary with metrics8 [n_clips][cap][8] in the same packed block: still ONE copy and ONE stream synchronisation.
 * VBT_ERR_STATE when metrics are not enabled. */
int vbt_tracker_summary_ex(vbt_tracker* t, int32_t* best_ids, int32_t* n_rows, int32_t* n_phases, int32_t* overflow, double* phases6,
                           double* metrics8, int cap);
/* vbt_tracker_live_poll with the leaders' metrics8 [n_clips][cap][8] (with flush_view: those of the appended phase included), in the
 * same packed block: ONE copy, ONE synchronisation.  VBT_ERR_STATE when live analysis or metrics are not enabled. */
int vbt_tracker_live_poll_ex(vbt_tracker* t, int flush_view, vbt_live_clip* clips, double* phases6, double* metrics8, int cap, void* stream);

/* ------------------------------------------------------------------ pipeline ----------------
 * Replaces the clip loop of the reference (track.py:129-260: `while cap.isOpened()` -> cap.read -> run_odt -> OCSort.update ->
 * row assembly, then the export of track.py:103-126 and analyze_df of plot.py:33-47) as ONE object behind the C ABI: SURVEY.md 8b's
 * "fused on-device path".  The handle owns everything the fast path needs and nothing of it lives in the caller's language:
 *   - `depth` detector instances (activation arenas) on `depth` HIP streams of their own, each checked at creation to sit on its own
 *     hardware queue (a pipeline whose busy streams share a queue loses a third of its throughput); the reference runs one
 *     interpreter.invoke() at a time (odt.py:58-61) - the detector has no state, so consecutive steps may overlap;
 *   - a ring of detector output slots and the events that order detector(t) -> tracker(t) -> slot reuse; the OC-SORT steps stay in
 *     frame order (track.py:186 is sequential per clip);
 *   - a copy stream with a ring of depth + 2 device staging buffers: frames handed over in host memory (the reference's situation,
 *     track.py:160) are uploaded up to two steps ahead of their forward; with frames at source resolution only the rows the bilinear
 *     resize of odt.py:10-19 reads are uploaded;
 *   - for batches of <= 8 frames, groups of `depth` tracker steps walked by one launch (the forward of a small batch is launch latency);
 *   - for batches of 32..64 frames, groups of `group` steps behind ONE forward of group x n_slots images: each step call runs the
 *     network entry on its own frames at once - the caller's buffer is consumed exactly as without groups - and the group's last
 *     call (or whatever reads or changes the pipeline's state before it) enqueues the rest of the network and one OC-SORT walk.
 * One handle is used by one host thread at a time.  Every call only ENQUEUES work unless its comment says it synchronises.
 * Frames: uint8 [*,H,W,3]; H,W = the network resolution (vbt_model_input_shape) unless src_h/src_w say otherwise.
 */
typedef struct vbt_pipeline vbt_pipeline;
typedef struct {
  int32_t n_slots;           /* frames per detector batch (>= 1) */
  int32_t n_clips;           /* clips the tracker follows; 0 = n_slots (one clip per slot) */
  int32_t rows_cap;          /* capacity of each clip's row log (rows = emitted (id,time,...) records) */
  int32_t device;
  int32_t depth;             /* forwards in flight, 1..8; 0 = default (environment VBT_PIPELINE_DEPTH, else 4 for n_slots <= 8, else 3) */
  int32_t tracker_stream;    /* where a frame's OC-SORT step runs: 0 = default (VBT_TRACKER_STREAM, else inline from depth 3), 1 = on a
                                stream of its own, 2 = inline at the end of the forward's stream */
  int32_t defer;             /* tracker steps of a small batch walked in groups of `depth`: -1 = default (VBT_TRACKER_DEFER, else on
                                for n_slots <= 8 with one clip per slot), 0 = off, 1 = on */
  int32_t selfcheck;         /* forwards on a blank batch per detector instance at creation: -1 = default (VBT_PIPELINE_SELFCHECK, else 1) */
  int32_t strict_placement;  /* busy streams that cannot be put on distinct hardware queues: 1 = vbt_pipeline_create fails with
                                VBT_ERR_STATE, 0 = a note on stderr, -1 = environment VBT_STRICT_PLACEMENT (default 0) */
  int32_t model_flags;       /* vbt_model_create_ex flags; VBT_MODEL_DEFAULT_FLAGS */
  float detection_threshold; /* detection_treshold of reference track.py:129,174 / odt.py:70-75 */
  int32_t group;             /* consecutive vbt_pipeline_step calls that share ONE forward of group x n_slots images (the network entry still
                                runs inside every call) and one time-batched OC-SORT walk: 0 = default (VBT_PIPELINE_GROUP, else 4 for
                                32 <= n_slots <= 64 with one clip per slot and a plan at that batch - a pinned VBT_PLAN_FILE or no
                                autotuning - else 1), 1 = off, up to 8.  One clip per slot only; replaces `defer` */
  double plate_diameter;     /* VelocityTracker(plate_diameter, diff_threshold, min_distance), reference VelocityTracker.py:16 */
  double diff_threshold;
  double min_distance;
  vbt_tracker_params tracker; /* OCSort(...) of reference track.py:157 */
} vbt_pipeline_params;
/* the reference's settings: OCSort(max_age=30, asso_func="diou", iou_threshold=0.1) (track.py:22,157), threshold 0.5,
 * VelocityTracker(0.45, 0.6, 0.1); everything else 0 / -1 = default */
void vbt_pipeline_default_params(vbt_pipeline_params* p);
/* fps_host [n_clips]: cap.get(cv2.CAP_PROP_FPS) of every clip (reference track.py:138) */
int vbt_pipeline_create(const char* container_path, const vbt_pipeline_params* p, const double* fps_host, vbt_pipeline** out);
/* The pipeline's clips are tracked by SORT (vbt_tracker_create_sort; reference track.py:16,156) instead of OC-SORT from here on:
 * vbt_pipeline_params.tracker is ignored, detection_threshold still applies.  Valid only before the first vbt_pipeline_step /
 * _step_runs / vbt_track_clip of the handle (VBT_ERR_STATE afterwards, a vbt_pipeline_reset does not reopen it); call it before
 * vbt_pipeline_live_enable.  VBT_ERR_ARG as vbt_tracker_create_sort.  Synchronises the device (the clip states are re-initialised). */
int vbt_pipeline_use_sort(vbt_pipeline* p, const vbt_sort_params* sp);
void vbt_pipeline_destroy(vbt_pipeline* p);

/* One frame of every clip: frames = uint8 [n_slots,H,W,3], frame number frame_count + 1 of each clip (track.py:161), time stamp
 * frame_count / fps (track.py:169).  frames_on_device != 0: a device pointer, valid on `caller_stream` when the call is made (the
 * forward waits for that point of the stream) and left untouched until the step has run (up to `depth` steps later).
 * frames_on_device == 0: host memory, final when the call is made; pinned memory is copied by DMA on the copy stream up to two steps
 * ahead and must stay untouched until the step has run; the call blocks only when the caller is depth + 2 steps ahead of the GPU.
 * src_h / src_w > 0: the frames are at source resolution and go through preprocess_image (odt.py:10-19) on the device; swap_rb: BGR
 * input (track.py:171).  active [n_slots] (or NULL): clips that have a frame in this step; the others keep their state and frame
 * counter.  clip_map / frame_idx [n_slots] (or NULL): slot i carries frame number frame_idx[i] (1-based) of clip clip_map[i] (-1:
 * empty slot) - more clips than slots.  track == 0: detector only (measurement splits). */
int vbt_pipeline_step(vbt_pipeline* p, const uint8_t* frames, int frames_on_device, int src_h, int src_w, int swap_rb,
                      const uint8_t* active, const int32_t* clip_map, const int32_t* frame_idx, int track, void* caller_stream);
/* Time-batched step: the batch holds RUNS of consecutive frames of a clip (vbt_run; fps <= 0 = the clip's own, slot_stride 0 = 1);
 * OC-SORT walks every run in frame order inside one launch.  Either `frames` is the assembled batch [B,H,W,3] (B = slots the runs
 * cover) or it is NULL and run_sources[i] points at the n_frames contiguous frames of run i (all device or all host): the batch is
 * then assembled here (one gather launch, or one copy per run on the copy stream).  The runs must cover slots 0..B-1 without a hole.
 * out_* != NULL (with track == 0): the detections go to these device buffers ([B,25,4], [B,25], [B,25], [B]) instead of the ring -
 * the frame-major multi-GPU mode collects them for its gather. */
int vbt_pipeline_step_runs(vbt_pipeline* p, const uint8_t* frames, const uint8_t* const* run_sources, int frames_on_device,
                           const vbt_run* runs, int n_runs, int src_h, int src_w, int swap_rb, int track,
                           float* out_boxes, float* out_scores, float* out_classes, int32_t* out_counts, void* caller_stream);
/* Pixel format (VBT_PIX_*) of the frames of every later vbt_pipeline_step, vbt_pipeline_step_runs and vbt_track_clip on this handle;
 * VBT_PIX_RGB24 is the default and restores it.  With a YUV format those calls take frames of src_h*src_w*3/2 bytes (that is the frame
 * stride of batches, run sources and clips), src_h and src_w must be given, > 0 and even, and swap_rb must be 0 - else VBT_ERR_ARG
 * with nothing enqueued and no state changed.  Conversion and resize run fused on the device (see VBT_PIX_NV12 above); host frames
 * of a source more than twice as tall as the network input upload only the luma row pairs the resize reads plus the chroma
 * plane(s).  VBT_ERR_ARG: an unknown format.
 * VBT_PIX_YUYV422 / VBT_PIX_UYVY422 / VBT_PIX_P010 are accepted too: the frame stride is vbt_pix_frame_bytes(src_h, src_w, format),
 * the size rules are the format's (4:2:2: any src_h, even src_w; P010: both even; none above 16384), and device frames must be
 * 4-byte aligned - else VBT_ERR_ARG in the same way.  (NV12 / I420 keep their rule as it was: even sides, no upper limit.)  The compact upload of a 4:2:2 source is that of RGB24 with rows of 2W bytes
 * (every row carries its own chroma); that of P010 is NV12's with rows of 2W bytes. */
int vbt_pipeline_set_pixel_format(vbt_pipeline* p, int pix_fmt);
/* Colour description (VBT_CS_*, VBT_RANGE_*) of the YUV frames of every later step call on this handle, read like the pixel format;
 * the default is (VBT_CS_BT601, VBT_RANGE_LIMITED).  It is kept but ignored while the format is VBT_PIX_RGB24.  VBT_ERR_ARG, nothing
 * changed: an unknown matrix or range. */
int vbt_pipeline_set_colour(vbt_pipeline* p, int matrix, int range);
/* frames read from the source but not processed (`frame_count % 16`, track.py:161-167): they advance the clip time only */
int vbt_pipeline_skip_frames(vbt_pipeline* p, int n);
int vbt_pipeline_set_frame_count(vbt_pipeline* p, int frame_count);
/* back to frame 0 of fresh clips; models, streams and buffers are kept; unread slot-close results are dropped (synchronises) */
int vbt_pipeline_reset(vbt_pipeline* p);
/* `stream` waits for every forward enqueued so far (after detector-only steps their outputs are then safe to read on it) */
int vbt_pipeline_join_detectors(vbt_pipeline* p, void* stream);
/* Clip close (track.py:103-126 export id, plot.py:33-47,87-95 rep analysis) of every clip: drains the pipeline, runs both on the
 * device, then ONE packed copy and ONE stream synchronisation.  Arrays of n_clips entries; phases6 [n_clips][cap][6].  Any of the
 * output pointers may be NULL (vbt_pipeline_finish = close without the read-back, synchronises too). */
int vbt_pipeline_close(vbt_pipeline* p, int32_t* best_ids, int32_t* n_rows, int32_t* n_phases, int32_t* overflow, double* phases6, int cap);
int vbt_pipeline_finish(vbt_pipeline* p);
/* Slot close: one clip ends while the others keep running, and a new clip starts in its tracker slot (a host whose clips arrive and
 * end at different times).  The result of a closed slot is what vbt_pipeline_close gives for that clip at that point, bit for bit. */
typedef struct {
  int32_t clip;      /* tracker slot the clip was closed from */
  int32_t best_id;   /* export id (track.py:107-115), -1: none */
  int32_t n_rows;    /* rows of the clip's log, all ids */
  int32_t n_phases;  /* phases of best_id */
  int32_t overflow;  /* tracker overflow | rows_overflow, as vbt_pipeline_close reports it */
  int32_t reserved;
} vbt_closed_clip;
/* Allocates what the slot close needs, once, so that no close allocates: per tracker clip a pinned record (24.6 KB), a device row outbox
 * (rows_cap x 64 bytes) and an event, and the stream rows are read back on.  Call it after vbt_pipeline_create; a second call does
 * nothing.  Synchronous (allocation). */
int vbt_pipeline_close_clips_enable(vbt_pipeline* p);
/* Enqueue the close of `n` slots and their reset to fresh clips; next_fps [n] or NULL (keep). Does not synchronise.
 * Every frame of a listed slot handed to a step before the call is covered (held-back tracker steps are enqueued first,
 * vbt_pipeline_drain); on the tracker stream the export id + rep analysis of the listed clips run (plot.py:33-47), their records go to
 * pinned memory and their rows into the slot's outbox, and the slots are reset (vbt_tracker_reset_clips); every later tracker launch
 * waits for the reset.  Only kernels, event records and event waits are enqueued: no allocation, no copy, no host wait.  The next step
 * may carry frames of the new clip at once: its plain-step frame numbers restart at 1 (time 1 / fps), as do those of `active` steps;
 * clip_map / run steps number frames themselves.  VBT_ERR_ARG: a slot out of range or listed twice, next_fps <= 0; VBT_ERR_STATE: the
 * slot close is not enabled (vbt_pipeline_close_clips_enable), or a listed slot still holds an unread result (vbt_pipeline_closed_clip). */
int vbt_pipeline_close_clips(vbt_pipeline* p, const int32_t* clips, int n, const double* next_fps);
/* The unread result of slot `clip`: wait = 0 never blocks (*ready = 0 until the device has done the close), wait = 1 waits for
 * that close only. phases6 [cap_phases][6]; rows_host [cap_rows] 64-byte records (NULL: rows not copied).
 * Once the close is done, rows_host != NULL copies the clip's whole log (emission order, the record of vbt_tracker_rows_all) on the
 * pipeline's read stream, after this close only, and waits for that copy (n_rows x 64 bytes) - with wait = 0 too; the record and the
 * phases need no copy.  A successful read (ready = 1) releases the slot's result.  VBT_ERR_STATE: nothing pending for `clip`;
 * VBT_ERR_CAPACITY: cap_phases < n_phases or (rows_host != NULL) cap_rows < n_rows - the result stays readable.  vbt_pipeline_reset
 * drops unread results. */
int vbt_pipeline_closed_clip(vbt_pipeline* p, int clip, int wait, int* ready, vbt_closed_clip* rec, double* phases6, int cap_phases,
                             void* rows_host, int cap_rows);
/* enqueue every tracker step still held back (deferred groups, the `depth - 1` steps the own-stream mode keeps ahead); no synchronisation */
int vbt_pipeline_drain(vbt_pipeline* p);
/* vbt_tracker_rows_all / vbt_tracker_rows / vbt_tracker_phases after draining the pipeline (synchronise) */
int vbt_pipeline_rows_all(vbt_pipeline* p, int32_t* counts, void* rows_host, int cap);
int vbt_pipeline_rows(vbt_pipeline* p, int clip, int64_t* id, double* cols7, int cap, int* n);
/* most recent step's detector outputs copied to host arrays [B,25,4], [B,25], [B,25], [B] (synchronises that forward; tests) */
int vbt_pipeline_detections(vbt_pipeline* p, float* boxes, float* scores, float* classes, int32_t* counts, int cap_slots, int* B);
/* measurement split: `count` tracker steps of all clips on the detections sitting in ring slot `slot` */
int vbt_pipeline_tracker_only_steps(vbt_pipeline* p, int count, int slot);
/* Live rep analysis of the pipeline's clips (vbt_tracker_live_enable with the VelocityTracker parameters of vbt_pipeline_params):
 * before the first step (or after vbt_pipeline_reset), else VBT_ERR_STATE.  The analysis then runs on the tracker's stream right
 * after every tracker launch, whichever path launched it. */
int vbt_pipeline_live_enable(vbt_pipeline* p, int path_cap, int phase_cap);
/* Drains the tracker steps still held back (vbt_pipeline_drain), then vbt_tracker_live_poll on the tracker stream: waits for the last
 * tracker launch only, ONE packed copy.  phases6 [n_clips][cap][6] = the leaders' phases. */
int vbt_pipeline_live_poll(vbt_pipeline* p, int flush_view, vbt_live_clip* clips, double* phases6, int cap);
/* Rep metrics of the pipeline's clips (vbt_tracker_rep_metrics_enable): before the first step (or after vbt_pipeline_reset), else
 * VBT_ERR_STATE; before or after vbt_pipeline_live_enable / vbt_pipeline_close_clips_enable.  With the slot close enabled it adds a
 * pinned block of 32 KB per tracker clip.  The _ex calls below are their twins with a metrics8 out-array ([..][8] wherever the twin
 * has phases6 [..][6]) and VBT_ERR_STATE when metrics are not enabled; a slot's metrics are those of the clip just closed in it. */
int vbt_pipeline_rep_metrics_enable(vbt_pipeline* p);
int vbt_pipeline_close_ex(vbt_pipeline* p, int32_t* best_ids, int32_t* n_rows, int32_t* n_phases, int32_t* overflow, double* phases6,
                          double* metrics8, int cap);
int vbt_pipeline_closed_clip_ex(vbt_pipeline* p, int clip, int wait, int* ready, vbt_closed_clip* rec, double* phases6, double* metrics8,
                                int cap_phases, void* rows_host, int cap_rows);
int vbt_pipeline_live_poll_ex(vbt_pipeline* p, int flush_view, vbt_live_clip* clips, double* phases6, double* metrics8, int cap);
typedef struct {
  int32_t n_slots, n_clips, rows_cap, device, depth, ring, defer, tracker_inline, image_size, frame_count, steps_enqueued, placement_ok;
  int32_t queue_groups_seen;  /* distinct hardware queues the placement probe has seen on this device */
  int32_t group;              /* steps per forward (1: every step runs its own forward) */
  int32_t next_slot;          /* detector instance / stream (index into det_streams) the next step call enqueues on */
  int32_t reserved[1];
  void* det_streams[8];
  void* copy_stream;
  void* tracker_stream;
  uint64_t h2d_bytes;         /* bytes copied host -> device by this pipeline so far */
  uint64_t step_host_ns;      /* host time spent inside vbt_pipeline_step / _step_runs so far (enqueue cost incl. any back-pressure wait) */
  uint64_t step_calls;        /* ... over this many calls (both zeroed by vbt_pipeline_reset) */
} vbt_pipeline_info;
int vbt_pipeline_get_info(const vbt_pipeline* p, vbt_pipeline_info* out);
/* borrowed handles (owned by the pipeline): detector instance k < depth, the tracker */
vbt_model* vbt_pipeline_model(vbt_pipeline* p, int k);
vbt_tracker* vbt_pipeline_tracker(vbt_pipeline* p);

/* track(src, interpreter, detection_treshold, ...) of reference track.py:129-260 for ONE clip held in memory: T frames uint8
 * [T,H,W,3] (host or device; any resolution: src_h/src_w as above, 0 = network resolution), every frame_stride-th frame processed
 * (track.py:166), `p` created with n_clips = 1; n_slots consecutive kept frames per detector batch.  Returns the clip's rows in
 * emission order = the dict of track.py:144-145,227-234 (id int64 [n]; cols7 float64 [n,7] = time,x,y,dx,dy,h,w).  Synchronises. */
int vbt_track_clip(vbt_pipeline* p, const uint8_t* frames, int frames_on_device, int T, int src_h, int src_w, int swap_rb,
                   int frame_stride, int64_t* id, double* cols7, int cap, int* n_rows);

/* Pinned host memory for callers without a runtime of their own (frames handed to vbt_pipeline_step from it are copied by DMA) */
int vbt_host_alloc(size_t bytes, void** out);
int vbt_host_free(void* ptr);
int vbt_device_alloc(int device, size_t bytes, void** out);
int vbt_device_free(void* ptr);
/* blocking copies for the same callers (kind: 0 = host -> device, 1 = device -> host) */
int vbt_memcpy(void* dst, const void* src, size_t bytes, int kind);
int vbt_stream_synchronize(void* stream);
int vbt_device_synchronize(int device);

/* ------------------------------------------------------------------ rep analysis ------------
 * Replaces VelocityTracker (reference VelocityTracker.py:15-230) as driven by analyze_df
 * (reference plot.py:33-47): cols7 [T,7] = time,x,y,dx,dy,norm_plate_height,norm_plate_width
 * of one track. preprocess != 0 applies plot.py:90-95 (rolling(5)/expanding means) first;
 * flush != 0 runs end_processing(). */
int vbt_analyze(const double* cols7, int T, int preprocess, int flush, double plate_diameter, double diff_threshold,
                double min_distance, double* phases6, int cap, int* P, int device);

/* vbt_analyze + the rep metrics ("Rep metrics" above) of its phases: metrics8 [P][8]; phases6 is what vbt_analyze returns. */
int vbt_analyze_metrics(const double* cols7, int T, int preprocess, int flush, double plate_diameter, double diff_threshold,
                        double min_distance, double* phases6, double* metrics8, int cap, int* P, int device);

/* The report of a set: the concentric phases (type 0) of one id in list order are its reps k = 1..n, mv_k / pv_k their VBT_RM_MV /
 * VBT_RM_PV.  best_k = max over j <= k of mv_j; loss_k = 100 * (1 - mv_k / best_k), 0 when best_k <= 0.  Sums run in list order;
 * means are over the reps and 0 when there are none. */
typedef struct {
  int32_t n_reps;         /* concentric phases */
  int32_t best_rep;       /* 1-based rep of best_mv (ties: the earlier rep); 0: no rep */
  int32_t stop_rep;       /* first k with loss_k >= stop_loss_pct; 0: none, or stop_loss_pct <= 0 */
  int32_t reserved;
  double best_mv, last_mv, mean_mv;
  double mean_pv, max_pv;
  double loss_last_pct;   /* loss_n */
  double concentric_s, eccentric_s;   /* summed time_end - time_start of the phases of type 0 / type 1 */
  double mean_x_dev;
} vbt_set_report;
/* phases6 [P][6], metrics8 [P][8] as the calls above return them.  loss_pct [cap]: loss_k of the first min(n_reps, cap) reps (the
 * report covers every rep whatever cap is).  Host only: no device call, usable without a GPU.  VBT_ERR_ARG: a NULL pointer (phases6 /
 * metrics8 may be NULL when P == 0, loss_pct when cap == 0), P < 0, cap < 0, a stop_loss_pct that is not finite. */
int vbt_set_summary(const double* phases6, const double* metrics8, int P, double stop_loss_pct, vbt_set_report* out, double* loss_pct, int cap);

/* Trailing / expanding window means of the columns of a row-major float64 table rows[T][ncols] (ncols <= 64),
 * bit-identical to pandas `Series.rolling(window, center=False, min_periods=1).mean()` (windows[c] > 0) and
 * `Series.expanding(min_periods=1).mean()` (windows[c] == 0); windows[c] < 0 copies column c.
 * Replaces the smoothing of reference plot.py:90-95, kinovea.py:99-105 and qualysis.py:113-117. */
int vbt_window_means(const double* rows, int T, int ncols, const int32_t* windows, double* out, int device);

/* ------------------------------------------------------------------ detector evaluation -----
 * Replaces the device-worthy part of the reference's eval.py: scaled_bbox / calculate_iou / match_bboxes for every image
 * (eval.py:57-71,74-93,96-153,182-205) and the curves scikit-learn computes for it (eval.py:232,245,360,370,515).
 * One handle holds ONE model's detection table on the device: rows (score float32, IoU float64, image number, detection index,
 * padded-matrix row) in the order eval.py:194-205 emits them for that model - images in the order they were added, inside an image
 * in idx_gt order, i.e. ground-truth rows first, then the dummy rows scipy's tie rule orders. */
typedef struct vbt_eval vbt_eval;
#define VBT_EVAL_MAX_GT 64          /* ground-truth boxes per image (the assignment solver's side) */
#define VBT_EVAL_NO_POSITIVES 1     /* no row with IoU > iou_threshold: recall, tpr, AP and AUC are NaN */
#define VBT_EVAL_NO_NEGATIVES 2     /* no row with IoU <= iou_threshold: fpr and AUC are NaN */
typedef struct {
  int32_t n_rows, n_pos, n_neg;   /* rows of the table, rows labelled True / False */
  int32_t n_pr;                   /* points of the PR curve (distinct scores + 1); it has n_pr - 1 thresholds */
  int32_t n_roc;                  /* points of the ROC curve after drop_intermediate, the leading (0, 0) included */
  int32_t flags;                  /* VBT_EVAL_NO_* */
  double ap, auc;                 /* average_precision_score, roc_auc_score (eval.py:245,370) */
} vbt_eval_summary;
/* max_batch: images per vbt_eval_add_detections call (1..4096); rows_cap: rows the table holds (25 per image is the most). */
int vbt_eval_create(int device, int max_batch, int rows_cap, vbt_eval** out);
void vbt_eval_destroy(vbt_eval* e);
/* an empty table again (synchronises the device) */
int vbt_eval_reset(vbt_eval* e);
/* The detections of B images as vbt_detect_async / vbt_pipeline_step_runs leave them on the device (boxes float32 [B,25,4]
 * normalised ymin,xmin,ymax,xmax, scores float32 [B,25], counts int32 [B]; every counted detection takes part: run_odt at
 * threshold 0, eval.py:176-180) matched against the images' ground truth and appended to the table: eval.py:182-205 for one model.
 * hw_host int32 [B][2] = the source image's (height, width) (eval.py:174,183-184); ground truth in CSR form: image b owns boxes
 * gt_offsets_host[b] .. gt_offsets_host[b+1]-1 of gt_boxes_host int32 [*][4] = ymin,xmin,ymax,xmax (create_bbox, eval.py:42-54).
 * Enqueue only, on `stream`: the host arrays are copied into pinned staging during the call and go up in ONE small copy per call
 * (four uploads may be in flight; a fifth call waits for the first).  Calls on one handle run in call order whatever their streams:
 * a call on another stream than the last one first makes its stream wait for the last call's kernels (the handle's scratch and table
 * are shared).  Box corners must be finite (numpy's astype(int) of a NaN / inf corner has no counterpart here).  VBT_ERR_CAPACITY, with nothing enqueued: B > max_batch, or an
 * image with more than VBT_EVAL_MAX_GT boxes (the message names it).  Rows beyond rows_cap are counted, not stored, and reported
 * as VBT_ERR_CAPACITY by vbt_eval_table / vbt_eval_curves. */
int vbt_eval_add_detections(vbt_eval* e, const float* boxes_dev, const float* scores_dev, const int32_t* counts_dev, int B,
                            const int32_t* hw_host, const int32_t* gt_offsets_host, const int32_t* gt_boxes_host, void* stream);
/* The table (the columns of the DataFrame of eval.py:207-211 plus the indices match_bboxes returns, eval.py:153): *n_rows always;
 * with any array non-NULL one copy per array, cap rows each (VBT_ERR_CAPACITY if cap < *n_rows).  gt_idx >= the image's number of
 * boxes marks a detection the assignment gave to a dummy row.  Synchronises the stream of the last vbt_eval_add_detections. */
int vbt_eval_table(vbt_eval* e, int* n_rows, float* scores, double* ious, int32_t* image, int32_t* det_idx, int32_t* gt_idx, int cap);
/* Label = IoU > iou_threshold (eval.py:515), then over the device table, without copying it:
 *   precision_recall_curve (eval.py:232): precision / recall [n_pr] ending in the (1, 0) point, pr_thresholds [n_pr - 1] increasing;
 *   average_precision_score (eval.py:245): ap = -sum(diff(recall) * precision[:-1]);
 *   roc_curve, drop_intermediate=True (eval.py:360): fpr / tpr / roc_thresholds [n_roc], the first point (0, 0) at threshold +inf;
 *   roc_auc_score (eval.py:370): auc by the trapezoid rule over those points.
 * Every point is bit-identical to scikit-learn's; ap / auc differ from it by the summation order only.  A rate whose denominator is
 * zero is NaN and `flags` says why (scikit-learn warns or raises there).  Scores must not be NaN.  Capacities in points;
 * VBT_ERR_CAPACITY when n_pr > pr_cap or n_roc > roc_cap: *s is filled, the arrays are not, and the call can be repeated.
 * Any array may be NULL.  Synchronises the stream of the last vbt_eval_add_detections. */
int vbt_eval_curves(vbt_eval* e, double iou_threshold, vbt_eval_summary* s, double* precision, double* recall, float* pr_thresholds,
                    int pr_cap, double* fpr, double* tpr, float* roc_thresholds, int roc_cap);
/* The same for a table held by the caller (host pointers, n rows: the Score and IoU columns of a DataFrame written earlier,
 * eval.py:510-512): upload, one launch, read-back.  No handle needed.  VBT_ERR_ARG: a NaN score. */
int vbt_eval_curves_from_table(const float* scores, const double* ious, int n, double iou_threshold, int device, vbt_eval_summary* s,
                               double* precision, double* recall, float* pr_thresholds, int pr_cap, double* fpr, double* tpr,
                               float* roc_thresholds, int roc_cap);

/* ------------------------------------------------------------------ COCO metrics -------------
 * The second set of numbers the reference reports its detectors by: the twelve COCO detection metrics that model.evaluate prints at
 * the end of every training log under models/ (train.py:64,70) - COCOeval's evaluateImg / accumulate / summarize for ONE category, no crowd and no
 * `difficult` boxes (class columns are ignored, as eval.py ignores them).
 * Box contract, all in double.  A detection (normalised float32 ymin,xmin,ymax,xmax, source size H x W): x = xmin W, y = ymin H,
 * w = xmax W - x, h = ymax H - y.  Ground truth (integer VOC corners): x = xmin, y = ymin, w = xmax - xmin, h = ymax - ymin.
 * area = w h in source-image pixels for both.  IoU is maskApi's bbIou on xywh: iw = min(dx+dw, gx+gw) - max(dx, gx), 0 if iw <= 0,
 * ih likewise, i = iw ih, IoU = i / (dw dh + gw gh - i).
 * Tables: IoU thresholds np.linspace(.5, .95, 10), recall thresholds np.linspace(0, 1, 101), area ranges [0,1e10], [0,32^2],
 * [32^2,96^2], [96^2,1e10] (a box is ignored for a range when area < lo || area > hi), maxDets 1 / 10 / 100.
 * One handle holds ONE model's rows on the device: per detection its score, image number, rank inside its image (descending score,
 * stable) and two 40-bit masks `matched` and `ignored`, bit a * 10 + t for area range a and IoU threshold t; and the number of
 * non-ignored ground-truth boxes per range over all images added. */
typedef struct vbt_coco vbt_coco;
typedef struct {
  double stats[12];               /* AP, AP50, AP75, APs, APm, APl, ARmax1, ARmax10, ARmax100, ARs, ARm, ARl; -1: no entry */
  int32_t n_images, n_rows;       /* images added, rows of the table */
  int32_t n_gt[4];                /* non-ignored ground-truth boxes per area range */
} vbt_coco_summary;
/* max_batch: images per vbt_coco_add_detections call (1..4096); rows_cap: rows the table holds (25 per image is the most). */
int vbt_coco_create(int device, int max_batch, int rows_cap, vbt_coco** out);
void vbt_coco_destroy(vbt_coco* c);
/* an empty table and zero counts again (synchronises the device) */
int vbt_coco_reset(vbt_coco* c);
/* The arguments and rules of vbt_eval_add_detections: the detections of B images as the detector leaves them on the device, the
 * source sizes and the ground truth in CSR form from the host.  evaluateImg of every image for the four ranges and ten thresholds,
 * one wavefront per image; the detections need not be sorted.  An image with neither boxes nor detections contributes nothing; one
 * with boxes and no detection counts its boxes.  Enqueue only, one pinned upload per call, calls run in call order whatever their
 * streams.  VBT_ERR_CAPACITY, with nothing enqueued: B > max_batch, or an image with more than VBT_EVAL_MAX_GT boxes.  Rows beyond
 * rows_cap are counted, not stored, and reported as VBT_ERR_CAPACITY by vbt_coco_table / vbt_coco_accumulate. */
int vbt_coco_add_detections(vbt_coco* c, const float* boxes_dev, const float* scores_dev, const int32_t* counts_dev, int B,
                            const int32_t* hw_host, const int32_t* gt_offsets_host, const int32_t* gt_boxes_host, void* stream);
/* The rows, images in the order added: *n_rows always; with any array non-NULL one copy per array, cap rows each (VBT_ERR_CAPACITY if
 * cap < *n_rows).  Synchronises the stream of the last vbt_coco_add_detections. */
int vbt_coco_table(vbt_coco* c, int* n_rows, float* scores, int32_t* image, int32_t* rank, uint64_t* matched, uint64_t* ignored, int cap);
/* COCOeval.accumulate and summarize over the device table: one stable sort by descending score (-0.0 and +0.0 one score), then one
 * workgroup per (range, maxDets, threshold).  precision [10][101][4][3] and scores [10][101][4][3] (the score at each recall
 * threshold, as double) in [T][R][A][M] order, recall [10][4][3] in [T][A][M] order: COCOeval's arrays without the category axis,
 * -1 throughout a slice whose range has no non-ignored box.  Every entry equals numpy's bit for bit; a stat is the mean over the
 * entries > -1 of its slice, summed on the host in index order, or -1.  Any array may be NULL.  Synchronises the stream of the last
 * vbt_coco_add_detections. */
int vbt_coco_accumulate(vbt_coco* c, vbt_coco_summary* s, double* precision, double* recall, double* scores);

/* ------------------------------------------------------------------ tracking overlay --------
 * Replaces draw_bounding_box / draw_bar_path (reference track.py:28-62,201-224): the tracked plate's box, its tracking id and the bar
 * path of its last `trail` centres, drawn into frames that already sit in device memory, in place and in the frames' own pixel
 * format (VBT_PIX_*).  The renderer is a pure function of (frames, DataFrame rows, fps): it needs nothing but the rows
 * vbt_tracker_rows_all returns, so it runs right after tracking or later from a stored DataFrame.  One colour per handle: the result
 * does not depend on the drawing order, so the kernel scatters.
 *
 * Raster contract.  cv2 is not a dependency: its rasteriser and Hershey font are not pinned and are not the contract.  The geometry
 * is the reference's; the coverage rules are this library's, stated so that they can be evaluated per pixel.  Once the pixel
 * coordinates are formed every value is an integer and every product is exact (int64 holds them, see rule 2).
 *
 * Per row (id, time, x, y, dx, dy, norm_plate_height h, norm_plate_width w) and a frame of H x W pixels, in IEEE double without
 * contraction, each double clamped to +-2^20 before a truncating cast (time * fps to +-2^30 before llrint):
 *   frame = llrint(time * fps)          the 1-based frame_count of track.py:169
 *   cx = trunc(x * W), cy = trunc(y * H)                                        the np.int32 cast of track.py:213-214
 *   xmin = trunc((x - w/2) * W), xmax = trunc((x + w/2) * W), ymin = trunc((y - h/2) * H), ymax = trunc((y + h/2) * H)
 * The box is rebuilt from the row, not taken from the tracker's x1..y2: it can differ from track.py:36-39 by one pixel where a
 * rounding falls on an integer.
 * The trail of a row is the (cx, cy) of that row and of the up to trail - 1 rows of the same id before it in (id, time) order -
 * rows of all earlier frames, whether or not those frames are drawn (track.py:57-58,217-224).
 *
 * Pixel (px, py) of a frame is covered when for some row of that frame one of these holds (t = thickness, R = radius, s = label_scale):
 *   1. Box outline (box != 0).  a = t/2, b = (t+1)/2 (integer division): the pixel lies inside [xmin-a, xmax+a] x [ymin-a, ymax+a]
 *      and not inside [xmin+b, xmax-b] x [ymin+b, ymax-b]; an empty inner rectangle excludes nothing.  t = 2: columns xmin-1, xmin.
 *   2. Trail segment, for consecutive trail points P0, P1, each coordinate of both first clamped to [-32768, 32768] (a point that
 *      far outside the frame bends its segment; frames are at most 16384 a side).  d = P1 - P0, q = (px, py) - P0, L2 = d.d,
 *      u = q.d, c = q x d = qx dy - qy dx.  If 0 < u < L2: covered iff 4 c^2 <= t^2 L2.  Otherwise: covered iff 4 |p - P|^2 <= t^2
 *      for the nearer end point P (P0 if u <= 0, else P1); L2 = 0 is the end-point test alone.  With those clamps |2c| < 2^34 and
 *      t^2 L2 < 2^54: whoever evaluates this in int64 compares |2c| with 3037000499 = floor(sqrt(2^63 - 1)) before squaring it.
 *   3. Marker: (px - cx)^2 + (py - cy)^2 <= R^2 around the row's own centre (track.py:61-62, filled).
 *   4. Label (label != 0): the text "id" followed by the decimal id, no space, bottom-left at (xmin, yb), yb = ymin - 15 if
 *      ymin - 15 > 15 else ymin + 15 (track.py:45).  The score of track.py:46-47 is not in the row log and is left out.  Character
 *      k, bitmap column c (0..4, left to right = MSB to LSB of the 5 bits) and bitmap row r (0..6, top to bottom) cover the s x s
 *      block with left column xmin + 6 s k + s c and top row yb - 7 s + 1 + s r.  Glyphs, rows top to bottom:
 *        0: 01110 10001 10011 10101 11001 10001 01110    6: 00110 01000 10000 11110 10001 10001 01110
 *        1: 00100 01100 00100 00100 00100 00100 01110    7: 11111 00001 00010 00100 01000 01000 01000
 *        2: 01110 10001 00001 00010 00100 01000 11111    8: 01110 10001 10001 01110 10001 10001 01110
 *        3: 11111 00010 00100 00010 00001 10001 01110    9: 01110 10001 10001 01111 00001 00010 01100
 *        4: 00010 00110 01010 10010 11111 00010 00010    i: 00100 00000 01100 00100 00100 00100 01110
 *        5: 11111 10000 11110 00001 00001 10001 01110    d: 00001 00001 01101 10011 10001 10001 01111
 * Covered pixels outside the frame are dropped.  VBT_PIX_RGB24: a covered pixel gets (r, g, b).  YUV: its luma sample gets Y and the
 * chroma sample at (py >> 1, px >> 1) gets U, V - a chroma sample is written iff one of its four pixels is covered - with
 *   Y = ((66 r + 129 g + 25 b + 128) >> 8) + 16;  U = ((-38 r - 74 g + 112 b + 128) >> 8) + 128;  V = ((112 r - 94 g - 18 b + 128) >> 8) + 128
 * (>> arithmetic).  Every other byte is untouched; drawing twice gives the frame drawing once gives.
 * One difference from the reference: it skips the VideoWriter.write of frames on which the detector found nothing (track.py:180-181),
 * which makes its video jump in time; here the caller keeps every frame, and a frame without rows comes back as it went in.
 *
 * Rep panel (vbt_overlay_set_hud; the content of the reference's figure, plot.py:112-232, in the video): the rep count, ROM and ACV
 * of the last completed rep, a bar per recent rep and a scrolling phase timeline (the axvspan of plot.py:162-169), as a small panel
 * on every frame.  Two colours and exactly one writer per pixel: the rules above scatter one colour and never read a pixel; the
 * panel never reads a pixel either but is a gather - EVERY pixel of the panel rectangle is written, with fg (the handle's rgb) where
 * it is covered and with bg (vbt_overlay_hud_params.bg) where it is not.  The result does not depend on any order and is idempotent.
 * The panel is drawn after the rules above by the same vbt_overlay_draw on the same stream: where a box or a trail crosses the
 * panel, the panel wins.  All values are integers once formed.  s = scale, (X, Y) = the panel's origin; the panel is
 * [X, X + 52 s) x [Y, Y + 50 s).
 *
 * Per phase (time_start, time_end, y_start, y_end, rom, type; type 0 concentric, 1 eccentric, 2 hold), formed on the host when the
 * phases are set, in IEEE double without contraction, frame() being the frame number above (llrint(time * fps) after the clamp):
 *   fs = frame(time_start), fe = frame(time_end)
 *   rom_cm = centi(rom);  acv_cm = centi(rom / (time_end - time_start)), and 0 when time_end - time_start <= 0
 *   centi(v) = 0 if v is NaN or v <= 0, else llrint(min(v * 100.0, 9999.0))
 * This is the library's own rounding: it can differ from Python's f'{v:0.2f}' (plot.py:178,186) in the last digit, where v * 100.0
 * rounds across a tie that the decimal expansion of v does not reach.
 *
 * State of frame f: the concentric phases with fe <= f are "completed", in table order; n = their number, last = the latest of them.
 *
 * Text: three lines of 8 characters.  Character k (0..7) of line l (0..2), bitmap column c and row r (as in rule 4) cover the s x s
 * block with left column X + 2 s + 6 s k + s c and top row Y + 2 s + 9 s l + s r.  Line 0 is "REP" and the decimal of
 * min(n, 99999) right-aligned in 5; line 1 is "ROM" and field(rom_cm of last); line 2 is "ACV" and field(acv_cm of last).
 * field(v) is five spaces when n = 0, else v / 100, '.', and the two digits of v % 100, right-aligned in 5 (field(5) = " 0.05").
 * A space covers nothing.  Digits are those of rule 4; the other glyphs, rows top to bottom:
 *        R: 11110 10001 10001 11110 10100 10010 10001    A: 01110 10001 10001 11111 10001 10001 10001
 *        E: 11111 10000 10000 11110 10000 10000 11111    C: 01110 10001 10000 10000 10000 10001 01110
 *        P: 11110 10001 10001 11110 10000 10000 10000    V: 10001 10001 10001 10001 10001 01010 00100
 *        O: 01110 10001 10001 10001 10001 10001 01110    .: 00000 00000 00000 00000 00000 01100 01100
 *        M: 10001 11011 10101 10101 10001 10001 10001
 * Rep bars: eight slots.  Slot j (0..7) holds completed rep number max(n - 8, 0) + j (0-based) if that is < n, else it is empty.
 * A filled slot has height hb = clamp(acv_cm * 12 s / full_scale_cm, 1, 12 s) (the product in int64, integer division) and covers
 * columns [X + 2 s + 6 s j, X + 2 s + 6 s j + 5 s) and rows [Y + 41 s - hb, Y + 41 s).
 * Phase timeline: columns c in [0, 47 s) at X + 2 s + c.  Column c stands for frame fc = f - (47 s - 1 - c) * frame_step (int64;
 * frame_step is the draw call's).  The first phase of the table with fs < fc <= fe decides (only fc >= 1 can match): concentric -
 * the column covers rows [Y + 43 s, Y + 47 s); eccentric - rows [Y + 45 s, Y + 47 s); a hold, or no such phase - nothing.  The
 * timeline uses the whole table, completed or not: with vbt_overlay_set_hud the panel is rendered after the clip is analysed and
 * every frame shows the finished analysis; a panel that follows the live analysis ("Rep panel from the live analysis" below) shows
 * the table as it stood at its last update.
 * Colours.  VBT_PIX_RGB24: a covered panel pixel gets fg, every other panel pixel bg.  YUV: luma per pixel in the same way; the chroma
 * sample at (py >> 1, px >> 1) gets fg's U, V if any of its four pixels is covered, else bg's - both colours through the integers
 * above.  For the YUV formats X and Y are even (52 s and 50 s always are): every chroma sample of the panel lies wholly inside it.
 * Every byte outside the panel rectangle is left as the rules above left it.
 *
 * Following a device row log (vbt_overlay_follow).  The raster contract is the one above; follow mode changes only where the rows come
 * from and when they become known.  The handle consumes a row log: rows_dev, the 64-byte records in emission order in device memory,
 * and nrows_dev, a device int32 with the number of valid records, which the log's writer (the tracker) advances.  The overlay only
 * ever reads both.  vbt_overlay_follow_update consumes rows [cursor, min(*nrows_dev, rows_cap)) in log order.  For each row it forms
 * the integers above by the statements of the prepare kernel (frame = llrint(time * fps) included).  The trail of a row is that row
 * and the up to trail - 1 ACCEPTED rows of the same id before it IN THE LOG; for a log whose per-id times do not decrease that is
 * the (id, time) order of vbt_overlay_set_rows.
 * Equality.  Let L be a log prefix that vbt_overlay_set_rows accepts once sorted by (id, time), every frame number in 1..max_frame
 * and no frame with more than max_rows_per_frame rows, and f a frame number not above the largest one in L.  vbt_overlay_draw of
 * frame f in follow mode then writes exactly the bytes it writes in sorted mode with the rows of the WHOLE clip: rows of later
 * frames never reach frame f.  How the log was cut into updates does not matter: one update per frame, per batch or for the whole
 * log leave the same handle state.
 * Skipped rows.  A kernel cannot refuse a call: it skips the row and says so.  A row is skipped when vbt_overlay_set_rows would
 * refuse it on its own (a non-finite value, id < 0, w < 0 or h < 0: VBT_OVERLAY_FOLLOW_BAD_ROW), when its time is smaller than that
 * of the previous accepted row of its id (_ORDER), when its frame number is outside 1..max_frame (_FRAME_RANGE), or when its frame
 * already holds max_rows_per_frame accepted rows (_FRAME_FULL); the first of these that holds, in this order of tests: BAD_ROW,
 * FRAME_RANGE, ORDER, FRAME_FULL.  A skipped row is not drawn, joins no trail, and sets its bit in a device word that
 * vbt_overlay_follow_status reads; its vbt_overlay_geometry record has trail length 0 (and is all zero for a BAD_ROW).  The equality
 * above holds while the flags are 0.
 * Rewound log.  *nrows_dev < cursor: the clip was reset or recycled.  Nothing is consumed, VBT_OVERLAY_FOLLOW_REWOUND is set, and the
 * caller calls vbt_overlay_follow again.
 * Frames without an accepted row, and frames beyond the last consumed row, are not touched.  The rep panel does not depend on the
 * row source: vbt_overlay_set_hud works on a handle in follow mode as on any other.
 *
 * Rep panel from the live analysis (vbt_overlay_hud_follow).  A handle's panel can FOLLOW one clip of a tracker that has live
 * analysis enabled (vbt_tracker_live_enable): its table is then formed on the device, from the phase list the live analysis keeps
 * for the clip's leader, by one launch per update.  The raster contract is the one of "Rep panel" above; only the table's source
 * changes.
 * Equality.  After vbt_overlay_hud_follow_update(o, flush_view, stream), a vbt_overlay_draw writes exactly the bytes it would write
 * after vbt_tracker_live_poll(t, flush_view, ...) at the same point of the tracker's stream, followed by vbt_overlay_set_hud(o,
 * params, the phases6 of that clip, its n_phases, fps, ...).  No byte is copied to the host and no stream is synchronised.  The
 * table's integers come from the same statements as vbt_overlay_set_hud's (overlay_core.h: fs, fe, centi, ACV, the running
 * concentric count), in IEEE double without contraction.
 * Snapshot semantics.  The panel is a snapshot at update granularity: every frame of a draw sees the leader's phase list as it stood
 * at the last update, and the per-frame rules above (completed = fe <= f, the timeline's window) apply to that snapshot.  With one
 * frame per tracker launch and one update per launch the panel is exactly causal; with a batch of frames per launch the first
 * frames of the batch already show what the batch's last frame established.
 * Difference from a panel set after the analysis (track --hud): that one shows the finished analysis on every frame.  The live panel
 * shows what is known so far.  Phases can also DISAPPEAR again - the analysis drops phases below its threshold when the clip's
 * max_y_diff grows - and the leader can change, with which the whole table changes: the rep count of the live panel can go down.
 * Blank panel.  The panel of P = 0 ("REP    0", blank fields, no bar, no timeline) is shown when the clip has no leader (-1), when the
 * leader has no entry in the live tables, and when the clip or the leader's entry carries any VBT_LIVE_* bit - the cases in which
 * the poll reports no phases.
 * Refusals become flags.  A kernel cannot refuse a call.  What vbt_overlay_set_hud would refuse in the phases - a non-finite value,
 * a type outside {0, 1, 2}, time_end < time_start, times decreasing along the table, fe above 2^24; the same tests in the same
 * order - sets VBT_OVERLAY_HUD_FOLLOW_BAD_PHASE, and the panel is blank for that update.  VBT_OVERLAY_HUD_FOLLOW_FLAGGED: the
 * VBT_LIVE_* case above.  VBT_OVERLAY_HUD_FOLLOW_CAPACITY: more phases than the handle's table holds (the tracker's phase_cap when
 * the panel was bound); blank as well.  The bits are sticky: vbt_overlay_hud_follow_status returns every bit set by an update
 * since vbt_overlay_hud_follow, with the leader and the phase count of the last update.
 * Ordering.  (a) The live tables are changed in place by the tracker launch that follows (its live analysis compacts the lists),
 * unlike the row log, which only grows: an update must not overlap a later launch of that tracker.  (b) An update overwrites the
 * table the previous draw may still be reading.  For the bare vbt_overlay_hud_follow_update both are the caller's duty: `stream` is
 * ordered behind the tracker launch whose state is to be shown, the next launch of that tracker behind the update, and the update
 * behind every draw of the handle enqueued before it - all three hold when tracker, update and draw share one stream.
 * vbt_pipeline_overlay_draw orders both itself, with one event in each direction and no host wait: the update runs on the
 * pipeline's tracker stream behind the last tracker launch; the event every later tracker launch and `stream` wait for is recorded
 * behind it; and the update waits for an event recorded on `stream` behind the handle's previous draw. */
typedef struct vbt_overlay vbt_overlay;
typedef struct {
  int32_t trail;        /* bar path length in points, track.py:57-58 -> 120 */
  int32_t thickness;    /* box outline and bar path, track.py:42,60 -> 2 */
  int32_t radius;       /* marker, track.py:62 -> 10 */
  int32_t label_scale;  /* pixels per bitmap cell -> 3 (a 15 x 21 character) */
  uint8_t rgb[3];       /* COLORS[1] of track.py:23 -> white */
  uint8_t label;        /* 0: no label */
  uint8_t box;          /* 0: no box outline */
  uint8_t reserved[3];
} vbt_overlay_params;
void vbt_overlay_default_params(vbt_overlay_params* p);
/* params NULL = the defaults.  VBT_ERR_ARG, before any device call: an unknown pix_fmt, H or W < 1 or above 16384, odd H or W with a
 * YUV format, trail < 1 or > 65536, thickness < 0 or > 1024, radius < 0 or > 16384, label_scale < 1 or > 64. */
int vbt_overlay_create(int device, int H, int W, int pix_fmt, const vbt_overlay_params* params, vbt_overlay** out);
void vbt_overlay_destroy(vbt_overlay* o);
/* The rows to draw from: rows_host = n of the 64-byte records vbt_tracker_rows_all returns, sorted by (id, time) - the order the
 * exported DataFrame has (track.py:105); fps = the clip's (track.py:136); n = 0 is allowed.  Replaces the handle's previous rows.
 * VBT_ERR_ARG, checked first and before any device call: fps <= 0 or not finite, a row with a non-finite value, an id < 0 (the label
 * has no sign), w < 0 or h < 0, rows not sorted by (id, time); VBT_ERR_CAPACITY: a frame number above 2^24 (the frame index is dense).
 * Uploads the rows and the index from frame number to rows, runs the prepare kernel (per row: the integers above and its trail
 * length) on `stream` and synchronises it. */
int vbt_overlay_set_rows(vbt_overlay* o, const void* rows_host, int n, double fps, void* stream);
/* Draw into B frames, contiguous in device memory (H*W*3 bytes each, H*W*3/2 for the YUV formats), frame i being frame number
 * frame0 + i * frame_step (frame0, frame_step >= 1).  In place; enqueue only: one launch, workgroups spread over (frame, row of that
 * frame, primitive), each walking its primitive clipped to the frame - no pass over the frame, no pixel read.  Frames without rows
 * are not touched - but for the rep panel, if vbt_overlay_set_hud set one: one more launch over (tile of the panel, frame). */
int vbt_overlay_draw(vbt_overlay* o, uint8_t* frames_dev, int B, int frame0, int frame_step, void* stream);
typedef struct {
  int32_t x, y;           /* panel origin -> 16, 16 */
  int32_t scale;          /* pixels per cell -> 3 (a 156 x 150 panel) */
  int32_t full_scale_cm;  /* ACV of a full-height bar, cm/s -> 200 */
  uint8_t bg[3];          /* -> 0,0,0 */
  uint8_t reserved[5];
} vbt_overlay_hud_params;
void vbt_overlay_hud_default_params(vbt_overlay_hud_params* p);
/* The rep panel ("Rep panel" above) of ONE id: phases6_host = P records of 6 doubles as vbt_tracker_phases / vbt_analyze return them,
 * fps = the clip's.  Replaces the handle's previous panel; P = 0 with params is a panel that shows "REP    0" and blank fields on
 * every frame; params NULL with P = 0 switches the panel off (only the handle is looked at then).  From then on every
 * vbt_overlay_draw draws the panel into every frame of its batch - frames without rows and frames past the last row included - with
 * one more launch that walks the panel, never the frame; without a panel vbt_overlay_draw launches exactly what it did before.
 * VBT_ERR_ARG, checked in this order and before any device call: P < 0, P > 0 with a NULL pointer or params NULL with P > 0; fps <= 0
 * or not finite; a non-finite phase value; a type outside {0, 1, 2}; time_end < time_start; time_start or time_end decreasing along
 * the table; scale outside 1..64; full_scale_cm outside 1..100000; x < 0 or y < 0.  VBT_ERR_CAPACITY: P > 65536 or a frame number
 * above 2^24.  Then the handle (NULL: VBT_ERR_ARG), then the geometry, VBT_ERR_ARG: odd x or y with a YUV handle, a panel that does
 * not lie wholly inside the frame (x + 52 scale > W or y + 50 scale > H).  A refused call leaves the handle's panel as it was.
 * Builds the table of per-phase integers (fs, fe, rom_cm, acv_cm, type, concentric phases up to and including this one) on the host,
 * uploads it in one copy on `stream` and synchronises it. */
int vbt_overlay_set_hud(vbt_overlay* o, const vbt_overlay_hud_params* params, const double* phases6_host, int P, double fps, void* stream);

/* A panel that follows the live analysis ("Rep panel from the live analysis" above) */
enum {
  VBT_OVERLAY_HUD_FOLLOW_FLAGGED = 1,    /* the clip or its leader carries a VBT_LIVE_* bit (or the leader has no entry) */
  VBT_OVERLAY_HUD_FOLLOW_BAD_PHASE = 2,  /* a phase vbt_overlay_set_hud would refuse */
  VBT_OVERLAY_HUD_FOLLOW_CAPACITY = 4    /* more phases than the handle's table holds */
};
/* Bind the handle's panel to clip `clip` of tracker `t`: replaces a panel set by vbt_overlay_set_hud, and vbt_overlay_set_hud
 * replaces a following one (params NULL with P = 0 switches either off).  `t` is borrowed and must outlive the handle's use of it.
 * The handle allocates its own table (phase_cap records of 24 bytes, the phase count, leader and flags) and its own flush-view
 * scratch (phase_cap x 6 doubles; not the poll's).  Synchronous (allocation + clears); the panel is blank until the first update.
 * Checked in this order and before any device call.  VBT_ERR_ARG: params NULL; fps <= 0 or not finite; scale outside 1..64;
 * full_scale_cm outside 1..100000; x < 0 or y < 0; the handle NULL; t NULL; clip outside the tracker's clips; odd x or y with a YUV
 * handle; a panel that does not lie wholly inside the frame.  VBT_ERR_STATE: live analysis is not enabled on t.  VBT_ERR_ARG: the
 * tracker is on another device than the handle.  A refused call leaves the handle's panel as it was. */
int vbt_overlay_hud_follow(vbt_overlay* o, const vbt_overlay_hud_params* params, vbt_tracker* t, int clip, double fps);
/* Form the table from the live analysis as it stands: ONE launch of one wavefront on `stream`, enqueue only (see "Ordering").
 * flush_view != 0: the phases as if the clip ended now, as the poll's flush view.  VBT_ERR_STATE: the panel follows nothing. */
int vbt_overlay_hud_follow_update(vbt_overlay* o, int flush_view, void* stream);
/* Leader and phase count of the last update and the VBT_OVERLAY_HUD_FOLLOW_* bits so far; one 16-byte copy on `stream`, which it
 * synchronises */
int vbt_overlay_hud_follow_status(vbt_overlay* o, int64_t* leader, int32_t* n_phases, int32_t* flags, void* stream);
/* The flush_view vbt_pipeline_overlay_draw passes to the update it makes for this handle (default 0) */
int vbt_overlay_hud_follow_flush(vbt_overlay* o, int flush_view);

/* Follow mode ("Following a device row log" above) */
enum {
  VBT_OVERLAY_FOLLOW_BAD_ROW = 1,
  VBT_OVERLAY_FOLLOW_ORDER = 2,
  VBT_OVERLAY_FOLLOW_FRAME_RANGE = 4,
  VBT_OVERLAY_FOLLOW_FRAME_FULL = 8,
  VBT_OVERLAY_FOLLOW_REWOUND = 16
};
/* Switch the handle to follow mode: it replaces the handle's rows, and vbt_overlay_set_rows switches back.  rows_dev / nrows_dev are
 * borrowed (vbt_tracker_rows_dev gives a clip's) and must outlive the handle's use of them.  Allocates, for rows_cap rows and frames
 * 1..max_frame: 48 bytes per row (geometry, links), 8 per frame (the frame index) and 16 per slot of the id table (the power of two
 * >= 2 rows_cap).  Synchronous (allocation + clears).  VBT_ERR_ARG, before any device call: a NULL pointer, rows_cap < 1, max_frame
 * outside 1..2^24, max_rows_per_frame outside 1..64, fps <= 0 or not finite. */
int vbt_overlay_follow(vbt_overlay* o, const void* rows_dev, const int32_t* nrows_dev, int rows_cap, int max_frame, int max_rows_per_frame,
                       double fps);
/* Consume the rows appended since the last call: ONE launch that reads *nrows_dev itself, enqueue only, on `stream` - which must be
 * ordered behind the launch that wrote the rows.  VBT_ERR_STATE: the handle is not in follow mode. */
int vbt_overlay_follow_update(vbt_overlay* o, void* stream);
/* Rows consumed so far and the VBT_OVERLAY_FOLLOW_* flags; one 8-byte copy on `stream`, which it synchronises */
int vbt_overlay_follow_status(vbt_overlay* o, int32_t* rows_consumed, int32_t* flags, void* stream);
/* In follow mode vbt_overlay_draw draws from the rows consumed so far, with a grid of (max_rows_per_frame x primitives, B): the host
 * knows no per-frame counts and never asks for them; the workgroups of absent rows leave at once. */
/* The pipeline's side of a one-pass export, for an overlay that follows one of the pipeline's clips: enqueue the tracker steps still
 * held back (vbt_pipeline_drain), make `stream` wait for the most recent tracker launch, then vbt_overlay_follow_update and
 * vbt_overlay_draw on `stream`.  Enqueue only.  The frames may be the ones the steps were given (drawn in place): the tracker launch
 * waited for depends on their forward, whichever stream the tracker runs on.
 * A handle whose panel follows this pipeline's tracker (vbt_overlay_hud_follow) also gets its vbt_overlay_hud_follow_update, with
 * the handle's vbt_overlay_hud_follow_flush setting, between the tracker launch and the draw ("Ordering" above: on the tracker
 * stream, events both ways, no host wait).  For every other handle the call enqueues exactly what it did without that. */
int vbt_pipeline_overlay_draw(vbt_pipeline* p, vbt_overlay* o, uint8_t* frames_dev, int B, int frame0, int frame_step, void* stream);

/* ------------------------------------------------------------------ Rep figure ----------
 * The reference's figure (plot.py:87-232) without a plotting library: bar position and velocity of ONE id over time, a tinted span
 * per phase, ROM and ACV written over every concentric phase.  A figure is a frame: a handle renders N figures of one size - N
 * tracks, each given as rows and phases - into N contiguous RGB24 frames in device memory, which vbt_mjpeg_encode can take on the
 * same stream.  As with the rep panel, cv2's and matplotlib's rasterisation is NOT the contract: the contract is the rules below,
 * stated a second time in numpy (tests/figure_ref.py).  All values are integers once formed; every double is IEEE, one operation
 * per statement, without contraction (the statements themselves: vbt_amd/csrc/figure_core.h).
 *
 * Input per figure.  T rows of 7 doubles (time, x, y, dx, dy, norm_plate_height, norm_plate_width: the columns of vbt_analyze), the
 * rows of one id sorted by time, and P phases of 6 doubles in the phases6 layout of vbt_overlay_set_hud.  The caller supplies the
 * phases (the VelocityTracker scan is not run here).
 * Series.  Four curves: pandas' rolling(5, min_periods=1) means of x, y (upper rectangle) and of dx, dy (lower rectangle), as
 * plot.py:90-92, computed on the device with the rolling mean of the rep analysis.
 *
 * Layout.  A white W x H frame, s = scale, holds two plot rectangles of PW x PH pixels, [X0, X0 + PW) x [Y0, Y0 + PH) above
 * [X0, X0 + PW) x [Y1, Y1 + PH).  Margins in cells of s pixels: 40 left, 4 right, 11 above the upper rectangle, 13 between the two,
 * 14 below the lower one:  X0 = 40 s, Y0 = 11 s, PW = W - 44 s, PH = (H - 38 s) / 2 (integer division), Y1 = Y0 + PH + 13 s.
 * vbt_figure_create refuses a size with PW < 16 or PH < 16.
 *
 * Axes.  t0, t1 = the first and last row time.  col(t) = t1 > t0 ? R((t - t0) / (t1 - t0) * (PW - 1)) : 0, where
 * R(v) = llrint(v) after v is clamped to [-32768, 32768] (a NaN, which only inf / inf can give, goes to -32768).
 * Position range, m and M the minimum and maximum over both smoothed position series: lo = max(m - 0.2, 0), hi = min(M + 0.2, 1);
 * if that gives hi <= lo, lo = m - 0.2 and hi = M + 0.2.  This is plot.py:145 WITHOUT the margin matplotlib's autoscale adds to
 * the data first.  Velocity range: pad = (M - m) * 0.05, and 0.5 when that is zero; lo = m - pad, hi = M + pad.
 * row(v) = R((hi - v) / (hi - lo) * (PH - 1)).  With T = 0 both ranges are [0, 1], the time axis is [0, 0], there are no curves
 * and everything else is drawn.  Rows and columns count from the rectangle's top left pixel.
 *
 * The figure is a list of RECORDS (vbt_figure_table returns them) and four curves.  A record is 12 int32:
 *   kind, x0, y0, x1, y1, ox, oy, chars[3], value, aux
 * [x0, x1] x [y0, y1] (inclusive, frame coordinates) is the part of the record that can be seen: its box [ox ..] x [oy ..] clipped to
 * the frame or, for spans and rep labels, to their rectangle; it is empty when x0 > x1 or y0 > y1, and the record is still listed.
 *   kind 0, span:   covers its visible box.  value = the phase's index, aux = its type.
 *   kind 1, line:   covers its visible box (frame lines, tick marks).
 *   kind 2, swatch: covers its visible box in the colour of curve aux (4 x, 5 y, 6 dx, 7 dy).
 *   kind 3, text:   aux = n | rot << 8; character k (0 .. n - 1) is byte k % 4 of chars[k / 4].  Not turned (rot = 0) the text's box
 *                   is (6 n - 1) s wide and 7 s high and bitmap column c, row r of character k cover the s x s block at
 *                   (ox + 6 s k + s c, oy + s r), as in the rep panel.  Turned a quarter (rot = 1, it reads bottom to top) the box is
 *                   7 s wide and (6 n - 1) s high and pixel (ox + a, oy + b) of it is pixel ((6 n - 1) s - 1 - b, a) of the text
 *                   not turned.  Only pixels inside the visible box are covered.
 * Character codes: 0..9 the digits, 12..21 R E P O M A C V . and space as in the rep panel (their glyphs are unchanged), and
 *   22 '-': 00000 00000 00000 11111 00000 00000 00000      25 'X': 10001 10001 01010 00100 01010 10001 10001
 *   23 '/': 00001 00001 00010 00100 01000 10000 10000      26 'Y': 10001 10001 01010 00100 00100 00100 00100
 *   24 'S': 01111 10000 10000 01110 00001 00001 11110      27 'D': 11110 10001 10001 10001 10001 10001 11110
 * The records, in table order:
 *   1. Spans.  For every phase i of type 0 (concentric) or 1 (eccentric), in phase order, two spans (upper, then lower rectangle) of
 *      columns X0 + col(time_start) .. X0 + col(time_end) over the rectangle's rows, clipped to the rectangle.  A hold draws nothing.
 *   2. Rep labels.  For every concentric phase, in phase order, two turned texts (upper: centi(rom); lower: centi(acv),
 *      acv = duration > 0 ? rom / duration : 0; centi as in the rep panel, so values above 99.99 show 99.99), "d.dd" or "dd.dd",
 *      at ox = X0 + col((time_start + time_end) / 2) - 3 s, oy = Y + 2 s (Y = Y0 or Y1), clipped to the rectangle; value = the centi.
 *   3. Per rectangle (upper first): four frame lines s wide AROUND the rectangle (top [X0 - s, X0 + PW + s) x [Y - s, Y), bottom the
 *      same at [Y + PH, Y + PH + s), left [X0 - s, X0) and right [X0 + PW, X0 + PW + s) over the rectangle's rows); the title at
 *      (X0, Y - 9 s): "ROM M" (position, ROM in m) / "ACV M/S" (velocity, ACV in m/s); two legend keys, at kx = X0 + 48 s and
 *      X0 + 70 s: a swatch [kx, kx + 6 s) x [Y - 7 s, Y - 4 s) and the text "X", "Y" / "DX", "DY" at (kx + 7 s, Y - 9 s); then
 *      the value ticks: step = the smallest of 10, 20, 50, 100, 200, 500, ... 10^7 thousandths with (hi - lo) * 1000 / step <= 6
 *      (no ticks if none, or if lo < -10^9 or hi > 10^9); for k from floor(lo * 1000 / step) - 1, ten values, those whose
 *      v = (k step) / 1000.0 (integer product, one divide) has lo <= v <= hi, each a line [X0 - 3 s, X0 - s) x [yt, yt + s),
 *      yt = Y + row(v) - s / 2, and a text of c = k step / 10 clamped to +-9999, "[-]d.dd" or "[-]dd.dd", right-aligned to end at
 *      X0 - 4 s (ox = X0 - 4 s - (6 n - 1) s), oy = Y + row(v) - 3 s; value = c.
 *   4. Time ticks under the lower rectangle (plot.py:208-215): u = the smallest power of ten with 256 u >= t1 - t0 (1 for every set
 *      shorter than 256 s), base = floor(t0) - floor(t0) mod 5 u (non-negative remainder); the seconds base + k u, k = 0 .. 263,
 *      that lie inside [t0, t1] (none if t0 < -10^9 or t1 > 10^9): a line [xt, xt + s) x [Y1 + PH + s, Y1 + PH + s + L),
 *      xt = X0 + col(second) - s / 2, L = 3 s for a multiple of 5 u (a major tick, aux = 1), else 2 s; a major tick is followed by
 *      its text: the integer, centred (ox = X0 + col - ((6 n - 1) s) / 2, oy = Y1 + PH + 5 s); value = the second.
 * Curves.  Point i of a figure is (col(time_i), row(v_i)) per series.  Consecutive points of a series are joined by rule 2 of the
 * tracking overlay with thickness t, in rectangle coordinates (segment i joins points i and i + 1; a one-point series is the
 * segment from the point to itself: a dot); a curve is clipped to its rectangle.
 *
 * One writer per pixel.  The value of every pixel is decided by the first of these that covers it: 1. a text record - ink;
 * 2. the second curve of the rectangle (y / dy); 3. the first curve (x / dx); 4. a line or a swatch (no two of different colour
 * meet); 5. a span - of those that cover it the one of the latest phase: concentric (247, 212, 212), eccentric (255, 229, 207),
 * the opaque colours alpha = 0.2 of matplotlib's C3 / C1 gives over white (plot.py:27-30,166-169); 6. white.  Ink is (0, 0, 0); the
 * curves are x (53, 25, 62), y (226, 75, 64), dx (112, 31, 87), dy (243, 118, 81) - four fixed colours in the spirit of the 'rocket'
 * palette, not seaborn's.  Nothing is read from the frames, rendering twice equals rendering once, every byte of the N frames is
 * written and no byte outside them.
 *
 * Staging.  A render workgroup owns a 256 x 32 pixel tile; it keeps the points its columns can meet and the records that touch it in
 * LDS when there are at most VBT_FIGURE_STAGE_POINTS / VBT_FIGURE_STAGE_RECORDS of them and reads global memory otherwise, by the
 * same statements. */
#define VBT_FIGURE_STAGE_POINTS 512
#define VBT_FIGURE_STAGE_RECORDS 96
typedef struct vbt_figure vbt_figure;
typedef struct {
  int32_t width, height;  /* -> 1280 x 800 */
  int32_t scale;          /* pixels per cell -> 2 */
  int32_t thickness;      /* of the curves -> 2 */
  int32_t max_figures;    /* -> 64 */
  int32_t max_rows;       /* per figure -> 16384 */
  int32_t max_phases;     /* per figure -> 512 */
  int32_t reserved;
} vbt_figure_params;
void vbt_figure_default_params(vbt_figure_params* p);
/* params NULL = the defaults.  VBT_ERR_ARG, before any device call: out NULL, width or height outside 1..16384, scale or thickness
 * outside 1..64, max_figures outside 1..4096, max_rows outside 1..2^20, max_phases outside 0..65536, max_figures * max_rows above
 * 2^26 or max_figures * max_phases above 2^22, a plot rectangle below 16 x 16.  One allocation: per figure 108 bytes per row and
 * 48 bytes per record (384 + 4 max_phases records); VBT_ERR_HIP, naming the size, when the device cannot give it. */
int vbt_figure_create(int device, const vbt_figure_params* params, vbt_figure** out);
void vbt_figure_destroy(vbt_figure* f);
/* The n figures to render: rows7_host = the rows of figure 0, 1, ... one after the other (row_counts[i] of 7 doubles each),
 * phases6_host likewise (phase_counts[i] of 6 doubles).  Replaces what the handle held; n = 0 leaves it with nothing set.
 * Refusals, on the host and before any launch, in this order: VBT_ERR_ARG n < 0 or NULL counts; VBT_ERR_CAPACITY n > 4096;
 * per figure VBT_ERR_ARG a negative count, VBT_ERR_CAPACITY more than 2^20 rows or 65536 phases; VBT_ERR_ARG, naming the figure and
 * the row or phase: a non-finite value, a time that decreases, a phase vbt_overlay_set_hud would refuse on its doubles.  Then the
 * handle (NULL: VBT_ERR_ARG) and VBT_ERR_CAPACITY: more figures, rows or phases than it was created for.  A refused call leaves the
 * handle as it was.  ONE upload (counts, rows and phases of all figures, concatenated) and ONE prepare launch, a workgroup per
 * figure, on `stream`, which it synchronises (the upload buffer is the call's own). */
int vbt_figure_set(vbt_figure* f, int n, const double* rows7_host, const int32_t* row_counts, const double* phases6_host,
                   const int32_t* phase_counts, void* stream);
/* Figures fig0 .. fig0 + n - 1 into n contiguous frames of W * H * 3 bytes at frames_dev.  Enqueue only: ONE launch, grid (tile,
 * figure); it needs no synchronisation behind a vbt_figure_set on the same stream, and vbt_mjpeg_encode can follow on it.  With
 * W % 4 == 0 and frames_dev 4-aligned four pixels go out as three 32-bit stores, else as bytes.  VBT_ERR_STATE: nothing is set;
 * VBT_ERR_ARG: a NULL argument, fig0 < 0, n < 0 or fig0 + n above the figures set.  The handle's tables must not be replaced (by
 * vbt_figure_set on another stream) while a render is in flight. */
int vbt_figure_render(vbt_figure* f, uint8_t* frames_dev, int fig0, int n, void* stream);
/* What the prepare launch formed for figure `fig`, read back (it waits for the stream of the last set or render): head6 = t0, t1,
 * position lo, hi, velocity lo, hi; points = T records of 5 int32 (column, then the pixel row of x, y, dx, dy); records = the
 * 12-int32 records above.  head6, *n_points and *n_records are always set; VBT_ERR_CAPACITY when cap_points or cap_records (in records)
 * is below them: no point and no record is copied.  VBT_ERR_STATE: nothing is set; VBT_ERR_ARG: fig outside the figures set. */
int vbt_figure_table(vbt_figure* f, int fig, double* head6, int32_t* points, int cap_points, int* n_points, int32_t* records, int cap_records,
                     int* n_records);

/* ------------------------------------------------------------------ Curve figure --------
 * The reference's second figure kind (eval.py:218-468): precision-recall and ROC curves of up to max_series models in one plot
 * rectangle, with a legend, a grid and, on the per-model figures, score-threshold annotations.  A handle renders N figures of one
 * size into N contiguous RGB24 frames in device memory, which vbt_mjpeg_encode can take on the same stream.  As with the rep figure,
 * matplotlib's rasterisation is NOT the contract: the contract is the rules below, stated a second time in numpy
 * (tests/curve_figure_ref.py).  All values are integers once formed; every double is IEEE, one operation per statement, without
 * contraction (the statements themselves: vbt_amd/csrc/curve_figure_core.h).  s = scale, t = thickness, b = (s + 1) / 2.
 *
 * Input per figure: a vbt_curve_figure_desc, n_series vbt_curve_series (a legend text, a colour 0..9 and n_points points of two
 * doubles x, y) and n_marks vbt_curve_mark (a series of the figure, a point of it by its index in the input, a text).
 *
 * Layout.  A white W x H frame holds ONE plot rectangle [X0, X0 + PW) x [Y0, Y0 + PH); margins in cells of s pixels: 30 left,
 * 4 right, 4 above, 22 below:  X0 = 30 s, Y0 = 4 s, PW = W - 34 s, PH = H - 26 s.  PW < 16 or PH < 16 is refused.
 *
 * Axes.  Both are fixed to [0, 1.01] (eval.py:254-255): col(x) = R(x / 1.01 * (PW - 1)), row(y) = R((1.01 - y) / 1.01 * (PH - 1)),
 * R the clamp-then-llrint of the rep figure; columns and rows count from the rectangle's top left pixel.
 *
 * Points.  A point is FINITE when both coordinates are.  x over the finite points of a series must not decrease, or must not
 * increase (roc_curve gives the first, precision_recall_curve the second); a series that decreases somewhere is taken in reversed
 * order, so it renders byte-identically to the same points given reversed.  Every finite point is a dot (rule 2 of the tracking
 * overlay on the segment from the point to itself) and two consecutive finite points are joined by rule 2, the exact capsule test,
 * with thickness t, in rectangle coordinates.  A non-finite point draws nothing and breaks the polyline.  n_points = 0 draws no
 * curve and still has its legend row.  Curves are clipped to the plot rectangle; where series overlap the later one wins.
 *
 * The run merge.  What vbt_curve_figure_table returns, and what the render kernel walks, are the MERGED points of a series: three
 * int32 each - column, row, join (1: a segment joins it to the merged point before it).  A RUN is a maximal stretch of consecutive
 * finite points of one column; of a run the first point, the last, the first of its lowest rows and the first of its highest rows
 * are kept, in input order (of the reversed series, if it is reversed).  The pixels do not change: the segments of a run lie on one
 * vertical line and form a connected path, so the union of their capsules is the capsule of [lowest, highest], which the kept
 * points still span, and the joins to the neighbouring columns need only the first and the last point.  The numpy statement renders
 * the UNMERGED polyline and the frames must match it byte for byte.
 *
 * Records (vbt_curve_figure_table returns them).  28 int32:  kind, x0, y0, x1, y1, ox, oy, value, aux, n, 0, 0, chars[16].
 * [x0, x1] x [y0, y1] (inclusive, frame coordinates) is the part of the record that can be seen: its box [ox ..] x [oy ..] clipped to
 * the frame or, for grid lines, to the plot rectangle; it is empty when x0 > x1 or y0 > y1, and the record is still listed.  The kind
 * is also the record's PRIORITY (below).
 *   kind 0 legend text, 3 mark text, 8 text: n bytes, byte k is byte k % 4 of chars[k / 4]; aux = rot.  Not turned the box is
 *        (6 n - 1) s wide and 7 s high and bitmap column c, row r of byte k cover the s x s block at (ox + 6 s k + s c, oy + s r);
 *        turned a quarter (rot = 1, reads bottom to top) the box is 7 s wide and (6 n - 1) s high and pixel (ox + a, oy + b') of it is
 *        pixel ((6 n - 1) s - 1 - b', a) of the text not turned.  Ink.
 *   kind 1 swatch: covers its visible box in the colour of palette index aux; value = the series.
 *   kind 2 legend box: value = its width BW, aux = its height BH.  A pixel within b of an edge of [ox, ox + BW) x [oy, oy + BH) is
 *        border grey (128, 128, 128), every other one white: the box is opaque.
 *   kind 4 marker: the disc (px - value)^2 + (py - aux)^2 <= (2 s)^2 around the marked point (value, aux); ox = value - 2 s.  Ink.
 *   kind 5 leader: rule 2 with thickness 1 on the segment from (ox, oy) to (value, aux), frame coordinates; the visible box is the
 *        segment's bounding box widened by 1.  Ink.  (The reference's arc is not reproduced.)
 *   kind 7 line: covers its visible box (spines, ticks).  Ink.  value = the tick's thousandths, aux = 1 on the y axis.
 *   kind 9 major grid line, kind 10 minor grid line: aux = 0 vertical, 1 horizontal; value = thousandths.  A major line covers its
 *        visible box, (176, 176, 176).  A minor line is DOTTED: with a = py - oy on a vertical and px - ox on a horizontal line,
 *        the pixels with (a / b) % 3 == 0 are covered, (204, 204, 204).  Both are opaque, not blended.
 * The records, in table order:
 *   1. The left spine [X0 - s, X0) x [Y0, Y0 + PH + s) and the bottom spine [X0, X0 + PW) x [Y0 + PH, Y0 + PH + s); no others
 *      (eval.py:256-257).
 *   2. Major ticks at v = 200 k / 1000.0, k = 0 .. 5, the x axis first.  x axis, x = X0 + col(v): the tick [x - s / 2, x - s / 2 + s)
 *      x [Y0 + PH + s, Y0 + PH + 4 s), the label "0.0" .. "1.0" at (x - (17 s) / 2, Y0 + PH + 5 s), the grid line [x, x + b) over the
 *      rectangle's rows.  y axis, y = Y0 + row(v): the tick [X0 - 4 s, X0 - s) x [y - s / 2, y - s / 2 + s), the label at
 *      (X0 - 22 s, y - 3 s), the grid line [y, y + b) over the rectangle's columns.
 *   3. Minor grid lines, x axis first: for every multiple m of the axis' step (minor_x, minor_y; 0 = none) with m <= 1000 that is no
 *      multiple of 200, a grid line as in 2 at v = m / 1000.0.
 *   4. The x title, centred under the labels at (X0 + (PW - (6 n - 1) s) / 2, Y0 + PH + 14 s), and the y title, turned, at
 *      (s, Y0 + (PH - (6 n - 1) s) / 2); an empty title has no record.
 *   5. The legend, when the figure has series: L = the longest legend text in bytes, BW = (L ? (6 L - 1) s : 0) + 16 s,
 *      BH = 9 s n_series + 4 s; the box at bx = X0 + 3 s (lower left, eval.py:264) or X0 + PW - 3 s - BW (lower right, eval.py:391),
 *      by = Y0 + PH - 3 s - BH, clipped to the frame; then per series k, ty = by + 3 s + 9 s k: the swatch
 *      [bx + 3 s, bx + 11 s) x [ty + 2 s, ty + 5 s) and the text at (bx + 13 s, ty).
 *   6. Per mark i of M (eval.py:313-334,443-464), (px, py) = (X0 + col, Y0 + row) of its point: the text, the marker, the leader.
 *      Lower-left figures (PR): the text's top RIGHT pixel is the corner (px - 8 s, py + (min(i, 3) + 1) 10 s); lower-right figures
 *      (ROC): its top LEFT pixel is the corner (px + (M - i) 6 s, py + (i + 1) 10 s).  The leader runs from the corner to (px, py).
 *      A mark on a non-finite point has its three records with an empty visible box.
 * Font.  The 5 x 7 cell of the rep panel for every byte 0x20..0x7E (vbt_amd/csrc/curve_font.h), rows top to bottom.  The characters
 * the overlay, the rep panel and the rep figure already draw (digits, R E P O M A C V S X Y D . - / space, i, d) have exactly their
 * bits; those tables and their codes 0..27 are untouched.
 *   ' ' 00000 00000 00000 00000 00000 00000 00000   '!' 00100 00100 00100 00100 00100 00000 00100   '"' 01010 01010 01010 00000 00000 00000 00000
 *   '#' 01010 01010 11111 01010 11111 01010 01010   '$' 00100 01111 10100 01110 00101 11110 00100   '%' 11000 11001 00010 00100 01000 10011 00011
 *   '&' 01100 10010 10100 01000 10101 10010 01101   ''' 00100 00100 01000 00000 00000 00000 00000   '(' 00010 00100 01000 01000 01000 00100 00010
 *   ')' 01000 00100 00010 00010 00010 00100 01000   '*' 00000 00100 10101 01110 10101 00100 00000   '+' 00000 00100 00100 11111 00100 00100 00000
 *   ',' 00000 00000 00000 00000 01100 00100 01000   '-' 00000 00000 00000 11111 00000 00000 00000   '.' 00000 00000 00000 00000 00000 01100 01100
 *   '/' 00001 00001 00010 00100 01000 10000 10000   '0' 01110 10001 10011 10101 11001 10001 01110   '1' 00100 01100 00100 00100 00100 00100 01110
 *   '2' 01110 10001 00001 00010 00100 01000 11111   '3' 11111 00010 00100 00010 00001 10001 01110   '4' 00010 00110 01010 10010 11111 00010 00010
 *   '5' 11111 10000 11110 00001 00001 10001 01110   '6' 00110 01000 10000 11110 10001 10001 01110   '7' 11111 00001 00010 00100 01000 01000 01000
 *   '8' 01110 10001 10001 01110 10001 10001 01110   '9' 01110 10001 10001 01111 00001 00010 01100   ':' 00000 01100 01100 00000 01100 01100 00000
 *   ';' 00000 01100 01100 00000 01100 00100 01000   '<' 00010 00100 01000 10000 01000 00100 00010   '=' 00000 00000 11111 00000 11111 00000 00000
 *   '>' 01000 00100 00010 00001 00010 00100 01000   '?' 01110 10001 00001 00010 00100 00000 00100   '@' 01110 10001 00001 01101 10101 10101 01110
 *   'A' 01110 10001 10001 11111 10001 10001 10001   'B' 11110 10001 10001 11110 10001 10001 11110   'C' 01110 10001 10000 10000 10000 10001 01110
 *   'D' 11110 10001 10001 10001 10001 10001 11110   'E' 11111 10000 10000 11110 10000 10000 11111   'F' 11111 10000 10000 11110 10000 10000 10000
 *   'G' 01110 10001 10000 10111 10001 10001 01111   'H' 10001 10001 10001 11111 10001 10001 10001   'I' 01110 00100 00100 00100 00100 00100 01110
 *   'J' 00111 00010 00010 00010 00010 10010 01100   'K' 10001 10010 10100 11000 10100 10010 10001   'L' 10000 10000 10000 10000 10000 10000 11111
 *   'M' 10001 11011 10101 10101 10001 10001 10001   'N' 10001 10001 11001 10101 10011 10001 10001   'O' 01110 10001 10001 10001 10001 10001 01110
 *   'P' 11110 10001 10001 11110 10000 10000 10000   'Q' 01110 10001 10001 10001 10101 10010 01101   'R' 11110 10001 10001 11110 10100 10010 10001
 *   'S' 01111 10000 10000 01110 00001 00001 11110   'T' 11111 00100 00100 00100 00100 00100 00100   'U' 10001 10001 10001 10001 10001 10001 01110
 *   'V' 10001 10001 10001 10001 10001 01010 00100   'W' 10001 10001 10001 10101 10101 10101 01010   'X' 10001 10001 01010 00100 01010 10001 10001
 *   'Y' 10001 10001 01010 00100 00100 00100 00100   'Z' 11111 00001 00010 00100 01000 10000 11111   '[' 01110 01000 01000 01000 01000 01000 01110
 *   '\' 10000 10000 01000 00100 00010 00001 00001   ']' 01110 00010 00010 00010 00010 00010 01110   '^' 00100 01010 10001 00000 00000 00000 00000
 *   '_' 00000 00000 00000 00000 00000 00000 11111   '`' 01000 00100 00010 00000 00000 00000 00000   'a' 00000 00000 01110 00001 01111 10001 01111
 *   'b' 10000 10000 10110 11001 10001 10001 11110   'c' 00000 00000 01110 10000 10000 10001 01110   'd' 00001 00001 01101 10011 10001 10001 01111
 *   'e' 00000 00000 01110 10001 11111 10000 01110   'f' 00110 01001 01000 11100 01000 01000 01000   'g' 00000 01111 10001 10001 01111 00001 01110
 *   'h' 10000 10000 10110 11001 10001 10001 10001   'i' 00100 00000 01100 00100 00100 00100 01110   'j' 00010 00000 00110 00010 00010 10010 01100
 *   'k' 10000 10000 10010 10100 11000 10100 10010   'l' 01100 00100 00100 00100 00100 00100 01110   'm' 00000 00000 11010 10101 10101 10001 10001
 *   'n' 00000 00000 10110 11001 10001 10001 10001   'o' 00000 00000 01110 10001 10001 10001 01110   'p' 00000 00000 11110 10001 11110 10000 10000
 *   'q' 00000 00000 01101 10011 01111 00001 00001   'r' 00000 00000 10110 11001 10000 10000 10000   's' 00000 00000 01110 10000 01110 00001 11110
 *   't' 01000 01000 11100 01000 01000 01001 00110   'u' 00000 00000 10001 10001 10001 10011 01101   'v' 00000 00000 10001 10001 10001 01010 00100
 *   'w' 00000 00000 10001 10001 10101 10101 01010   'x' 00000 00000 10001 01010 00100 01010 10001   'y' 00000 00000 10001 10001 01111 00001 01110
 *   'z' 00000 00000 11111 00010 00100 01000 11111   '{' 00010 00100 00100 01000 00100 00100 00010   '|' 00100 00100 00100 00100 00100 00100 00100
 *   '}' 01000 00100 00100 00010 00100 00100 01000   '~' 00000 00000 01000 10101 00010 00000 00000
 *
 * One writer per pixel.  The value of every pixel is decided by the first of these that covers it, a total order that is the same in
 * the kernel, in the shared core and in numpy: 0 legend text (ink); 1 legend swatch; 2 legend box (border or white); 3 mark text;
 * 4 marker; 5 leader; 6 the curves, from the last series to the first, in their palette colours; 7 spines and ticks; 8 tick and axis
 * text; 9 major grid; 10 minor grid; then white.  Palette 0..9: (31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40),
 * (148, 103, 189), (140, 86, 75), (227, 119, 194), (127, 127, 127), (188, 189, 34), (23, 190, 207).  Nothing is read from the frames,
 * rendering twice equals rendering once, every byte of the N frames is written and no byte outside them.
 *
 * Staging.  A render workgroup owns a 256 x 8 pixel tile; it keeps the merged points of all series its columns can meet and the
 * records that touch it in LDS when there are at most VBT_CURVE_FIGURE_STAGE_POINTS / VBT_CURVE_FIGURE_STAGE_RECORDS of them, and
 * reads both from global memory otherwise, by the same statements. */
#define VBT_CURVE_FIGURE_STAGE_POINTS 384
#define VBT_CURVE_FIGURE_STAGE_RECORDS 64
typedef struct vbt_curve_figure vbt_curve_figure;
typedef struct {
  int32_t width, height;  /* -> 1120 x 640 (the reference's 7 x 4 in) */
  int32_t scale;          /* pixels per cell -> 2 */
  int32_t thickness;      /* of the curves -> 2 */
  int32_t max_figures;    /* -> 16 */
  int32_t max_series;     /* per figure -> 8 */
  int32_t max_points;     /* per figure, all its series together -> 131072 */
  int32_t max_marks;      /* per figure -> 8 */
} vbt_curve_figure_params;
typedef struct {
  int32_t n_series, n_marks;
  int32_t legend_corner;  /* 0 lower left (PR), 1 lower right (ROC); it also chooses the side of the marks' texts */
  int32_t minor_x, minor_y; /* minor grid step in thousandths, 0 = none, else 20..1000 */
  int32_t reserved[3];
  char x_title[32], y_title[32]; /* NUL-terminated, at most 31 bytes */
} vbt_curve_figure_desc;
typedef struct {
  int32_t n_points;
  int32_t colour;         /* palette index 0..9 */
  char text[64];          /* the legend text, NUL-terminated, at most 63 bytes */
} vbt_curve_series;
typedef struct {
  int32_t series, point;  /* a series of the figure and a point of it, by its index in the input */
  char text[16];          /* NUL-terminated, at most 15 bytes */
} vbt_curve_mark;
void vbt_curve_figure_default_params(vbt_curve_figure_params* p);
/* params NULL = the defaults.  VBT_ERR_ARG, before any device call: out NULL, width or height outside 1..16384, scale or thickness
 * outside 1..64, max_figures outside 1..1024, max_series outside 1..16, max_points outside 1..2^22, max_marks outside 0..64,
 * max_figures * max_points above 2^26, a plot rectangle below 16 x 16.  One allocation: per figure 52 bytes per point and 112 bytes
 * per record (145 + 2 max_series + 3 max_marks records); VBT_ERR_HIP, naming the size, when the device cannot give it. */
int vbt_curve_figure_create(int device, const vbt_curve_figure_params* params, vbt_curve_figure** out);
void vbt_curve_figure_destroy(vbt_curve_figure* f);
/* The n figures to render: figs[n]; series = the series of figure 0, 1, ... one after the other; xy = their points in the same order,
 * two doubles each; marks likewise.  Replaces what the handle held; n = 0 leaves it with nothing set.  Refusals, on the host and
 * before any launch, in this order: VBT_ERR_ARG n < 0 or figs NULL; VBT_ERR_CAPACITY n > 1024; per figure VBT_ERR_ARG a negative
 * count, a corner that is not 0 or 1, a minor step that is neither 0 nor in 20..1000, VBT_ERR_CAPACITY more than 16 series or 64
 * marks; VBT_ERR_ARG NULL series, marks or xy where some are counted; then, naming the figure and the series or mark, VBT_ERR_ARG: a
 * negative n_points (VBT_ERR_CAPACITY above 2^22 per figure), a colour outside 0..9, a text or title without its NUL or with a byte
 * outside 0x20..0x7E, x that is not monotone (the point's index is named), a mark whose series or point does not exist.  Then the
 * handle (NULL: VBT_ERR_ARG) and VBT_ERR_CAPACITY: more figures, series, points or marks than it was created for.  A refused call
 * leaves the handle as it was.  ONE upload (everything, concatenated) and ONE prepare launch, a workgroup per figure, on `stream`,
 * which it synchronises (the upload buffer is the call's own). */
int vbt_curve_figure_set(vbt_curve_figure* f, int n, const vbt_curve_figure_desc* figs, const vbt_curve_series* series, const double* xy,
                         const vbt_curve_mark* marks, void* stream);
/* Figures fig0 .. fig0 + n - 1 into n contiguous frames of W * H * 3 bytes at frames_dev.  Enqueue only: ONE launch, grid (tile,
 * figure); vbt_mjpeg_encode can follow on the same stream.  With W % 4 == 0 and frames_dev 4-aligned four pixels go out as three
 * 32-bit stores, else as bytes.  VBT_ERR_STATE: nothing is set; VBT_ERR_ARG: a NULL argument, fig0 < 0, n < 0 or fig0 + n above the
 * figures set.  The handle's tables must not be replaced while a render is in flight. */
int vbt_curve_figure_render(vbt_curve_figure* f, uint8_t* frames_dev, int fig0, int n, void* stream);
/* What the prepare launch formed for figure `fig`, read back (it waits for the stream of the last set or render): counts[k] = the
 * merged points of series k; points = those of all series, one after the other, 3 int32 each; records = the 28-int32 records above.
 * *n_series, *n_points and *n_records are always set; VBT_ERR_CAPACITY when a capacity (in entries) is below them: nothing is copied.
 * VBT_ERR_STATE: nothing is set; VBT_ERR_ARG: fig outside the figures set. */
int vbt_curve_figure_table(vbt_curve_figure* f, int fig, int32_t* counts, int cap_series, int* n_series, int32_t* points, int cap_points,
                           int* n_points, int32_t* records, int cap_records, int* n_records);

/* ------------------------------------------------------------------ Validation figure --------
 * The accuracy study of the reference's kinovea.py:90-172 / qualysis.py:100-187 for N (ground truth, tracked rows) pairs in one
 * upload and one prepare launch: per pair the numbers validate.metric_trajectory + validate.compare give (vbt_amd/validate.py), and
 * the reference's figure of the pair - two stacked panels, X and Y over time, ground truth against tracker - rendered into an RGB24
 * frame that stays in device memory, where vbt_mjpeg_encode takes it.  The aligned trajectories never leave the device between the
 * comparison and the figure.  There is no display, no LaTeX table and no p-value (the reference drops them before it prints).  The
 * statements themselves: vbt_amd/csrc/validation_core.h; in numpy: tests/validation_ref.py.  Every double is IEEE, one operation
 * per statement, without contraction.
 *
 * Input per pair: ref [N][3] = time, x, y in metres; rows [T][5] = time, x, y, norm_plate_height, norm_plate_width of one track.
 * kind, per pair: 0 = kinovea, 1 = qualisys.
 *
 * Numbers.  (1) Window means of the rows exactly as vbt_window_means forms them: kinovea (copy, 5, 5, expanding, expanding),
 * qualisys (copy, copy, copy, 30, 30).  (2) x = sx * plate_diameter / sw, y = -sy * plate_diameter / sh.  (3) y += mean(ref y) -
 * mean(y), then x likewise.  (4) Every sum - the means, the MSE, the Pearson terms - is taken in ONE fixed order: 256 partial
 * sums, partial l = 0.0 + term(l) + term(l + 256) + ... in rising order, then a halving tree over the 256 (p[l] += p[l + h],
 * h = 128 .. 1).  It is not numpy's pairwise order: parity with numpy is to a tolerance.  (5) t_max = min(last times), t_min =
 * max(first times), n = (int)(t_max * rate).  (6) The grid as numpy.linspace: step = (t_max - t_min) / (n - 1), ts_i = i * step +
 * t_min, ts_{n-1} = t_max.  (7) Linear interpolation as scipy's interp1d: lower-bound search, hi clipped to 1..len-1, slope *
 * (ts - t_lo) + v_lo.  (8) mse = sum((a - b)^2) / n.  (9) Pearson r: centre, divide by sqrt(sum of squares), dot, clamp to
 * [-1, 1]; a constant series gives NaN and sets flag bit 0 (r_x) or 1 (r_y) of the pair.
 *
 * Figure.  s = scale, t = thickness.  Margins in cells of s pixels: left 50, right 4, top 17, between the panels 6, bottom 23; the
 * panels share what height is left.  Time axis [0, max(last ref time, last tracked time)], minor ticks every second, major,
 * labelled ones every five (every 10^k seconds from 128 ticks on).  Value axes per panel: m, M over both series, d = M - m,
 * e = 0.05 d (0.05 for d == 0), lo = m - e, hi = M + e; then with dX = hiX - loX, dY = hiY - loY: kinovea, if dX < dY the X panel
 * becomes [loX - dY/2, hiX + dY/2]; qualisys, if dX > dY the Y panel becomes [loY - dX/2, hiY + dX/2], else the X panel as for
 * kinovea.  Value ticks at the multiples of the rep figure's step, labelled d.dd.  Texts: `X [m]`, `Y [m]` turned at the left,
 * `Time [s]` below; the legend in a border at the top right, two entries side by side: `Kinovea` or `Qualisys`, `Velocity Tracker`.
 * Curves: four series (ref x, tracker x, ref y, tracker y), each with its own times, as MERGED points (column, row, join) by the
 * curve figure's run merge on this figure's mapping; the tracker's curve is drawn over the ground truth's.  Colours: ground truth
 * (53, 25, 62), tracker (243, 118, 81).  Records are the curve figure's 28 int32 with its kinds (0 legend text, 1 swatch, 2 legend
 * box, 7 lines, 8 text) and its rule: the smallest kind that covers a pixel decides it, the curves have place 6.  Nothing is read
 * from the frames, rendering twice equals rendering once, every byte of the N frames is written and no byte outside them.
 *
 * Staging.  A render workgroup owns a 256 x 8 pixel tile; it keeps the merged points of the four series its columns can meet and
 * the records that touch it in LDS when there are at most VBT_VALIDATION_STAGE_POINTS / VBT_VALIDATION_STAGE_RECORDS of them, and
 * reads both from global memory otherwise, by the same statements. */
#define VBT_VALIDATION_STAGE_POINTS 768
#define VBT_VALIDATION_STAGE_RECORDS 64
#define VBT_VALIDATION_KINOVEA 0
#define VBT_VALIDATION_QUALISYS 1
typedef struct vbt_validation vbt_validation;
typedef struct {
  int32_t width, height;  /* -> 1280 x 640 (the reference's 8 x 4 in) */
  int32_t scale;          /* pixels per cell -> 2 */
  int32_t thickness;      /* of the curves -> 2 */
  int32_t max_pairs;      /* -> 64 */
  int32_t max_rows;       /* tracked rows per pair -> 4096 */
  int32_t max_ref_rows;   /* ground truth rows per pair -> 4096 */
  int32_t max_grid;       /* grid points per pair -> 4096 */
  int32_t reserved;
} vbt_validation_params;
void vbt_validation_default_params(vbt_validation_params* p);
/* params NULL = the defaults.  VBT_ERR_ARG, before any device call: out NULL, width or height outside 1..16384, scale or thickness
 * outside 1..64, max_pairs outside 1..1024, max_rows, max_ref_rows or max_grid outside 2..2^20, max_pairs * (max_rows +
 * max_ref_rows + max_grid) above 2^26, a panel below 16 x 16 pixels.  One allocation, create-time only; VBT_ERR_HIP, naming the
 * size, when the device cannot give it. */
int vbt_validation_create(int device, const vbt_validation_params* params, vbt_validation** out);
void vbt_validation_destroy(vbt_validation* h);
/* The n pairs: kind[i] = the kind of pair i; ref = the ground truth rows of pair 0, 1, ... one after the other (ref_counts[i] rows of 3 doubles), rows = the
 * tracked rows likewise (row_counts[i] rows of 5 doubles).  Replaces what the handle held; n = 0 leaves it with nothing set.
 * Refusals, on the host and before any device call, in this order: VBT_ERR_ARG n < 0, a NULL pointer or (VBT_ERR_CAPACITY) n > 1024;
 * an unknown kind (the pair is named); plate_diameter or rate that is not finite and > 0; a negative count; then per pair, naming the pair and the row:
 * a value that is not finite, a plate size <= 0, fewer than 2 rows in either series, a time that does not rise strictly in either
 * series, no common span or n < 2.  Then the handle (NULL: VBT_ERR_ARG) and VBT_ERR_CAPACITY: more pairs, rows or grid points than
 * it was created for.  A refused call leaves the handle as it was.  ONE upload and ONE prepare launch, a workgroup per pair, on
 * `stream`, which it synchronises (the upload buffer is the call's own). */
int vbt_validation_set(vbt_validation* h, int n, const int32_t* kind, double plate_diameter, double rate, const double* ref, const int32_t* ref_counts,
                       const double* rows, const int32_t* row_counts, void* stream);
/* Per pair 8 doubles: mse_x, mse_y, r_x, r_y, n, t_min, t_max, flags; one copy (it waits for the stream of the last set or render).
 * cap in pairs.  VBT_ERR_STATE: nothing is set; VBT_ERR_CAPACITY: cap below the pairs set. */
int vbt_validation_stats(vbt_validation* h, double* out, int cap);
/* What the prepare launch formed for pair `pair`: head[6] = time lo, hi, X lo, hi, Y lo, hi; traj = the aligned trajectory, T rows
 * of time, x, y; grid = n rows of ts, ref x, tracker x, ref y, tracker y; counts[4] = the merged points of ref x, tracker x, ref y,
 * tracker y; points = those of all series one after the other, 3 int32 each; records = the 28-int32 records.  *n_rows, *n_grid,
 * *n_points, *n_records and counts are always set; VBT_ERR_CAPACITY when a capacity (in entries) is below them: nothing else is
 * copied.  VBT_ERR_STATE: nothing is set; VBT_ERR_ARG: pair outside the pairs set. */
int vbt_validation_table(vbt_validation* h, int pair, double* head, double* traj, int cap_rows, int* n_rows, double* grid, int cap_grid, int* n_grid,
                         int32_t* counts, int32_t* points, int cap_points, int* n_points, int32_t* records, int cap_records, int* n_records);
/* Figures pair0 .. pair0 + n - 1 into n contiguous frames of W * H * 3 bytes at frames_dev.  Enqueue only: ONE launch, grid (tile,
 * pair); vbt_mjpeg_encode can follow on the same stream.  With W % 4 == 0 and frames_dev 4-aligned four pixels go out as three
 * 32-bit stores, else as bytes.  VBT_ERR_STATE: nothing is set; VBT_ERR_ARG: a NULL argument, pair0 < 0, n < 0 or pair0 + n above
 * the pairs set. */
int vbt_validation_render(vbt_validation* h, uint8_t* frames_dev, int pair0, int n, void* stream);

/* ------------------------------------------------------------------ MJPEG export --------
 * A playable export of the drawn frames (the reference's VideoWriter, track.py:96-98,153-154,241-242): every frame of a batch that
 * sits in device memory is encoded there as one baseline JPEG and only the compressed bytes come back; the host wraps them in an AVI
 * (vbt_amd/mjpeg.py).  The bitstream is pinned to the integer, so an implementation in numpy (tests/mjpeg_ref.py) gives the same bytes.
 *
 * Frame = one complete JFIF file: SOI; APP0 "JFIF\0" 1.01, density unit 0, 1:1, no thumbnail; DQT table 0 (luma), DQT table 1
 * (chroma), each 8-bit, in zigzag order; SOF0 8-bit, H, W, 3 components: Y id 1 2x2 table 0, Cb id 2 1x1 table 1, Cr id 3 1x1 table 1
 * (4:2:0); DHT DC 0, AC 0, DC 1, AC 1; DRI; SOS (Y: DC 0 / AC 0, Cb and Cr: DC 1 / AC 1, Ss 0, Se 63, Ah/Al 0); the scan; EOI.
 * 629 bytes precede the scan.
 *
 * Size.  VBT_PIX_RGB24: any H, W in 1..16384; the YUV formats: even H and W.  An MCU is 16 x 16 pixels; partial MCUs are filled by
 * replicating the last column and row.  The code clamps the coordinates it loads from: for RGB24 that replicates the pixel before
 * the 2 x 2 chroma sum, for YUV it replicates the last sample of each plane - the same thing as replicating the converted samples.
 *
 * Colour (JFIF full range; >> arithmetic; results clipped to 0..255).
 *   RGB24: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16 per pixel; per 2 x 2 cell, from the channel sums S (0..1020):
 *     Cb = ((-11059 S_R - 21709 S_G + 32768 S_B + 2^17) >> 18) + 128;  Cr = ((32768 S_R - 27439 S_G - 5329 S_B + 2^17) >> 18) + 128.
 *   NV12 / I420 are BT.601 limited range (see VBT_PIX_NV12): luma becomes (Y - 16) 255 / 219, chroma (C - 128) 255 / 224 + 128, each
 *     the exact rational rounded to nearest, ties away from zero (the one tie: C = 128 +- 112).  Chroma samples are used at their own
 *     resolution; nothing is resampled.
 * Forward DCT of x = sample - 128, int32 throughout: T[k][n] = rint(2^13 s_k cos((2n+1) k pi / 16)) in double, s_0 = sqrt(1/8),
 *   s_k = 1/2;  rows A[y][u] = (sum_n x[y][n] T[u][n] + 2^10) >> 11;  columns F[v][u] = (sum_y A[y][u] T[v][y] + 2^14) >> 15.
 * Quantisation: base tables Annex K.1 / K.2; quality q in 1..100 by the IJG rule s = 5000 / q (integer) for q < 50, else 200 - 2 q,
 *   Q = clip((base s + 50) / 100, 1, 255);  level = sign(F) ((|F| + (Q >> 1)) / Q);  AC clamped to +-1023, DC to -1024..1023.
 * Entropy coding: the Annex K.3 tables, zigzag order, ZRL and EOB as in the standard.  The restart interval is one MCU row (DRI =
 *   ceil(W / 16)): DC predictors reset, the interval is padded with 1-bits to a byte, 0xFF bytes are followed by 0x00, and RSTm (m =
 *   interval index mod 8) follows every interval but the last.  Every MCU row is an independent byte-aligned unit: one workgroup each.
 *
 * Capacity.  Nothing is ever truncated: the scratch is sized for the proven worst case.  A block is at most 22 + 63 x 26 = 1660 bits
 * (longest DC code + 11 bits; longest AC code + 10 bits per coefficient; ZRL and EOB only replace coefficients by something shorter)
 * and stuffing at most doubles a byte, so an interval of n MCUs holds at most 2 ceil(6 n 1660 / 8) bytes.  With MW = ceil(W / 16) and
 * MH = ceil(H / 16) a handle allocates, per frame of max_batch,
 *     MW MH (768 + 2496) + 629 + MH (2496 MW + 2) bytes, about 5.8 KB per MCU
 * (int16 levels, the intervals' stuffed bytes at a worst-case stride, and the contiguous output): 47 MB per frame of 1920 x 1080, 6 GB
 * per frame of 16384 x 16384.  vbt_mjpeg_create fails with VBT_ERR_HIP, naming the size, when the device cannot give max_batch times
 * that; a caller of very large frames chooses max_batch accordingly.  Every store in the kernels is still checked against its buffer;
 * a miss sets an overflow word that lives behind the offset table at a fixed place, is cleared on the stream by every
 * vbt_mjpeg_encode and, if ever set, makes vbt_mjpeg_read return VBT_ERR_CAPACITY and drop that batch.  No torch, no library: HIP
 * kernels for gfx950 (vbt_amd/csrc/mjpeg.hip). */
typedef struct vbt_mjpeg vbt_mjpeg;
/* VBT_ERR_ARG, before any device call: out NULL, an unknown pix_fmt, H or W outside 1..16384, odd H or W with a YUV format, quality
 * outside 1..100, max_batch outside 1..1024. */
int vbt_mjpeg_create(int device, int H, int W, int pix_fmt, int quality, int max_batch, vbt_mjpeg** out);
void vbt_mjpeg_destroy(vbt_mjpeg* m);
/* Encode B frames, contiguous in device memory (the layout vbt_overlay_draw takes).  Enqueue only, on `stream`: behind a
 * vbt_overlay_draw on the same stream it needs no synchronisation in between.  The frames are read, not written.  VBT_ERR_CAPACITY:
 * B > max_batch; VBT_ERR_STATE: the previous batch has not been read; B = 0 is VBT_ERR_ARG.  Nothing is enqueued on an error. */
int vbt_mjpeg_encode(vbt_mjpeg* m, const uint8_t* frames_dev, int B, void* stream);
/* The batch's bytes: frame i is host_buf[offsets[i] .. offsets[i + 1]).  One synchronisation of `stream` (the one given to
 * vbt_mjpeg_encode), then two copies: the offset table (max_batch + 2 words, the overflow word last), then offsets[B] bytes.
 * VBT_ERR_CAPACITY when cap < offsets[B]: offsets is filled, nothing else is copied and the batch stays readable.  VBT_ERR_STATE:
 * no batch is pending.  A successful read releases the handle for the next vbt_mjpeg_encode. */
int vbt_mjpeg_read(vbt_mjpeg* m, uint8_t* host_buf, uint64_t cap, uint64_t* offsets, void* stream);

/* ------------------------------------------------------------------ Scaled export --------
 * The reference shows every annotated frame resized to --display_image_height, the width following the source's aspect ratio
 * (track.py:69,139-140,237-239).  There is no display here, so the display is the export: frames of H x W in, frames (or JPEGs) of
 * h x w out, on the device, between the overlay and the encoder or the copy back.
 *
 * Order.  The overlay and the panels are drawn at full resolution first, then the frame is resized (track.py:201-224 before :237).
 * Filter.  cv2.resize's default: bilinear with half-pixel centres, no anti-aliasing (below half size a sample skips source pixels,
 * as in the reference).  cv2's fixed-point rounding is not the contract; the contract is the integers below (the numpy statement of
 * it is tests/scale_ref.py), within 0.5 + 255 / 2048 of the bilinear filter in real numbers.
 *
 * Size.  vbt_display_size: h = display_height, w = (int)(h * ((double)W / (double)H)) - the reference's expression, in double,
 * truncated; for the YUV 4:2:0 formats w is then rounded down to even and an odd h is refused.  h and w must lie in 1..16384.  The
 * handles below take any (h, w), not only aspect-preserving ones.
 * Axis table, for destination index o of an axis with n_src source and n_dst destination samples, built on the host in double:
 *     f = max((o + 0.5) * (n_src / n_dst) - 0.5, 0);  i0 = min(floor(f), n_src - 1);  i1 = min(i0 + 1, n_src - 1);
 *     a = rint((f - i0) * 2048), which lies in 0..2048.
 * Sample, int32 throughout (the largest sum is 255 * 2^22 + 2^21 < 2^31):
 *     out = ((p[y0][x0] (2048 - ax) + p[y0][x1] ax) (2048 - ay) + (p[y1][x0] (2048 - ax) + p[y1][x1] ax) ay + 2^21) >> 22.
 * n_dst == n_src gives a = 0 everywhere: the output is a byte copy.
 * Planes.  VBT_PIX_RGB24: the three channels of a pixel share one table pair.  NV12 / I420: the luma plane uses the tables of
 * (H, W) -> (h, w), each chroma plane those of (H/2, W/2) -> (h/2, w/2); samples are scaled as stored (limited range), the output is
 * in the source's own pixel format, and NV12's interleaved U, V are two planes that share a table pair.
 * Not covered: anti-aliasing, letterboxing.  HIP kernels for gfx950 (vbt_amd/csrc/scale.hip, the SCALED transform of mjpeg.hip). */
typedef struct vbt_scaler vbt_scaler;
/* Host only, no device call.  VBT_ERR_ARG, the text naming the argument: h or w NULL, an unknown pix_fmt, H or W outside 1..16384 or
 * odd with a YUV format, display_height outside 1..16384 or odd with a YUV format, a resulting width outside 1..16384 (2.. for YUV). */
int vbt_display_size(int H, int W, int pix_fmt, int display_height, int* h, int* w);
/* VBT_ERR_ARG, before any device call: out NULL, an unknown pix_fmt, H, W, h or w outside 1..16384, an odd one with a YUV format.
 * Builds the tables (plane 0 y and x; for YUV plane 1 y and x) and uploads them in one copy: 8 bytes per entry. */
int vbt_scaler_create(int device, int H, int W, int h, int w, int pix_fmt, vbt_scaler** out);
void vbt_scaler_destroy(vbt_scaler* s);
/* B contiguous frames of H x W at src_dev -> B contiguous frames of h x w at dst_dev, both in the layout vbt_overlay_draw takes.
 * Enqueue only, one launch on `stream`; src is read, every byte of dst is written.  Stores are 32-bit words where a plane's rows
 * begin 4-aligned (dst_dev, the frame size, the plane's offset and its row bytes all multiples of 4), bytes otherwise.
 * VBT_ERR_ARG: a NULL argument, B < 1; VBT_ERR_CAPACITY: B > 65535.  Nothing is enqueued on an error. */
int vbt_scaler_run(vbt_scaler* s, const uint8_t* src_dev, uint8_t* dst_dev, int B, void* stream);
/* The handle's table of `plane` (0: luma or RGB, 1: chroma of a YUV handle) and `axis` (0: y, 1: x), read back from the device for
 * tests: i0[k] and a[k] of destination index k.  *n is always set; VBT_ERR_CAPACITY when cap < *n (nothing is copied);
 * VBT_ERR_ARG: a NULL argument, a plane or axis the handle does not have. */
int vbt_scaler_tables(vbt_scaler* s, int plane, int axis, int32_t* i0, int32_t* a, int cap, int* n);
/* A vbt_mjpeg that takes frames of H x W and emits JPEGs of h x w: vbt_mjpeg_encode, vbt_mjpeg_read and vbt_mjpeg_destroy work on
 * it unchanged, the scratch is sized by (h, w) and the JFIF header says h x w.  Defining property: the bytes are those
 * vbt_mjpeg_encode of a vbt_mjpeg_create(h, w) handle produces for the frames vbt_scaler_run produces.  The colour stage of the
 * transform kernel takes each pixel through the sample above; the scaled frame never exists in memory.  With (h, w) == (H, W) the
 * handle is exactly what vbt_mjpeg_create returns.  VBT_ERR_ARG as vbt_mjpeg_create, for either size. */
int vbt_mjpeg_create_scaled(int device, int H, int W, int h, int w, int pix_fmt, int quality, int max_batch, vbt_mjpeg** out);

/* ------------------------------------------------------------------ MJPEG import --------
 * The way in for video files (the reference's cv2.VideoCapture, track.py:129-160): the frames of a Motion-JPEG AVI - the files
 * the export above writes, and what many cameras and ffmpeg -c:v mjpeg write - are decoded on the device.  The host parses the
 * headers and uploads only the compressed bytes; the frames appear in device memory as RGB24 [B,H,W,3], the layout
 * vbt_pipeline_step_runs and vbt_overlay_draw take.  The reconstruction is pinned to the integer and is, bit for bit, what
 * libjpeg-turbo does by default (the decoder behind Pillow, OpenCV and most players); the numpy statement is tests/mjpeg_dec_ref.py.
 *
 * Accepted (one JPEG file per frame): SOF0 baseline, 8-bit, Huffman; 1 component (grey) or 3 components (JFIF YCbCr); luma
 * sampling 1x1, 2x1 or 2x2 with both chroma components 1x1 (4:4:4, 4:2:2, 4:2:0); one scan holding all components in frame order
 * with Ss = 0, Se = 63, Ah = Al = 0; 8-bit DQT with table ids 0..3, several tables per segment allowed, a later table replaces an
 * earlier one of its id; DHT ids 0..1 per class, several per segment, redefinition before SOS; NO DHT AT ALL = the Annex K.3 tables
 * (the MJPG-in-AVI convention); any DRI, none or 0 included (an interval of 0 MCUs, or of more MCUs than the frame has, is one
 * interval); APPn, COM and other segments with a length are skipped; 0xFF fill bytes before markers; 1..16384 pixels a side; a
 * missing EOI.  A DC size category up to 16 is decoded.
 * Refused, VBT_ERR_IO with a vbt_last_error() text that names the frame of the batch and the reason: SOF1, SOF2 and every other
 * SOFn (progressive, arithmetic, lossless, hierarchical); a precision other than 8 bits; a 16-bit DQT; any other sampling or
 * component count; more than one scan (a scan that does not hold all components, or a SOS / SOFn / DQT / DRI behind the scan); an
 * Adobe APP14 segment whose transform is not 1 (0 = RGB / CMYK, 2 = YCCK); a segment length that runs past the frame; a missing SOI,
 * SOS, SOF, a DQT or DHT the scan names; a DHT with more codes than a length holds or more than 256 symbols; a frame size other
 * than the handle's; a frame of 2 GiB or more.
 *
 * Entropy decoding (T.81 F.2.2): the scan runs from behind SOS to the first marker that is neither RSTm nor a stuffed FF 00.  It is
 * cut at its RSTm markers into restart intervals; interval k holds MCUs k ri .. min((k + 1) ri, MCUs) and starts with DC predictors
 * 0.  Its levels are stored as int16 in natural order.  Per-frame scan status (vbt_mjpeg_decode_status), the largest raised:
 *   0 fine;  1 an interval's bits ended before its MCUs did;  2 a bit pattern that no code of the table matches (or a DC size
 *   above 16);  3 a run that takes the coefficient index above 63;  4 the number of RSTm markers is not ceil(MCUs / ri) - 1 (the
 *   frame is then not walked at all);  5 a marker's m is not its index mod 8.
 * Codes 1..3 end their interval: the blocks it had not reached keep level 0 (mid-grey for a first block, since predictors restart
 * per interval).  A damaged scan spoils its own frame only; what such a frame shows is deterministic, but not part of the contract.
 * Two ways through an interval give these levels and this status, bit for bit (vbt_mjpeg_decoder_set_entropy):
 *   INTERVAL  one lane walks the interval.  Fast when a frame has many intervals (this project's export: one per MCU row), one lane
 *     per frame when it has no restart markers - what ffmpeg, cameras and Pillow write.
 *   SYNC  one workgroup per interval.  The interval is cut into subsequences of S raw bytes (subseq_bytes, a power of two); lane i
 *     owns the symbols that begin in its S bytes, 256 lanes (a chunk) at a time, the chunks in order.  A lane does not know the
 *     state (raw bit position, block slot in the MCU, zigzag index) at its first byte: it guesses "a block begins here", walks, and
 *     then takes its left neighbour's exit state as its entry, round after round, until no entry changes.  Lanes 0 .. r - 1 are final
 *     after round r, so a chunk takes at most 257 rounds - the loop's bound; real scans synchronise within a few symbols, and the
 *     rounds a batch needed are reported (vbt_mjpeg_decode_entropy_info).  Prefix sums over block counts and DC differences then give
 *     every lane its block number and predictors, and a second walk stores the levels.  A walk from a guess meets codes no table
 *     holds and indices above 63 all the time; it records them and goes on.  When a lane with a true entry recorded one before the
 *     interval's last block, or the bits end before the blocks do, nothing of that chunk is stored in parallel: ONE lane finishes the
 *     interval from the chunk's entry state with the statements of INTERVAL, so a damaged scan is decoded exactly as before.
 *   AUTO (the default) takes SYNC for a batch in which some frame has scan bytes / intervals >= auto_min_interval_bytes
 *     (vbt_mjpeg_decoder_get_entropy; measured, profiles/mjpeg_decode.md), INTERVAL otherwise.
 *
 * Reconstruction, int32 throughout (wrapping; >> arithmetic):
 *   Dequantise: c = level Q, natural order.
 *   IDCT ("islow", Loeffler-Ligtenberg-Moschytz, 13-bit constants).  One 8-point pass on x[0..7] with descale shift s:
 *     z1 = (x2 + x6) 4433;  t2 = z1 - x6 15137;  t3 = z1 + x2 6270;  t0 = (x0 + x4) << 13;  t1 = (x0 - x4) << 13;
 *     t10 = t0 + t3;  t13 = t0 - t3;  t11 = t1 + t2;  t12 = t1 - t2;
 *     a0 = x7, a1 = x5, a2 = x3, a3 = x1;  z1 = a0 + a3;  z2 = a1 + a2;  z3 = a0 + a2;  z4 = a1 + a3;  z5 = (z3 + z4) 9633;
 *     a0 *= 2446;  a1 *= 16819;  a2 *= 25172;  a3 *= 12299;  z1 *= -7373;  z2 *= -20995;  z3 = z3 (-16069) + z5;  z4 = z4 (-3196) + z5;
 *     a0 += z1 + z3;  a1 += z2 + z4;  a2 += z2 + z3;  a3 += z1 + z4;
 *     y0, y7 = t10 +- a3;  y1, y6 = t11 +- a2;  y2, y5 = t12 +- a1;  y3, y4 = t13 +- a0;  each (y + 2^(s-1)) >> s.
 *   Pass 1 runs down the columns of c with s = 11 (2 extra bits kept), pass 2 along the rows of the result with s = 18; the sample is
 *   clip(value + 128, 0, 255).  (A stream whose dequantised values or pass-1 results leave int16 is outside the bit-for-bit
 *   claim: SIMD builds of libjpeg-turbo keep those in 16 bits.)
 *   Upsampling ("fancy", triangle).  A chroma component holds dw = ceil(W / hs) by dh = ceil(H / vs) samples; the edge rules use dw
 *   and dh, never the padded MCU grid.  With in[i] a row of it and i = x >> 1:
 *     h2v1 (4:2:2): out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2; out[0] = in[0], out[2dw-1] = in[dw-1].
 *     h2v2 (4:2:0): the output row y takes row j = y >> 1 and its neighbour j - 1 (y even) or j + 1 (y odd), clamped to 0 .. dh - 1:
 *       s[i] = 3 in_j[i] + in_neighbour[i];  out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4;
 *       out[0] = (4 s[0] + 8) >> 4, out[2dw-1] = (4 s[dw-1] + 7) >> 4.
 *     dw <= 2 (W <= 4): no filter, every sample is replicated 2 x (and 2 x down for h2v2) - the IJG decoder's rule.
 *   Colour (JFIF full range), cb = Cb - 128, cr = Cr - 128:
 *     R = Y + ((91881 cr + 32768) >> 16);  G = Y + ((-22554 cb - 46802 cr + 32768) >> 16);  B = Y + ((116130 cb + 32768) >> 16),
 *     each clipped to 0..255.  Grey: R = G = B = Y.
 *
 * Capacity.  A handle is one frame size and up to max_batch frames.  vbt_mjpeg_decoder_create allocates, per frame of max_batch and
 * with NB = 3 (2 ceil(W / 16)) (2 ceil(H / 16)) blocks (the 4:4:4 worst case), 128 NB bytes of levels, 64 NB bytes of planar
 * components and 4 ceil(W / 8) ceil(H / 8) bytes of interval table (the worst case, one MCU per interval): 18.9 MB per frame of
 * 1920 x 1080, 2.4 GB per frame of 16384 x 16384.  It fails with VBT_ERR_HIP, naming the size, when the device cannot give that.
 * The compressed bytes of a batch (a 4.1 KB descriptor per frame and the entropy-coded segments) travel through two pinned staging
 * buffers, used in turn, and one device buffer; these start at H W / 4 bytes per frame and grow on demand up to 1 GiB per batch
 * (VBT_ERR_CAPACITY above that); a growing call allocates, and so waits for the device - every other call only enqueues.  One handle
 * serves one stream at a time.  No torch, no library: HIP kernels for gfx950 (vbt_amd/csrc/mjpeg_decode.hip); the parser and the
 * decoding statements are vbt_amd/csrc/jpeg_parse.h and jpeg_core.h. */
typedef struct vbt_mjpeg_decoder vbt_mjpeg_decoder;
/* Host only, no device call: the size, the component count (1 or 3) and the luma sampling as (hs << 4) | vs (0x11, 0x21, 0x22) of
 * one JPEG file the decoder accepts; any of the four pointers may be NULL.  VBT_ERR_IO with the reason otherwise. */
int vbt_jpeg_probe(const uint8_t* bytes, uint64_t n, int* H, int* W, int* components, int* sampling);
/* VBT_ERR_ARG, before any device call: out NULL, H or W outside 1..16384, max_batch outside 1..1024. */
int vbt_mjpeg_decoder_create(int device, int H, int W, int max_batch, vbt_mjpeg_decoder** out);
void vbt_mjpeg_decoder_destroy(vbt_mjpeg_decoder* d);
/* Decode B frames: frame i is host_bytes[offsets[i] .. offsets[i + 1]) (B + 1 offsets, ascending), a complete JPEG file; the frames
 * go to frames_dev_out, B x H x W x 3 bytes of device memory.  All B headers are parsed first: a refusal returns VBT_ERR_IO with
 * nothing enqueued and frames_dev_out untouched.  Then the descriptors and scans are packed into the staging buffer whose turn it
 * is - the host waits for the event behind that buffer's last copy; no stream wait is put in front of the copy - followed by one
 * H2D copy and the launches, all on `stream`.  host_bytes may be reused as soon as the call returns.  VBT_ERR_CAPACITY:
 * B > max_batch, or more than 1 GiB of compressed bytes; VBT_ERR_ARG: B < 1 or a NULL argument. */
int vbt_mjpeg_decode(vbt_mjpeg_decoder* d, const uint8_t* host_bytes, const uint64_t* offsets, int B, uint8_t* frames_dev_out, void* stream);
/* The scan status of every frame of the last batch (B words, codes above): ONE synchronisation of `stream`, one copy.
 * VBT_ERR_STATE: nothing has been decoded yet. */
int vbt_mjpeg_decode_status(vbt_mjpeg_decoder* d, int32_t* status, void* stream);
#define VBT_MJPEG_ENTROPY_AUTO     0   /* default */
#define VBT_MJPEG_ENTROPY_INTERVAL 1   /* one lane per restart interval */
#define VBT_MJPEG_ENTROPY_SYNC     2   /* subsequences that synchronise */
/* Host only, takes effect at the next vbt_mjpeg_decode.  subseq_bytes: 0 = the default, else a power of two in 4..4096.
 * VBT_ERR_ARG otherwise, handle unchanged. */
int vbt_mjpeg_decoder_set_entropy(vbt_mjpeg_decoder* d, int mode, int subseq_bytes);
/* The mode, the subsequence size SYNC would use (the default resolved) and AUTO's threshold; any pointer may be NULL. */
int vbt_mjpeg_decoder_get_entropy(vbt_mjpeg_decoder* d, int* mode, int* subseq_bytes, int* auto_min_interval_bytes);

/* ------------------------------------------------------------------ JPEG stills --------
 * The way in for image files (the reference's cv2.imread in eval.py:173-180): one batch of JPEG files, EVERY FILE ITS OWN SIZE AND
 * SAMPLING, decoded on the device - straight to the network input, or to RGB24 frames.  The host parses the headers and uploads
 * only the compressed bytes.
 *
 * Bitstream scope, refusals, entropy decoding with its per-frame scan status codes and its two ways through an interval, and the
 * reconstruction (dequantisation, islow IDCT, fancy upsampling, JFIF colour) are those of "MJPEG import" above, word for word, with
 * one difference: no frame size is insisted on, so "a frame size other than the handle's" is not a refusal here.  The kernels are
 * the same ones; where a frame's blocks, restart positions and output lie comes from a per-frame table that travels with the
 * descriptors in the batch's ONE H2D copy (32 bytes per frame behind the 4.1 KB descriptors).
 *
 * Capacity.  A handle is up to max_batch files per batch and a BUDGET OF 8 x 8 BLOCKS FOR THE WHOLE BATCH, not per file.  A file of
 * H x W takes, with MW = ceil(W / (8 hs)) and MH = ceil(H / (8 vs)) MCUs a side, MW MH (hs vs + 2) blocks in colour and MW MH in
 * grey - vbt_jpeg_blocks tells it from the header, so that a caller can cut a file list into batches.  The scratch is 128 bytes of
 * levels, 64 bytes of planar components and one 4-byte restart-table word per block of budget (a file has fewer restart markers
 * than blocks): 196 bytes per block, 822 MB for 2^22 blocks (forty-three 1920 x 1080 files at 4:4:4, or eighty-five at 4:2:0).
 * It is allocated by the first batch, not by vbt_jpeg_stills_create, so that every refusal of an argument, a header or a batch
 * over the budget is made before any device call; that first call fails with VBT_ERR_HIP, naming the size, when the device
 * cannot give it.  The compressed bytes travel as in "MJPEG import": two pinned staging buffers used in turn, one device buffer,
 * growing on demand up to 1 GiB per batch.  One handle serves one stream at a time.
 *
 * Output.
 *   vbt_jpeg_stills_decode_resized: dst_dev = uint8 [B,h,w,3]; frame i is preprocess_image(decode(file i), (h, w), swap_rb), bit for
 *     bit - the float32 bilinear statement of vbt_resize_frames (half-pixel centres: in = (out + 0.5) scale - 0.5 with scale =
 *     float32(H_i) / float32(h); lower = max(floor(in), 0), upper = min(ceil(in), H_i - 1), lerp = in - floor(in); top = tl +
 *     (tr - tl) lx, bottom likewise, value = top + (bottom - top) ly, truncated to uint8) applied to the reconstruction above.  One
 *     kernel, one thread per output pixel: the four taps are reconstructed from the planes (upsampling and colour at full
 *     resolution) and lerped; no RGB frame at source size is written or read.  swap_rb != 0 stores B, G, R (the decoder yields RGB).
 *   vbt_jpeg_stills_decode: frame i as RGB24 [H_i, W_i, 3] at frames_dev_out + out_offsets[i] (B offsets in bytes, any alignment;
 *     the caller sizes the buffer and keeps the frames apart).
 * Both parse all B headers first and enqueue nothing on an error, the output untouched: VBT_ERR_ARG for a NULL argument, B < 1,
 * descending offsets, h or w outside 1..4096; VBT_ERR_CAPACITY for B > max_batch, a batch over the block budget or over 1 GiB of
 * compressed bytes; VBT_ERR_IO for a refused header, the text naming the frame of the batch and the reason.  Then one H2D copy and
 * four launches on `stream`; host_bytes may be reused as soon as the call returns. */
typedef struct vbt_jpeg_stills vbt_jpeg_stills;
/* Host only, no device call: the blocks one file takes of a handle's budget.  VBT_ERR_IO with the reason when the file is refused. */
int vbt_jpeg_blocks(const uint8_t* bytes, uint64_t n, uint32_t* blocks);
/* Host only, no device call.  VBT_ERR_ARG: out NULL, device < 0, max_batch outside 1..1024, block_budget outside 1..2^24.  A device
 * index the machine does not have is not seen here: the handle's first batch fails with it (VBT_ERR_HIP, "device not available",
 * as every other *_create says it), like the allocation, with nothing enqueued. */
int vbt_jpeg_stills_create(int device, int max_batch, uint64_t block_budget, vbt_jpeg_stills** out);
void vbt_jpeg_stills_destroy(vbt_jpeg_stills* s);
int vbt_jpeg_stills_decode_resized(vbt_jpeg_stills* s, const uint8_t* host_bytes, const uint64_t* offsets, int B, uint8_t* dst_dev, int h, int w, int swap_rb,
                                   void* stream);
int vbt_jpeg_stills_decode(vbt_jpeg_stills* s, const uint8_t* host_bytes, const uint64_t* offsets, int B, uint8_t* frames_dev_out, const uint64_t* out_offsets,
                           void* stream);
/* The scan status of every file of the last batch (B words): ONE synchronisation of `stream`, one copy.  VBT_ERR_STATE: nothing
 * has been decoded yet. */
int vbt_jpeg_stills_status(vbt_jpeg_stills* s, int32_t* status, void* stream);
/* As vbt_mjpeg_decoder_set_entropy / _get_entropy (VBT_MJPEG_ENTROPY_*).  AUTO keeps its rule: a batch takes SYNC when some file has
 * scan bytes / intervals >= auto_min_interval_bytes - files without restart markers, what cameras and Pillow write, are one
 * interval each. */
int vbt_jpeg_stills_set_entropy(vbt_jpeg_stills* s, int mode, int subseq_bytes);
int vbt_jpeg_stills_get_entropy(vbt_jpeg_stills* s, int* mode, int* subseq_bytes, int* auto_min_interval_bytes);

#ifdef __cplusplus
}
#endif
#endif /* VBT_HIP_H */
