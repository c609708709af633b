/*
 * vbt_hip_diag.h - measurement and test entry points of libvbt_hip.so.  NOT part of the drop-in boundary (vbt_hip.h): nothing
 * here has a counterpart in the reference; these are what the parity tests (every graph tensor, every plan mode), the
 * autotuner tools and bench.py's roofline block use.
 */
#ifndef VBT_HIP_DIAG_H
#define VBT_HIP_DIAG_H

#include "vbt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ execution-plan flags (vbt_model_create_ex) ---------- */
/* flags: VBT_MODEL_NO_FUSION runs every graph op as its own kernel (every tensor readable by
 * vbt_model_read_tensor); the default fuses MBConv / SeparableConv blocks on LDS tiles.
 * vbt_model_create == _ex with VBT_MODEL_DEFAULT_FLAGS (or the integer in the environment variable
 * VBT_FUSION_FLAGS). */
#define VBT_MODEL_NO_FUSION 1
#define VBT_MODEL_NO_MBCONV_FUSION 2
#define VBT_MODEL_NO_SEPCONV_FUSION 4
#define VBT_MODEL_NO_NODE_FUSION 16  /* keep BiFPN resample/add ops out of the fused SeparableConv kernels */
#define VBT_MODEL_SINGLE_STREAM 32   /* do not split the batch over side streams */
#define VBT_MODEL_NO_GRAPH 64        /* never replay the forward from a captured hipGraph */
#define VBT_MODEL_NO_HEAD_BATCHING 128 /* one launch per head layer and level instead of one per layer */
#define VBT_MODEL_NO_STEM_FUSION 256  /* stem conv as its own kernel instead of stem + first SeparableConv fused */
#define VBT_MODEL_CHUNK48 2048        /* heuristic plan: 48-channel chunks in fused MBConv blocks whose expanded width allows it */
#define VBT_MODEL_IMAGE_BLOCKS 512    /* heuristic plan: whole-image MBConv kernel wherever it applies (autotuning decides otherwise) */
#define VBT_MODEL_TILE128 16384       /* heuristic plan: 128-pixel tiles in the fused MBConv blocks that allow them */
#define VBT_MODEL_NO_BAND 8192        /* do not use the row-band SeparableConv kernel of the BiFPN nodes / head layers */
#define VBT_MODEL_NO_EXPDW 4096       /* do not use the whole-image expand+depthwise kernel of the low-resolution MBConv blocks */
#define VBT_MODEL_NO_PW_MERGE 32768    /* keep the P6 conv, its pools and the lateral convs of the first BiFPN cell as separate launches */
#define VBT_MODEL_NO_AUTOTUNE 8     /* keep the heuristic plan (most fused alternative, default kernel variants) */

/* ------------------------------------------------------------------ graph introspection -------------------------------- */
/* 1 if graph tensor `tensor_id` is written to HBM by the execution plan, 0 if it only exists in LDS */
int vbt_model_tensor_materialized(const vbt_model* m, int tensor_id);
/* kernels launched per forward */
int vbt_model_num_launches(const vbt_model* m);

/* Parity/debug: copy graph tensor `tensor_id` ([B,H,W,C] int8) of the last vbt_detect to host. */
int vbt_model_read_tensor(vbt_model* m, int tensor_id, int B, int8_t* host_out);
/* Test equipment: the reverse copy, host [B,H,W,C] int8 into the buffer the plan's launches read for graph tensor `tensor_id`
 * (same checks as the read).  With vbt_detect_range_async it runs single plan steps on crafted inputs (tests/test_gpu_postprocess.py
 * drives decode + NMS alone this way); the next full forward overwrites what was written. */
int vbt_model_write_tensor(vbt_model* m, int tensor_id, int B, const int8_t* host_in);

/* The plan space: what a plan file (VBT_PLAN_FILE) may select, as the loader checks it.  One entry per step of every alternative
 * of every group, in that order; `variants` lists the values a file may name for that step.  *n = the number of entries; a `cap`
 * below it, or a step with more than 48 variants, is VBT_ERR_CAPACITY (nothing is truncated; *n still says how many are needed). */
typedef struct {
  int group, alt, step;
  int chosen;             /* 1 if `alt` is the group's current alternative */
  int variant;            /* this step's current variant */
  int first_op, last_op;  /* lowest and highest graph op the step evaluates */
  char family[32];        /* kernel family, as the plan file spells it */
  int n_variants;
  int variants[48];
} vbt_plan_step_space;
int vbt_model_plan_space(const vbt_model* m, vbt_plan_step_space* out, int cap, int* n);
/* The execution list: what vbt_detect_range_async's step indices count.  It is the chosen alternatives of the plan space AFTER the
 * planner merged the side convolutions into one launch, so it cannot be derived from vbt_model_plan_space.  Entry i = plan step i;
 * *n = vbt_model_num_launches; a `cap` below it is VBT_ERR_CAPACITY with nothing written.  Host only: nothing is launched. */
typedef struct {
  char family[32];        /* kernel family, as the plan file spells it */
  int variant;            /* the step's current variant (-1: the heuristic default) */
  int reads_frames;       /* 1 if the step reads the uint8 frames (a range holding it needs frames_dev) */
  int image0_only;        /* 1 if vbt_detect_range_async refuses the step for img0 != 0 (its grid carries whole-batch pointers) */
  int group, step;        /* where the step sits in the plan space (its group's chosen alternative); -1, -1: the merged launch */
  int first_op, last_op;  /* lowest and highest graph op the step names (resamples and partial sums it absorbs are not among them) */
  int n_members;          /* problems launched as one grid (0: a single problem) */
} vbt_plan_step_info;
int vbt_model_plan_steps(const vbt_model* m, vbt_plan_step_info* out, int cap, int* n);
/* Live 16-channel tiles of the part-filled last output block that step (group, alt, step) of the plan space runs tile-major under its
 * current variant: fused_mbconv launches built with a live-tile count and pw_conv_mfma_i8 variants 9 / 10.  0: the step runs the
 * block-major layout (a full last block, another family, no such kernel, or VBT_PROJ_TAIL turned it off); < 0: no such step. */
int vbt_model_step_proj_tail(const vbt_model* m, int group, int alt, int step);
/* 1 if step (group, alt, step) is a fused_mbconv launch that, under its current variant, fetches its chunk parameters once per workgroup and
 * hands them to its waves through LDS; 0: the step's waves load them from global memory (another family, no such kernel, the tile would not
 * fit 64 KB of LDS with the parameter area, or VBT_FUSED_PARAMS turned it off); < 0: no such step. */
int vbt_model_step_fused_params(const vbt_model* m, int group, int alt, int step);

/* ------------------------------------------------------------------ stream placement probe ----------------------------- */
/* *shared = 1 when the two streams sit on one hardware queue (their kernels cannot overlap): a single wave spins `us`
 * microseconds on each and the pair is timed.  The device must be otherwise idle. */
int vbt_streams_share_queue(void* a, void* b, int us, int* shared);

/* ------------------------------------------------------------------ per-kernel accounting and timing ------------------- */
/* Per-kernel-family accounting of the last enqueued forward: fills up to `cap` entries.
 * Algorithmic bytes = inputs read once + output written once + weights once. */
typedef struct {
  char name[32];
  int launches;
  double algorithmic_bytes;
  double macs;
} vbt_kernel_stat;
int vbt_model_kernel_stats(const vbt_model* m, int B, vbt_kernel_stat* out, int cap, int* n);
/* Per-launch profile of the execution plan (one forward in flight, HIP events around every launch; average of `reps`):
 * entry i = launch i of the forward.  `op` / `first_op` = last / first graph op the launch covers. */
typedef struct {
  char family[32];
  int op, first_op, variant;
  double ms, algorithmic_bytes, macs;
} vbt_step_time;
int vbt_model_profile_steps(vbt_model* m, const uint8_t* frames_dev, int B, int reps, void* stream, vbt_step_time* out, int cap, int* n);
/* Measurement: each plan step `reps` times on one stream (single_ms, per launch) and on `nstreams` streams at once
 * (conc_ms, wall time per launch): how much of a step the other forwards in flight can hide. */
int vbt_model_profile_overlap(vbt_model* m, int B, int reps, int nstreams, float* single_ms, float* conc_ms, int cap, int* n);

/* Time each kernel family with HIP events on `stream` over `reps` forwards of batch B
 * (frames must be device-resident). ms_out[i] = average milliseconds per forward spent in
 * family i (same order as vbt_model_kernel_stats). */
int vbt_model_profile(vbt_model* m, const uint8_t* frames_dev, int B, int reps, void* stream,
                      double* ms_out, int cap);

/* The same, measured the way rocprofv3 --kernel-trace sees it: all launches of a family back to back between ONE pair of HIP
 * events (`reps` passes), no event pair around every short launch.  ms_out[i] = milliseconds per pass of family i. */
int vbt_model_profile_families(vbt_model* m, int B, int reps, void* stream, double* ms_out, int cap);

/* ------------------------------------------------------------------ tracking overlay ---------------------------------- */
/* What the prepare kernel of vbt_overlay_set_rows made of every row, in row order: out[i] = frame, cx, cy, xmin, ymin, xmax, ymax,
 * trail length (points) - so that a failing picture can be told from failing geometry.  *n = the handle's rows; cap < *n is
 * VBT_ERR_CAPACITY with nothing copied.  One blocking copy.  In follow mode: the records of the rows consumed so far, in log order
 * (*n = their number, read from the device first: it waits for the updates enqueued); a skipped row has trail length 0. */
int vbt_overlay_geometry(vbt_overlay* o, int32_t* out, int cap, int* n);
/* The table vbt_overlay_set_hud uploaded, read back from the device: out[i] = fs, fe, rom_cm, acv_cm, type, concentric phases among
 * phases 0..i - so that a failing panel pixel can be told from a wrong integer.  *P = the panel's phases (0 without a panel);
 * cap < *P is VBT_ERR_CAPACITY with nothing copied.  One blocking copy.  A panel that follows the live analysis
 * (vbt_overlay_hud_follow): the table as the updates COMPLETED so far left it, *P read from the device first.  The copies are plain
 * blocking copies: they wait for updates enqueued on the null stream or on a stream that synchronises with it, not for one on a
 * non-blocking stream (the pipeline's tracker stream) - synchronise that stream, or a stream ordered behind it such as the one
 * vbt_pipeline_overlay_draw was given, before the call. */
int vbt_overlay_hud_table(vbt_overlay* o, int32_t* out /*[P][6]*/, int cap, int* P);

/* MJPEG import, measurement (tools/mjpeg_decode_bench.py).  With VBT_MJPEG_DECODE_STAMPS=1 in the environment of
 * vbt_mjpeg_decoder_create, every vbt_mjpeg_decode records a HIP event around each of its stages; this call waits for the last one and
 * gives the six stage times of the last batch in milliseconds: H2D copy, memsets, marker scan, entropy decode, IDCT, upsampling +
 * colour.  VBT_ERR_STATE without the variable or before the first decode. */
int vbt_mjpeg_decode_stage_ms(vbt_mjpeg_decoder* d, float* ms6);
/* How the last batch's entropy stage ran: info4 = { path taken (VBT_MJPEG_ENTROPY_INTERVAL or _SYNC), subseq_bytes used (0 on
 * INTERVAL), the most rounds any chunk took, intervals finished by the single lane }.  One synchronisation of `stream`, one copy.
 * VBT_ERR_STATE before the first decode. */
int vbt_mjpeg_decode_entropy_info(vbt_mjpeg_decoder* d, int32_t* info4, void* stream);
/* JPEG stills, measurement (tools/eval_jpeg_bench.py): the same two queries for a vbt_jpeg_stills handle - the sixth stage time is
 * upsampling + colour (vbt_jpeg_stills_decode) or upsampling + colour + resize (vbt_jpeg_stills_decode_resized); the variable is read
 * by the handle's first batch - and the bytes of the last batch's one H2D copy (0 before the first batch). */
int vbt_jpeg_stills_stage_ms(vbt_jpeg_stills* s, float* ms6);
int vbt_jpeg_stills_entropy_info(vbt_jpeg_stills* s, int32_t* info4, void* stream);
int vbt_jpeg_stills_uploaded_bytes(vbt_jpeg_stills* s, uint64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* VBT_HIP_DIAG_H */
