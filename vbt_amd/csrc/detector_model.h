// The detector's model handle, the plan it holds (Step / Alt / Group) and the host functions its units share: detector.hip (variant
// resolution, launches, forward), planner.hip (graph ops -> plan), detector_plan.hip (parameter pool, autotuner, plan files, model
// life cycle) and detector_profile.hip (diagnostic timings).  Host code.
#pragma once
#include <cstdarg>
#include <map>
#include <tuple>
#include <vector>

#include "dev_mem.h"
#include "hip_handles.h"
#include "launchers.h"   // the argument structs / tile constants of every kernel family + the launchers
#include "plan_geom.h"

namespace vbt {

enum Family { F_STEM = 0, F_PW, F_DW, F_ADD, F_MAXPOOL, F_RESIZE, F_POST, F_MBCONV, F_SEPCONV, F_NODE, F_MULTI, F_STEMBLK, F_EXPDW, F_BAND, F_COUNT };
inline const char* const kFamilyName[F_COUNT] = {"stem_conv_mfma_i8", "pw_conv_mfma_i8", "dw_conv_f32acc", "add_requant",
                                                 "maxpool3x3s2", "resize_nn", "decode_nms", "fused_mbconv", "fused_sepconv", "fused_bifpn_node", "fused_heads_multi",
                                                 "fused_stem_block", "fused_expand_dw", "fused_sepconv_band"};

// accounting of a step: per-frame bytes / MACs and once-per-launch weight bytes of the graph ops it stands for (element counts far
// below 2^53: sums are exact in any order)
struct Cost {
  double alg_bytes_per_frame = 0, weight_bytes = 0, macs_per_frame = 0;
  Cost& operator+=(const Cost& o) { alg_bytes_per_frame += o.alg_bytes_per_frame; weight_bytes += o.weight_bytes; macs_per_frame += o.macs_per_frame; return *this; }
};

struct Step {
  int op;       // index into ops
  int family;
  // conv
  long* wp = nullptr;      // packed MFMA weights, 16x16x32 layout (device): stem kernel and the expand stage of the fused kernels
  v4i* wp64 = nullptr;     // pointwise convs: 16x16x64 layout (pack_weights64)
  int KS64 = 0;            // K-steps of 64
  v4i* wp64t = nullptr;    // the same with a tile-major part-filled last block of `ntl` tiles (pack_weights64_tail); nullptr: N % 64 == 0
  int ntl = 0;             // live 16-channel tiles of the part-filled last output block (F_PW: of wp64t; F_MBCONV: of fa.wpt / fa.wpt3); 0: none
  int res_op = -1;         // F_PW: the residual ADD evaluated in the epilogue (op = that ADD, p_op = the conv)
  long* wdm = nullptr;     // depthwise: matrix-pipe (diagonal-embedded) weights
  int* bdm = nullptr;      // depthwise: bias folded for raw int8 inputs, padded to 64
  float* mdm = nullptr;    // depthwise: multipliers padded to 64
  float* wf = nullptr;     // depthwise weights as float [k*k][C] (device)
  int* bias = nullptr;     // folded bias (device, padded)
  float* mult = nullptr;   // multipliers (device, padded)
  int KS = 0, NB = 0;
  AddQ addq = {0, 0, 0, 0, 0, 0, 0};   // F_ADD: XNNPACK qs8-vadd parameters, derived from the tensor scales
  Cost cost;               // compulsory traffic and work of the graph ops this step stands for
  // fused block (F_MBCONV / F_SEPCONV): constituent op indices (-1 = absent) and kernel arguments
  int e_op = -1, d_op = -1, p_op = -1, a_op = -1;
  int sum_op = -1;          // F_NODE: the n-ary ADD feeding the depthwise
  int src_tensor[3] = {-1, -1, -1};
  FusedArgs fa;
  int nbp = 0, lds_bytes = 0;
  int block = 0;     // F_MBCONV: the block's number in the backbone (depthwise convs before its own: b1, b2, ...), for VBT_PROJ_TAIL / VBT_FUSED_PARAMS
  // F_MBCONV: per-chunk parameter blocks (pack_fused_chunk_params) by [48-channel chunks][depthwise form, fused_params_geom.h][tile-major
  // panel of ntl tiles]; nullptr: no launch with the parameters in LDS is built for that combination
  const unsigned char* cpar[2][3][2] = {};
  int variant = -1;  // kernel variant chosen by the autotuner (-1 = heuristic default)
  double tuned_ms = 0;
  // F_MULTI: independent fused problems launched as one grid
  std::vector<Step> members;
  FusedArgs* d_multi = nullptr;
  // F_STEMBLK: stem -> depthwise -> project in one kernel (op = project op, e_op = stem op)
  StemBlockArgs sb;
  // F_BAND: SeparableConv / BiFPN node on row bands (band_block.h); members non-empty: several problems in one grid
  BandArgs bd_args;
  BandArgs* d_band = nullptr;   // device copy of the problem list (pointers are those of the whole batch); a single problem passes bd_args by value
  int band_tiles = 0;           // workgroups per image of this problem
  // F_EXPDW: expand + depthwise on whole images, expanded channels split over workgroups (expdw_block.h; op = depthwise op)
  ExpDwArgs xd;
  ExpDw2Args xd2;              // the same step on the second form of the kernel (expdw2_block.h); variant 100 + cpw runs it
  bool xd2_ok = false;
  int xd2_lds = 0, xd2_gpw = 0, xd2_gpw16 = 0;   // input pixel groups per wave on 8 / 16 waves (0: that wave count is not available)
  bool xd2_small = false;      // the small-map instantiation applies (expdw2_geom.h: expdw2_small_ok); variant 300 + cpw runs it
  // F_MBCONV on a low-resolution map: per-chunk weight records of the whole-image kernel (data == nullptr: not built)
  ImageBundle ib = {nullptr, 0, 0, 0, 0, 0, 0, 0};
};

// The graph ops a step names, its members' included (a resample or partial sum it absorbs is named by no step): the one list
// merge_side_convs, vbt_model_plan_space and vbt_model_plan_steps go by.
template <typename F>
inline void for_each_named_op(const Step& s, F&& f) {
  for (int o : {s.op, s.e_op, s.d_op, s.p_op, s.a_op, s.res_op, s.sum_op})
    if (o >= 0) f(o);
  for (const Step& ms : s.members) for_each_named_op(ms, f);
}

// A group of consecutive graph ops with alternative realisations (all bit-identical); the planner keeps
// the fastest one measured on this device at this batch size.
struct Alt {
  std::vector<Step> steps;
  std::vector<int> hidden;  // tensors that never reach HBM under this alternative
  double ms = 0;
};
struct Group {
  std::vector<Alt> alts;
  int chosen = 0;
};

}  // namespace vbt

struct vbt_model {
  vbt_model() = default;
  // Graph execs, streams and events are released before the buffers, in the order the hand-written destroy had: here in the body, which
  // runs before any member's destructor - the order of the member declarations below carries no meaning.  No hipSetDevice.
  ~vbt_model() {
    for (int k = 0; k < 4; k++) { sub_streams[k].reset(); ev_join[k].reset(); }
    ev_fork.reset();
    clear_graphs();
    cap_stream.reset();
  }
  vbt::Header hdr;
  std::vector<vbt::TensorRec> tensors;
  std::vector<vbt::OpRec> ops;
  std::vector<uint8_t> blob;
  int device = 0, max_batch = 0;
  std::vector<int8_t*> tptr;   // device pointer of each tensor ([max_batch][h][w][c])
  std::vector<size_t> telems;  // per-frame elements
  int8_t* arena = nullptr;          // (in `owned`, like frames_stage)
  uint8_t* frames_stage = nullptr;  // device staging for host frames
  vbt::DevBuf<unsigned char> out_block;   // device staging for host outputs: ONE block boxes | scores | classes | counts ...
  float* out_boxes = nullptr;             // ... these four point into
  float* out_scores = nullptr;
  float* out_classes = nullptr;
  int* out_counts = nullptr;
  vbt::PinnedBuf<unsigned char> out_host;   // ... and its pinned host mirror: vbt_detect's results come back with one copy
  size_t out_bytes = 0;
  float* d_anchors = nullptr;
  unsigned char* d_luts = nullptr;   // post-process tables (see PostArgs)
  vbt::PostArgs post = {};           // decode + NMS: everything but the ten head tensor pointers, built once with the tables ...
  int post_lds = 0;                  // ... and the kernel's dynamic LDS for the model's anchors
  std::vector<vbt::Step> steps;      // execution list (after fusion + autotuning)
  std::vector<vbt::Group> groups;
  std::vector<vbt::Step> op_steps;   // one per graph op (weights live here)
  std::vector<char> materialized;  // per tensor: written to HBM by the execution list
  int flags = 0;
  int n_sub = 1;                         // sub-batches run concurrently on side streams
  vbt::Stream sub_streams[4];
  vbt::Event ev_fork, ev_join[4];
  // hipGraph replay of the forward for launch-bound (small) batches: one executable graph per (B, buffers)
  struct GraphKey {
    const void* frames; void* boxes; void* scores; void* classes; void* counts; int B;
    bool operator<(const GraphKey& o) const {
      return std::tie(frames, boxes, scores, classes, counts, B) < std::tie(o.frames, o.boxes, o.scores, o.classes, o.counts, o.B);
    }
  };
  std::map<GraphKey, hipGraphExec_t> graphs;
  void clear_graphs() {   // every cached graph destroyed: the bounded cache's eviction (forward) and the destructor
    for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
    graphs.clear();
  }
  vbt::Stream cap_stream;
  int graph_max_batch = 0;  // 0 = graphs off
  bool ran_eager = false;   // one forward has been enqueued outside a stream capture (per-device LDS opt-ins, lazy uploads)
  std::vector<vbt::DevBuf<char>> owned;  // device allocations, freed with the model
  // Parameter pool: weights, biases, multipliers and argument tables are sub-allocated from a few large device chunks and
  // mirrored on the host; flush_uploads() brings a chunk up to date with ONE copy (a model used to issue ~1 800 small blocking
  // hipMemcpy calls at creation).  Off under VBT_DEBUG_FENCE, where every buffer ends at its own allocation boundary.
  struct PoolChunk { vbt::DevBuf<char> dev; std::vector<char> host; size_t used, flushed; };
  std::vector<PoolChunk> pool;
  bool pool_dirty = false;
  int last_B = 0;
};

namespace vbt {

// ---- parameter pool (detector_plan.hip) ----
// h.size() elements (at least 16 bytes, + 64 of slack) of device memory that lives as long as the model, in *dev; the bytes reach the
// device at the next flush_uploads (under VBT_DEBUG_FENCE: at once, in an allocation of their own)
int upload_bytes(vbt_model* m, const void* src, size_t bytes, void** dev);
template <typename T>
int upload(vbt_model* m, const std::vector<T>& h, T** d) { return upload_bytes(m, h.data(), h.size() * sizeof(T), (void**)d); }
// Everything uploaded since the last flush reaches the device: one copy per chunk that grew.  Called before any kernel of
// the model can run (launch_step).
int flush_uploads(vbt_model* m);

// ---- planner (planner.hip) ----
int build_plan(vbt_model* m);       // graph ops -> op_steps and groups of alternatives, weights uploaded
void finalize_plan(vbt_model* m);   // the chosen alternatives -> steps and materialized

// ---- variant resolution (detector.hip): one pure host function per launch family turns (step, variant, batch; -1 = heuristic default)
// into the launch it stands for, or refuses it.  The launches, the autotuner's candidates and the plan-file check all ask these. ----
struct Verdict {   // rc != VBT_OK: the step is refused, and `why` is the error text of its launch
  int rc = VBT_OK; char why[160] = "";
  void refuse(int code, const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(why, sizeof(why), fmt, ap); va_end(ap); rc = code; }
  int report() const { set_error("%s", why); return rc; }
};
struct PwLaunch : Verdict, PwKernel { int nb_per_y = 0, lds = 0; dim3 grid; };   // (PwKernel, PW_F_MAX_NB, pw_f_tail_built: op_args.h)
enum DwForm { DW_ROW, DW_COL, DW_TILE };
struct DwLaunch : Verdict {   // tile geometry (DW_TILE), rows per lane and row segments (DW_COL), lanes (DW_ROW / DW_COL)
  DwForm form = DW_COL; bool mdw = false; int TX = 0, TY = 0, tiles_x = 0, tiles_y = 0, lds = 0, rows = 0, nseg = 0; long total = 0; dim3 grid;
};
struct FusedPlan : Verdict {
  bool image = false; int PW = 0, PH = 0, NB = 0, maxu = 0;   // whole-image kernel: padded map, output channel blocks, work units per wave
  int TX = 0, TY = 0, tiles_x = 0, tiles_y = 0; FusedLaunch L{};   // (whole image: k, stride and lds_bytes of L)
};
struct ExpDwLaunch : Verdict {   // chunks per workgroup; second form: waves per workgroup, input pixel groups per wave, its small-map instantiation
  bool second = false, small = false; int cpw = 1, nw = 0, gpw = 0, lds = 0; unsigned grid = 0;
};
struct BandLaunch : Verdict { bool chained = false; int lds = 0; };
struct StemLaunch : Verdict { bool direct = false; };
PwLaunch resolve_pw(const vbt_model* m, const Step& s, int variant, int B);
DwLaunch resolve_dw(const vbt_model* m, const Step& s, int variant, int B);
FusedPlan resolve_fused(const vbt_model* m, const Step& s, int variant, int B);
ExpDwLaunch resolve_expdw(const vbt_model* m, const Step& s, int variant, int B);
BandLaunch resolve_band(const vbt_model* m, const Step& s, int variant, int B);
StemLaunch resolve_stemblk(const vbt_model* m, const Step& s, int variant, int B);

// ---- launches (detector.hip) ----
// Launches one plan step for frames [boff, boff + B) of the batch (every tensor is batch-major).  `frames` = frame boff, the first one
// of the range; the output pointers are those of the whole batch.
int launch_step(vbt_model* m, const Step& s, int B, hipStream_t st, const uint8_t* frames, float* boxes, float* scores, float* classes,
                int* counts, int boff = 0);
// ... on the model's own staging buffers (the autotuner and the diagnostic timings)
inline int launch_step_staged(vbt_model* m, const Step& s, int B, hipStream_t st) {
  return launch_step(m, s, B, st, m->frames_stage, m->out_boxes, m->out_scores, m->out_classes, m->out_counts);
}
// every step of the plan on st, enqueue only; evs: an event recorded before every step and one after the last (steps + 1 of them)
int enqueue_forward(vbt_model* m, const uint8_t* frames_dev, int B, hipStream_t st, float* boxes, float* scores, float* classes, int* counts,
                    const Event* evs);

}  // namespace vbt
