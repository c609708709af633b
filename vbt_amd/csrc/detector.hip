// EfficientDet-Lite int8 detector on gfx950 (MI355X): execution plan (planner + autotuner), launches and the C ABI.
// The single-op kernels are in op_kernels.h, the host-side weight layouts in weight_pack.h and the planner in planner.h (all three
// included below); the fused kernel families live in their own translation units (k_*.hip, reached through launchers.h).
//
// Replaces the TFLite interpreter invoke at reference odt.py:58-66 (signature_fn(images=...)).
// Arithmetic contract = the kernels tflite-runtime 2.14 executes on x86-64 (XNNPACK delegate by default, TFLite builtin
// kernels for what it does not take; table in vbt_amd/quant.py), bit-exact with oracle/detector.c:
//   conv:  acc(int32) = sum (x_q - z_x) * w_q + bias_q ;  q = clamp(rne(float(acc) * M[c]) + z_y)   (XNNPACK qs8-qc8w, fp32)
//   add :  q = clamp(((bias + a*a_mult + b*b_mult) >> shift) + z_y), binary, integer                 (XNNPACK qs8-vadd-minmax)
//   post:  LOGISTIC / DEQUANTIZE tables, centre-size decode in double rounded to float once per quantity, greedy NMS in
//          (score desc, anchor asc) order                                                            (detection_postprocess.cc)
// Design (MI355X-first):
//   * activations int8 NHWC, batch-major [B][H][W][C]; pointwise convs run on the double-rate int8 MFMA
//     (v_mfma_i32_16x16x64_i8; the stem conv and the fused tiles' expand / project stages on v_mfma_i32_16x16x32_i8) with the
//     WEIGHTS as the A operand so every lane ends up holding 16 consecutive output channels of one pixel -> one 16-byte
//     coalesced store per lane;
//   * stand-alone depthwise convs: row / column walkers (v_cvt_f32_ubyteN + v_fma_f32, exact: |sum| < 2^24, 4 channels per
//     lane on contiguous NHWC channel vectors) or LDS tiles on the matrix pipe (diagonal-embedded weights);
//   * zero points are folded into the bias on the host at load time; padding uses the zero point;
//   * decode + NMS: one workgroup per frame, 256-bin score histogram -> bitonic sort of the top
//     candidates in LDS -> greedy suppression by one wavefront with ballot/shuffle.
#include <algorithm>
#include <cmath>
#include <chrono>
#include <functional>
#include <map>
#include <set>
#include <type_traits>
#include <tuple>

#include "dev_mem.h"
#include "launchers.h"   // dev_common.h + the argument structs / tile constants of every kernel family + the launchers

namespace vbt {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int use_device(const char* fn, int device, bool set_current) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    set_error("%s: HIP device %d not available (%d visible) - no CPU fallback", fn, device, ndev);
    return VBT_ERR_HIP;
  }
  if (set_current) VBT_HIP_CHECK(hipSetDevice(device));
  return VBT_OK;
}

bool lds_opt_in(const void* fn, LdsOptIn* state) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { set_error("lds_opt_in: no current HIP device"); return false; }
  if (state->dev[dev] > 0) return true;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("device %d refuses more than 64 KB of dynamic LDS for a kernel that needs it: %s", dev, hipGetErrorString(e));
    return false;
  }
  state->dev[dev] = 1;
  return true;
}

#include "op_kernels.h"   // the single-op kernels (pw_a / pw_b / pw_c / pw_d, stem, depthwise, add, pool, resize, decode + NMS, frame resize)

// ------------------------------------------------------------------------------------------
// host: model, plan, launches
// ------------------------------------------------------------------------------------------
enum Family { F_STEM = 0, F_PW, F_DW, F_ADD, F_MAXPOOL, F_RESIZE, F_POST, F_MBCONV, F_SEPCONV, F_NODE, F_MULTI, F_STEMBLK, F_EXPDW, F_BAND, F_COUNT };
static const char* kFamilyName[F_COUNT] = {"stem_conv_mfma_i8", "pw_conv_mfma_i8", "dw_conv_f32acc", "add_requant",
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
  // F_MBCONV on a low-resolution map: per-chunk weight records of the whole-image kernel (data == nullptr: not built)
  ImageBundle ib = {nullptr, 0, 0, 0, 0, 0, 0, 0};
};

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

using namespace vbt;

struct vbt_model {
  Header hdr;
  std::vector<TensorRec> tensors;
  std::vector<OpRec> ops;
  std::vector<uint8_t> blob;
  int device = 0, max_batch = 0;
  std::vector<int8_t*> tptr;   // device pointer of each tensor ([max_batch][h][w][c])
  std::vector<size_t> telems;  // per-frame elements
  int8_t* arena = nullptr;
  uint8_t* frames_stage = nullptr;  // device staging for host frames
  float* out_boxes = nullptr;       // device staging for host outputs: ONE block boxes | scores | classes | counts ...
  float* out_scores = nullptr;
  float* out_classes = nullptr;
  int* out_counts = nullptr;
  unsigned char* out_host = nullptr;   // ... and its pinned host mirror: vbt_detect's results come back with one copy
  size_t out_bytes = 0;
  float* d_anchors = nullptr;
  unsigned char* d_luts = nullptr;   // post-process tables (see PostArgs)
  std::vector<float> post_tables_host;   // scores indexed by rank byte + 128
  std::vector<Step> steps;      // execution list (after fusion + autotuning)
  std::vector<Group> groups;
  std::vector<Step> op_steps;   // one per graph op (weights live here)
  std::vector<char> materialized;  // per tensor: written to HBM by the execution list
  int flags = 0;
  int n_sub = 1;                         // sub-batches run concurrently on side streams
  hipStream_t sub_streams[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
  // hipGraph replay of the forward for launch-bound (small) batches: one executable graph per (B, buffers)
  struct GraphKey {
    const void* frames; void* boxes; void* scores; void* classes; void* counts; int B;
    bool operator<(const GraphKey& o) const {
      return std::tie(frames, boxes, scores, classes, counts, B) < std::tie(o.frames, o.boxes, o.scores, o.classes, o.counts, o.B);
    }
  };
  std::map<GraphKey, hipGraphExec_t> graphs;
  hipStream_t cap_stream = nullptr;
  int graph_max_batch = 0;  // 0 = graphs off
  bool ran_eager = false;   // one forward has been enqueued outside a stream capture (per-device LDS opt-ins, lazy uploads)
  std::vector<void*> owned;  // device allocations to free
  // Parameter pool: weights, biases, multipliers and argument tables are sub-allocated from a few large device chunks and
  // mirrored on the host; flush_uploads() brings a chunk up to date with ONE copy (a model used to issue ~1 800 small blocking
  // hipMemcpy calls at creation).  Off under VBT_DEBUG_FENCE, where every buffer ends at its own allocation boundary.
  struct PoolChunk { char* dev; std::vector<char> host; size_t used, flushed; };
  std::vector<PoolChunk> pool;
  bool pool_dirty = false;
  int last_B = 0;
};

namespace vbt {

// Debug "electric fence" (VBT_DEBUG_FENCE=1): every device buffer is placed so that it ENDS at the end of its own
// 2 MiB-granular allocation; a kernel reading past the documented slack then touches unmapped memory and faults
// instead of silently reading a neighbour.  Used once per model family by tests/tools, never in production.
static bool fence_on() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("VBT_DEBUG_FENCE"); v = (e && e[0] == '1') ? 1 : 0; }
  return v == 1;
}
static hipError_t fenced_malloc(vbt_model* m, void** out, size_t bytes) {
  if (!fence_on()) {
    hipError_t e = hipMalloc(out, bytes);
    if (e == hipSuccess) m->owned.push_back(*out);
    return e;
  }
  const size_t G = 2u << 20;
  size_t total = (bytes + G - 1) / G * G;
  char* base = nullptr;
  hipError_t e = hipMalloc((void**)&base, total);
  if (e != hipSuccess) return e;
  m->owned.push_back(base);
  *out = base + ((total - bytes) & ~(size_t)255);   // keep 256-B alignment; the buffer ends <= 255 B before the fence
  return hipSuccess;
}

constexpr size_t POOL_CHUNK = 32u << 20;
static int pool_alloc(vbt_model* m, size_t bytes, void** dev, char** host) {
  bytes = (bytes + 255) & ~(size_t)255;   // 256-byte alignment, like hipMalloc
  if (m->pool.empty() || m->pool.back().used + bytes > m->pool.back().host.size()) {
    vbt_model::PoolChunk c;
    c.dev = nullptr; c.used = 0; c.flushed = 0;
    const size_t cap = std::max(POOL_CHUNK, bytes);
    VBT_HIP_CHECK(hipMalloc((void**)&c.dev, cap));
    m->owned.push_back(c.dev);
    c.host.assign(cap, 0);
    m->pool.push_back(std::move(c));
  }
  vbt_model::PoolChunk& c = m->pool.back();
  *dev = c.dev + c.used;
  *host = c.host.data() + c.used;
  c.used += bytes;
  m->pool_dirty = true;
  return VBT_OK;
}
// Everything uploaded since the last flush reaches the device: one copy per chunk that grew.  Called before any kernel of
// the model can run (launch_step).
static int flush_uploads(vbt_model* m) {
  if (!m->pool_dirty) return VBT_OK;
  for (auto& c : m->pool)
    if (c.used > c.flushed) {
      VBT_HIP_CHECK(hipMemcpy(c.dev + c.flushed, c.host.data() + c.flushed, c.used - c.flushed, hipMemcpyHostToDevice));
      c.flushed = c.used;
    }
  m->pool_dirty = false;
  return VBT_OK;
}

template <typename T>
static int upload(vbt_model* m, const std::vector<T>& h, T** d) {
  size_t bytes = std::max<size_t>(h.size() * sizeof(T), 16);
  if (fence_on()) {
    VBT_HIP_CHECK(fenced_malloc(m, (void**)d, bytes + 64));
    if (!h.empty()) VBT_HIP_CHECK(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return VBT_OK;
  }
  char* host = nullptr;
  int rc = pool_alloc(m, bytes + 64, (void**)d, &host);   // (+64: kernels read K-padding bytes past a weight row's end)
  if (rc) return rc;
  if (!h.empty()) memcpy(host, h.data(), h.size() * sizeof(T));
  return VBT_OK;
}

#include "weight_pack.h"   // the weight / bias layouts of every kernel family: one pure host function each
#include "planner.h"       // graph ops -> Steps, alternatives and groups (build_plan / fuse_plan / finalize_plan)

// ---- variant resolution: one pure host function per launch family turns (step, variant, batch; -1 = heuristic default) into the
// launch it stands for, or refuses it.  The launches, the autotuner's candidates and the plan-file check all ask these. ----
struct Verdict {   // rc != VBT_OK: the step is refused, and `why` is the error text of its launch
  int rc = VBT_OK; char why[160] = "";
  void refuse(int code, const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(why, sizeof(why), fmt, ap); va_end(ap); rc = code; }
  int report() const { set_error("%s", why); return rc; }
};

// pointwise conv (one conv; the merged launch of merge_side_convs has no variants)
enum PwForm { PW_A, PW_B, PW_C, PW_D, PW_E };
struct PwLaunch : Verdict { PwForm form = PW_B; int ms = 1, nbt = 1, nb_per_y = 0, lds = 0; dim3 grid; };
static PwLaunch resolve_pw(const vbt_model* m, const Step& s, int variant, int B) {
  PwLaunch L;
  const TensorRec& to = m->tensors[m->ops[s.res_op >= 0 ? s.p_op : s.op].output];
  const long M = (long)B * to.h * to.w;
  if (s.KS64 <= 4) {   // K <= 256 (pw_a_kernel): variant bit 0 = two pixel groups per wave
    L.form = PW_A;
    L.ms = variant >= 0 ? (variant & 1) + 1 : (M >= 32768 ? 2 : 1);
    const long waves = (M + 16 * L.ms - 1) / (16 * L.ms);
    const unsigned gx = (unsigned)((waves + 3) / 4);
    int ysplit = 1;
    while (gx * ysplit < 1024 && ysplit < s.NB) ysplit++;
    L.nb_per_y = (s.NB + ysplit - 1) / ysplit;
    L.grid = dim3(gx, (s.NB + L.nb_per_y - 1) / L.nb_per_y);
    return L;
  }
  // VBT_PW_VARIANT (tests): the kernel variant of every pointwise conv with K > 256, whatever the plan says
  static const int pw_force = getenv("VBT_PW_VARIANT") ? atoi(getenv("VBT_PW_VARIANT")) : -100;
  if (pw_force != -100) variant = pw_force;
  if (variant >= 3 && variant <= 6) {   // 64 (3 / 5) or 128 (4 / 6) pixels per workgroup; weights shared through LDS (3 / 4: pw_d_kernel)
    L.form = variant <= 4 ? PW_D : PW_E;   // or the block's whole weight panel in LDS and a K loop without barriers (5 / 6: pw_e_kernel)
    L.ms = 2 - (variant & 1);
    L.lds = L.form == PW_E ? s.KS64 * 4096 : 0;
    L.grid = dim3((unsigned)((M + 64 * L.ms - 1) / (64 * L.ms)), (unsigned)s.NB);
    if (L.lds > 160 * 1024) L.refuse(VBT_ERR_ARG, "pw_conv: a weight panel of %d bytes does not fit the LDS", L.lds);
  } else if (variant == 2) {   // split-K over the 4 waves of a workgroup
    // one 64-channel block per workgroup (16 KB of LDS for the cross-wave reduction, twice the workgroups) rather than two
    // (32 KB): +1.4 % end to end with three forwards in flight - the workgroups of one launch then fit the CUs in one round.
    // Two pixel groups per workgroup (half the weight bytes through L1) as long as the grid still has two workgroups per CU.
    L.form = PW_C;
    L.ms = ((M + 31) / 32) * s.NB >= 512 ? 2 : 1;
    L.grid = dim3((unsigned)((M + 16 * L.ms - 1) / (16 * L.ms)), (unsigned)s.NB);
  } else {   // K streamed through registers (pw_b_kernel), nbt 64-channel blocks per wave
    const unsigned gx = (unsigned)(((M + 15) / 16 + 3) / 4);
    L.nbt = std::min(s.NB, 4);   // (1 or 2 blocks per wave measured no better: 93.0 / 92.7 k vs 93.0 k frames/s)
    if (gx < 512 && L.nbt > 2) L.nbt = 2;  // more workgroups for the low-resolution layers
    if (gx < 128) L.nbt = 1;
    L.grid = dim3(gx, (s.NB + L.nbt - 1) / L.nbt);
  }
  return L;
}
static int launch_pw_step(const vbt_model* m, const Step& s, int B, hipStream_t st, const int8_t* x, const int8_t* res, int8_t* out) {
  const PwLaunch L = resolve_pw(m, s, s.variant, B);
  if (L.rc) return L.report();
  const OpRec& pop = m->ops[s.res_op >= 0 ? s.p_op : s.op];
  const TensorRec& tpo = m->tensors[pop.output];
  const Epi e{s.bias, s.mult, tpo.zero_point, pop.act_min, pop.act_max, make_rq(tpo.zero_point, pop.act_min, pop.act_max)};
  const ResArgs ra{res, s.addq};
  const long M = (long)B * tpo.h * tpo.w;
  const int K = m->tensors[pop.inputs[0]].c, N = tpo.c;
#define PW(KERNEL, LDS) KERNEL<<<L.grid, 256, LDS, st>>>(x, s.wp64, e, ra, out, M, K, s.KS64, N, s.NB)
#define PW_A(KS) (L.ms == 2 ? pw_a_kernel<KS, 2><<<L.grid, 256, 0, st>>>(x, s.wp64, e, ra, out, M, K, N, s.NB, L.nb_per_y) \
                            : pw_a_kernel<KS, 1><<<L.grid, 256, 0, st>>>(x, s.wp64, e, ra, out, M, K, N, s.NB, L.nb_per_y))
  switch (L.form) {
    case PW_A: if (s.KS64 == 1) PW_A(1); else if (s.KS64 == 2) PW_A(2); else if (s.KS64 == 3) PW_A(3); else PW_A(4); break;
    case PW_D: if (L.ms == 2) PW(pw_d_kernel<2>, 0); else PW(pw_d_kernel<1>, 0); break;
    case PW_C: if (L.ms == 2) PW((pw_c_kernel<1, 2>), 0); else PW((pw_c_kernel<1, 1>), 0); break;
    case PW_E:
      if (L.ms == 2) { if (L.lds > 64 * 1024) VBT_LDS_OPT_IN(pw_e_kernel<2, 4>); PW((pw_e_kernel<2, 4>), L.lds); }
      else { if (L.lds > 64 * 1024) VBT_LDS_OPT_IN(pw_e_kernel<1, 4>); PW((pw_e_kernel<1, 4>), L.lds); }
      break;
    case PW_B:
      if (L.nbt == 1) PW(pw_b_kernel<1>, 0); else if (L.nbt == 2) PW(pw_b_kernel<2>, 0); else if (L.nbt == 3) PW(pw_b_kernel<3>, 0); else PW(pw_b_kernel<4>, 0);
      break;
  }
#undef PW
#undef PW_A
  return VBT_OK;
}

// stand-alone depthwise conv: 0 = one output row x 4 columns per lane, 100 / 101 = LDS tiles, chunk-parallel (101: depthwise on the
// matrix pipe), anything else = column walker with `variant` output rows per lane (-1: rows chosen by the map size)
enum DwForm { DW_ROW, DW_COL, DW_TILE };
struct DwLaunch : Verdict {   // tile geometry (DW_TILE), rows per lane and row segments (DW_COL), lanes (DW_ROW / DW_COL)
  DwForm form = DW_COL; bool mdw = false; int TX = 0, TY = 0, tiles_x = 0, tiles_y = 0, lds = 0, rows = 0, nseg = 0; long total = 0; dim3 grid;
};
static DwLaunch resolve_dw(const vbt_model* m, const Step& s, int variant, int B) {
  DwLaunch L;
  const OpRec& op = m->ops[s.op];
  const TensorRec& to = m->tensors[op.output];
  if (variant == 100 || variant == 101) {
    L.form = DW_TILE; L.mdw = variant == 101;
    choose_tile(to.h, to.w, op.k, op.stride, false, &L.TX, &L.TY);
    L.tiles_x = (to.w + L.TX - 1) / L.TX;
    L.tiles_y = (to.h + L.TY - 1) / L.TY;
    const int TXp = (L.TX + 3) & ~3;
    L.lds = ((TXp - 1) * op.stride + op.k) * ((L.TY - 1) * op.stride + op.k) * 80;
    L.grid = dim3((unsigned)((long)B * L.tiles_x * L.tiles_y), (unsigned)((to.c + 63) / 64));
  } else if (variant == 0) {
    L.form = DW_ROW;
    L.total = (long)B * to.h * ((to.w + 3) / 4) * (to.c / 4);
    L.grid = dim3((unsigned)((L.total + 255) / 256));
  } else {
    const long per_seg = (long)B * ((to.w + 3) / 4) * (to.c / 4);
    L.rows = std::min(variant > 0 ? variant : (int)std::min<long>(std::max<long>(to.h * per_seg / 400000, 1), 16), to.h);
    L.nseg = (to.h + L.rows - 1) / L.rows;
    L.total = per_seg * L.nseg;
    L.grid = dim3((unsigned)((L.total + 255) / 256));
  }
  return L;
}
static int launch_dw_step(const vbt_model* m, const Step& s, int B, hipStream_t st, const int8_t* x, int8_t* out, const Epi& e) {
  const DwLaunch L = resolve_dw(m, s, s.variant, B);
  if (L.rc) return L.report();
  const OpRec& op = m->ops[s.op];
  const TensorRec& ti = m->tensors[op.inputs[0]];
  const TensorRec& to = m->tensors[op.output];
  if (L.form == DW_TILE) {
    DwTileArgs a;
    a.x = x; a.out = out; a.wf = s.wf; a.bias = s.bias; a.mult = s.mult; a.wdm = s.wdm; a.bdm = s.bdm; a.mdm = s.mdm;
    a.H = ti.h; a.W = ti.w; a.C = to.c; a.OH = to.h; a.OW = to.w; a.pad_t = op.pad_t; a.pad_l = op.pad_l;
    a.TX = L.TX; a.TY = L.TY; a.tiles_x = L.tiles_x; a.tiles_y = L.tiles_y; a.zx = ti.zero_point; a.rq = e.rq;
    return launch_dw_tile(a, op.k, op.stride, L.mdw, L.grid, L.lds, st);
  }
  const unsigned pb = (unsigned)((128 + ti.zero_point) & 255);
  const unsigned pad4 = pb | (pb << 8) | (pb << 16) | (pb << 24);
#define DW_LAUNCH(KERNEL, ...)                                                                    \
  do {                                                                                            \
    if (op.k == 3 && op.stride == 1) KERNEL<3, 1><<<L.grid, 256, 0, st>>>(__VA_ARGS__);           \
    else if (op.k == 3 && op.stride == 2) KERNEL<3, 2><<<L.grid, 256, 0, st>>>(__VA_ARGS__);      \
    else if (op.k == 5 && op.stride == 1) KERNEL<5, 1><<<L.grid, 256, 0, st>>>(__VA_ARGS__);      \
    else KERNEL<5, 2><<<L.grid, 256, 0, st>>>(__VA_ARGS__);                                       \
  } while (0)
  if (L.form == DW_ROW) DW_LAUNCH(dw_kernel, x, s.wf, e, out, L.total, ti.h, ti.w, to.c, to.h, to.w, op.pad_t, op.pad_l, pad4);
  else DW_LAUNCH(dw_col_kernel, x, s.wf, e, out, L.total, ti.h, ti.w, to.c, to.h, to.w, op.pad_t, op.pad_l, pad4, L.rows, L.nseg);
#undef DW_LAUNCH
  return VBT_OK;
}

// fused MBConv / SeparableConv / BiFPN node on LDS tiles (fused_block.h) or, MBConv on a low-resolution map, one workgroup per image
// (image_block.h).  Variant bits: 1 = depthwise on the matrix pipe (else VALU), 2 = half-height tile, 4 = whole image, 8 = 48-channel
// chunks, 16 = 128-pixel (16 x 8) tiles, 32 = band-Toeplitz depthwise (fused_block.h: TPZ); a bit whose conditions the step does not
// meet is ignored, except that the whole-image and 128-pixel kernels refuse a step they do not fit and that bit 32 resolves only as
// 33, 41, 49 or 57 on a step where each of its other bits holds.
struct FusedPlan : Verdict {
  bool image = false; int PW = 0, PH = 0, NB = 0, maxu = 0;   // whole-image kernel: padded map, output channel blocks, work units per wave
  int TX = 0, TY = 0, tiles_x = 0, tiles_y = 0; FusedLaunch L{};   // (whole image: k, stride and lds_bytes of L)
};
static FusedPlan resolve_fused(const vbt_model* m, const Step& s, int variant, int B) {
  const FusedArgs& a = s.fa;
  const OpRec& dop = m->ops[s.d_op];
  const int k = dop.k, stride = dop.stride;
  const bool ex = s.family == F_MBCONV, ks12 = a.KSe == 1 || a.KSe == 2;
  int var = variant;
  if (var < 0) {   // heuristic default: what the plan-shaping flags ask for, where it applies
    var = ((m->flags & VBT_MODEL_IMAGE_BLOCKS) && !resolve_fused(m, s, 5, B).rc) ? 5 : ((m->flags & VBT_MODEL_CHUNK48) ? 9 : 1);
    const FusedPlan p17 = (m->flags & VBT_MODEL_TILE128) ? resolve_fused(m, s, 17, B) : FusedPlan{};
    if (!p17.rc && p17.L.ppw2) var |= 16;
  }
  const bool mdw = var & 1, half = var & 2;
  const bool nt3 = (var & 8) && mdw && a.nch3 > 0 && s.nbp <= 2 && a.KSe >= 1 && a.KSe <= 4;
  FusedPlan p;
  if ((var & 32) && (var & 4)) { p.refuse(VBT_ERR_ARG, "fused_mbconv: variant %d: the Toeplitz depthwise does not apply to this step", var); return p; }
  if (var & 4) {
    const int HW = a.H * a.W, OHW = a.OH * a.OW;
    if (!ex || HW > 400 || OHW > 400 || !s.ib.data) { p.refuse(VBT_ERR_ARG, "fused_mbconv: whole-image variant not applicable"); return p; }
    p.image = true;
    p.PH = std::max((a.OH - 1) * stride + k, a.pad_t + a.H);
    p.PW = std::max((a.OW - 1) * stride + k, a.pad_l + a.W);
    p.NB = (a.Cout + 63) / 64;
    const int NPGo = (OHW + 15) / 16;
    const int units = (NPGo * p.NB + IB_WAVES - 1) / IB_WAVES;
    p.maxu = units <= 2 ? 2 : units <= 3 ? 3 : 4;
    p.L.k = k; p.L.stride = stride; p.L.lds_bytes = ((HW * a.T0S + 15) & ~15) + p.PH * p.PW * FB_EST + NPGo * 16 * FB_DST + s.ib.bytes;
    if (units > 4 || p.L.lds_bytes > 160 * 1024 || s.ib.bytes > 16 * IB_NPF * IB_THREADS) p.refuse(VBT_ERR_ARG, "fused_mbconv: whole-image variant not applicable");
    return p;
  }
  p.TX = a.TX;
  p.TY = half && a.TY >= 2 ? (a.TY + 1) / 2 : a.TY;
  // 128-pixel tiles (PPW = 2): matrix-pipe depthwise on the 16x16x64 MFMA, register-resident expand weights (K <= 64), <= 128 output channels
  const bool ppw2 = (var & 16) && ex && mdw && ks12 && s.nbp <= 2 && !half;
  if (ppw2) { p.TX = 16; p.TY = 8; }
  // otherwise 64-pixel tiles of exactly 8 x 8 outputs with the same limits take the 16x16x64 depthwise too (DW64)
  const bool dw64 = ppw2 || (ex && mdw && a.wd64 && p.TX == 8 && p.TY == 8 && ks12 && s.nbp <= 2);
  const int est = !ex ? 0 : !nt3 ? FB_EST : dw64 ? 48 : 72;   // E row bytes (fused_block.h: EST)
  // Toeplitz depthwise (bit 32): a form of dw64, selected by exactly 33, 41, 49 or 57 on a step it is built for - refused anywhere else
  const bool tpz = var & 32;
  const bool tpz_ok = tpz && dw64 && a.wtz && fused_tpz_built(k, stride, s.nbp, a.KSe, ppw2) && (var & ~(1 | 8 | 16 | 32)) == 0 && nt3 == bool(var & 8) && ppw2 == bool(var & 16);
  const TpzGeom tg = tpz_ok ? tpz_geom(k, stride, ppw2 ? 2 : 1, nt3 ? 3 : 4) : TpzGeom{};
  const int e_bytes = tpz_ok ? tg.e_bytes + 8 * tg.DSK : -1;   // (with the tile rows' shift of D)
  p.tiles_x = (a.OW + p.TX - 1) / p.TX;
  p.tiles_y = (a.OH + p.TY - 1) / p.TY;
  p.L = FusedLaunch{k, stride, s.nbp, ex, mdw, nt3, ppw2, dw64, fused_tile_lds(a, k, stride, p.TX, p.TY, est, ppw2 ? 2 : 1, s.nbp, e_bytes),
                    (unsigned)((long)B * p.tiles_x * p.tiles_y), tpz_ok};
  if (ppw2 && (a.OW < 16 || a.OH < 8 || !a.wd64)) p.refuse(VBT_ERR_ARG, "fused_mbconv: the 128-pixel variant needs maps of at least 16 x 8");
  else if (ppw2 && p.L.lds_bytes > 64 * 1024) p.refuse(VBT_ERR_ARG, "fused_mbconv: 128-pixel tile needs %d bytes of LDS", p.L.lds_bytes);
  else if (tpz && !tpz_ok) p.refuse(VBT_ERR_ARG, "fused_mbconv: variant %d: the Toeplitz depthwise does not apply to this step", var);
  else if (tpz && p.L.lds_bytes > 64 * 1024) p.refuse(VBT_ERR_ARG, "fused_mbconv: the Toeplitz depthwise tile needs %d bytes of LDS", p.L.lds_bytes);
  return p;
}
static int launch_fused_step(const vbt_model* m, const Step& s, FusedArgs a, int B, hipStream_t st) {
  const FusedPlan p = resolve_fused(m, s, s.variant, B);
  if (p.rc) return p.report();
  if (p.image) return launch_mbconv_image(a, s.ib, p.L.k, p.L.stride, p.maxu, p.PW, p.PH, p.NB, p.L.lds_bytes, B, st);
  a.TX = p.TX; a.TY = p.TY; a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y;
  return launch_fused_block(a, p.L, st);
}

// expand + depthwise on whole images or row bands.  Variant: chunks per workgroup on the first form of the kernel (expdw_block.h),
// 100 + chunks per workgroup on the second (expdw2_block.h) with 8 waves, 200 + chunks with 16 waves; -1: heuristic default
struct ExpDwLaunch : Verdict {   // chunks per workgroup; second form: waves per workgroup, input pixel groups per wave
  bool second = false; int cpw = 1, nw = 0, gpw = 0, lds = 0; unsigned grid = 0;
};
static ExpDwLaunch resolve_expdw(const vbt_model*, const Step& s, int variant, int B) {
  // VBT_XD_VARIANT (tests): that variant for every step that supports it, whatever the plan says
  static const int xd_force = getenv("VBT_XD_VARIANT") ? atoi(getenv("VBT_XD_VARIANT")) : -100;
  if (xd_force != -100 && (xd_force < 100 || (s.xd2_ok && (xd_force < 200 ? s.xd2_gpw > 0 : s.xd2_gpw16 > 0)))) variant = std::min(xd_force, xd_force / 100 * 100 + s.xd.nchunks);
  ExpDwLaunch L;
  if (s.xd2_ok && (variant >= 100 || variant < 0)) {
    if (variant >= 200 && s.xd2_gpw16 == 0) { L.refuse(VBT_ERR_ARG, "expand + depthwise: plan asks for the 16-wave form on a step that does not support it"); return L; }
    if (variant >= 100 && variant < 200 && s.xd2_gpw == 0) { L.refuse(VBT_ERR_ARG, "expand + depthwise: plan asks for the 8-wave form on a step that does not support it"); return L; }
    const ExpDw2Args& a = s.xd2;   // the second form
    L.second = true;
    L.nw = (variant >= 200 || (variant < 0 && s.xd2_gpw16 > 0)) ? 16 : 8;
    L.gpw = L.nw == 16 ? s.xd2_gpw16 : s.xd2_gpw;
    L.cpw = std::min(variant >= 100 ? variant % 100 : std::max(1, (a.nchunks * a.nbands * B + 1023) / 1024), a.nchunks);   // default: about four workgroups per CU
    L.grid = (unsigned)(B * ((a.nchunks + L.cpw - 1) / L.cpw) * a.nbands);
    L.lds = s.xd2_lds;
    return L;
  }
  if (variant >= 100) { L.refuse(VBT_ERR_ARG, "expand + depthwise: plan asks for the second kernel form on a step that does not support it"); return L; }
  const ExpDwArgs& a = s.xd;
  L.cpw = variant > 0 ? variant : std::max(1, (a.nchunks * a.nbands * B + 511) / 512);   // default: about two workgroups per CU
  L.grid = (unsigned)(B * ((a.nchunks + L.cpw - 1) / L.cpw) * a.nbands);
  L.lds = s.lds_bytes;
  return L;
}
static int launch_expdw_step(const vbt_model* m, const Step& s, int B, hipStream_t st, const int8_t* x, int8_t* out) {
  const ExpDwLaunch L = resolve_expdw(m, s, s.variant, B);
  if (L.rc) return L.report();
  const OpRec& dop = m->ops[s.d_op];
  if (L.second) {
    ExpDw2Args a = s.xd2;
    a.x = x; a.out = out; a.cpw = L.cpw;
    return launch_expdw2(a, dop.k, dop.stride, (a.Cin + 63) / 64, L.nw, L.gpw, L.grid, L.lds, st);
  }
  ExpDwArgs a = s.xd;
  a.x = x; a.out = out; a.cpw = L.cpw;
  return launch_expdw(a, dop.k, dop.stride, (a.Cin + 63) / 64, L.grid, L.lds, st);
}

// SeparableConv / BiFPN node / head layer on row bands.  Variant: 0 = depthwise and projection as two stages around the LDS tile D,
// 1 = chained (band_block.h; 64-channel maps with at most 64 output channels), -1: chained where it resolves and max_batch > 8, else two stages.  A step of several
// problems carries one variant for all its members.
struct BandLaunch : Verdict { bool chained = false; int lds = 0; };
static bool band_chainable(const Step& s) {
  if (s.members.empty()) return s.bd_args.wpc != nullptr;
  for (const Step& ms : s.members)
    if (!ms.bd_args.wpc) return false;
  return true;
}
static BandLaunch resolve_band(const vbt_model* m, const Step& s, int variant, int) {
  BandLaunch L;
  const bool can = band_chainable(s);
  // what the plan asks for is judged as it stands, before any override: a variant that does not exist for the step is never offered
  if (variant < -1 || variant > 1) { L.refuse(VBT_ERR_ARG, "fused_sepconv_band: no kernel form %d", variant); return L; }
  if (variant == 1 && !can) { L.refuse(VBT_ERR_ARG, "fused_sepconv_band: plan asks for the chained form on a step that does not support it"); return L; }
  // VBT_BAND_VARIANT (tests): that form for every step that supports it, whatever the plan says
  static const int bd_force = getenv("VBT_BAND_VARIANT") ? atoi(getenv("VBT_BAND_VARIANT")) : -100;
  if (bd_force == 0 || (bd_force == 1 && can)) variant = bd_force;
  // the default: chained where it resolves, except for models of max_batch <= 8 (64-pixel bands, make_band): forced onto them the chained
  // form lost 3-7 % at batch 1 and 1-3 % at batch 8 (profiles/r08_band_chain_ab.md section 5), so they stay on the two-stage form
  L.chained = variant == 1 || (variant < 0 && can && m->max_batch > 8);
  if (s.members.empty()) L.lds = band_lds(s.bd_args, L.chained);
  for (const Step& ms : s.members) L.lds = std::max(L.lds, band_lds(ms.bd_args, L.chained));
  if (L.lds > 160 * 1024) L.refuse(VBT_ERR_ARG, "fused_sepconv_band: a band of %d bytes does not fit the LDS", L.lds);
  return L;
}

// Launches one plan step for frames [boff, boff + B) of the batch (every tensor is batch-major): the batch-offset pointers here, the
// variant and the launch in the family's own function above.  `frames` = frame boff, the first one of the range; the output pointers
// are those of the whole batch.
static int launch_step(vbt_model* m, const Step& s, int B, hipStream_t st, const uint8_t* frames, float* boxes, float* scores,
                       float* classes, int* counts, int boff = 0) {
  if (m->pool_dirty) { const int rc = flush_uploads(m); if (rc) return rc; }
  const OpRec& op = m->ops[s.op];
  const TensorRec& to = m->tensors[op.output];
  auto TP = [&](int t) { return m->tptr[t] + (size_t)boff * m->telems[t]; };
  const uint8_t* frame0 = frames;
  int8_t* out = TP(op.output);
  // start of every member's workgroups in a grid of several problems (F_MULTI, F_BAND); start[n] = the grid
  auto member_tiles = [&](auto tiles_of) {
    MultiTiles mt;
    mt.n = (int)s.members.size();
    mt.start[0] = 0;
    for (int i = 0; i < mt.n; i++) mt.start[i + 1] = mt.start[i] + B * tiles_of(s.members[i]);
    return mt;
  };
  const Epi e{s.bias, s.mult, to.zero_point, op.act_min, op.act_max, make_rq(to.zero_point, op.act_min, op.act_max)};   // (F_PW builds its own from its conv op)
  switch (s.family) {
    case F_STEM: {
      const TensorRec& ti = m->tensors[op.inputs[0]];
      long M = (long)B * to.h * to.w;
      dim3 grid((unsigned)((M + 63) / 64));
      stem_kernel<<<grid, 256, 0, st>>>(frame0, s.wp, e, out, M, ti.h, ti.w, to.h, to.w, to.c, op.pad_t, op.pad_l, ti.zero_point);
      return VBT_OK;
    }
    case F_PW: {
      if (s.members.empty())   // op = the op whose output is written: the conv itself, or the residual ADD evaluated in its epilogue (res_op)
        return launch_pw_step(m, s, B, st, TP(m->ops[s.res_op >= 0 ? s.p_op : s.op].inputs[0]),
                              s.res_op >= 0 ? TP(m->ops[s.res_op].inputs[1]) : nullptr, out);   // ADD(conv output, skip): planner guarantees the order
      // several convs in one launch (merge_side_convs)
      if (boff != 0) { set_error("merged pointwise convs: sub-batch streams are not supported (VBT_SUBSTREAMS)"); return VBT_ERR_ARG; }
      PwMulti pm;
      memset(&pm, 0, sizeof(pm));
      const int nconv = (int)s.members.size() - (s.nbp ? 2 : 0);
      int acc = 0;
      for (int i = 0; i < nconv; i++) {
        const Step& ms = s.members[i];
        const OpRec& pop = m->ops[ms.op];
        const TensorRec& ti = m->tensors[pop.inputs[0]];
        const TensorRec& tpo = m->tensors[pop.output];
        PwProb& q = pm.p[i];
        q.x = TP(pop.inputs[0]); q.wp = ms.wp64; q.bias = ms.bias; q.mult = ms.mult; q.out = TP(pop.output);
        q.rq = make_rq(tpo.zero_point, pop.act_min, pop.act_max);
        q.K = ti.c; q.KS = ms.KS64; q.N = tpo.c; q.NB = ms.NB;
        pm.start[i] = acc;
        if (i == 0 && s.nbp) {
          const OpRec &p1 = m->ops[s.members[nconv].op], &p2 = m->ops[s.members[nconv + 1].op];
          const TensorRec &t1 = m->tensors[p1.output], &t2 = m->tensors[p2.output];
          q.M = tpo.h * tpo.w;
          q.pool1 = TP(p1.output); q.pool2 = TP(p2.output);
          q.H = tpo.h; q.W = tpo.w; q.H1 = t1.h; q.W1 = t1.w; q.pt1 = p1.pad_t; q.pl1 = p1.pad_l;
          q.H2 = t2.h; q.W2 = t2.w; q.pt2 = p2.pad_t; q.pl2 = p2.pad_l;
          acc += B;
        } else {
          q.M = B * tpo.h * tpo.w;
          acc += ((q.M + 63) / 64) * q.NB;
        }
      }
      pm.n = nconv;
      pm.start[nconv] = acc;
      for (int i = nconv + 1; i <= PWM_MAX; i++) pm.start[i] = acc;
      pw_multi_kernel<<<dim3((unsigned)acc), 256, s.nbp ? s.lds_bytes : 0, st>>>(pm);
      return VBT_OK;
    }
    case F_DW:
      return launch_dw_step(m, s, B, st, TP(op.inputs[0]), out, e);
    case F_ADD: {
      long n4 = (long)B * to.h * to.w * to.c / 4;
      add_kernel<<<dim3((unsigned)((n4 + 1023) / 1024)), 256, 0, st>>>(TP(op.inputs[0]), TP(op.inputs[1]), s.addq, out, n4);
      return VBT_OK;
    }
    case F_MAXPOOL: {
      const TensorRec& ti = m->tensors[op.inputs[0]];
      long total = (long)B * to.h * to.w * (to.c / 4);
      maxpool_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(TP(op.inputs[0]), out, total, ti.h, ti.w, ti.c,
                                                                             to.h, to.w, op.pad_t, op.pad_l);
      return VBT_OK;
    }
    case F_RESIZE: {
      const TensorRec& ti = m->tensors[op.inputs[0]];
      long total = (long)B * to.h * to.w * (to.c / 4);
      resize_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(TP(op.inputs[0]), out, total, ti.h, ti.w, ti.c,
                                                                            to.h, to.w);
      return VBT_OK;
    }
    case F_MULTI: {
      if (boff != 0) {  // side-stream sub-batches: pointers differ, launch the members one by one
        for (const Step& ms : s.members) {
          Step t = ms;
          t.variant = s.variant;
          const int rc = launch_step(m, t, B, st, frames, boxes, scores, classes, counts, boff);
          if (rc) return rc;
        }
        return VBT_OK;
      }
      const MultiTiles mt = member_tiles([](const Step& ms) { return ms.fa.tiles_x * ms.fa.tiles_y; });
      const OpRec& dop = m->ops[s.d_op];
      return launch_fused_multi(s.d_multi, mt, dop.k, dop.stride, s.nbp, s.variant != 0, s.lds_bytes, (unsigned)mt.start[mt.n], st);
    }
    case F_MBCONV:
    case F_NODE:
    case F_SEPCONV: {
      FusedArgs a = s.fa;
      a.x = s.e_op >= 0 ? TP(m->ops[s.e_op].inputs[0]) : TP(m->ops[s.d_op].inputs[0]);
      for (int j = 0; j < 3; j++) a.src[j] = s.src_tensor[j] >= 0 ? TP(s.src_tensor[j]) : nullptr;
      a.out = out;
      return launch_fused_step(m, s, a, B, st);
    }
    case F_BAND: {
      if (boff != 0) { set_error("fused_sepconv_band: sub-batch streams are not supported (VBT_SUBSTREAMS)"); return VBT_ERR_ARG; }
      const BandLaunch L = resolve_band(m, s, s.variant, B);
      if (L.rc) return L.report();
      if (s.members.empty()) return launch_band_one(s.bd_args, L.chained, (unsigned)(B * s.band_tiles), L.lds, st);
      const MultiTiles mt = member_tiles([](const Step& ms) { return ms.band_tiles; });
      return launch_band_multi(s.d_band, mt, s.members[0].bd_args.C, L.chained, (unsigned)mt.start[mt.n], L.lds, st);
    }
    case F_EXPDW:
      return launch_expdw_step(m, s, B, st, TP(m->ops[s.e_op].inputs[0]), out);
    case F_STEMBLK: {
      StemBlockArgs a = s.sb;
      a.frames = frame0;
      a.out = out;
      return launch_stem_block(a, a.rqs.full && a.rqd.full && a.rqp.full, (unsigned)((long)B * a.tiles_x * a.tiles_y), st);
    }
    case F_POST: {
      PostArgs p;
      int base = 0;
      p.C = m->hdr.num_classes > 0 ? m->hdr.num_classes : 1;
      for (int l = 0; l < 5; l++) {
        const TensorRec& tc = m->tensors[op.inputs[l]];
        p.cls[l] = TP(op.inputs[l]);
        p.box[l] = TP(op.inputs[5 + l]);
        p.base[l] = base;
        base += tc.h * tc.w * tc.c / p.C;
      }
      p.base[5] = base;
      p.anchors = m->d_anchors;
      p.tables = m->d_luts;
      p.A = m->hdr.num_anchors;
      p.max_det = m->hdr.max_detections;
      p.iou_thr = m->hdr.nms_iou_threshold;
      int qmin = 128;   // in rank bytes
      for (int q = 127; q >= -128; q--)
        if (m->post_tables_host[q + 128] >= m->hdr.nms_score_threshold) qmin = q; else break;
      p.qmin = qmin;
      const int lds = post_lds_bytes(p.A);
      if (lds > 64 * 1024) VBT_LDS_OPT_IN(postprocess_kernel);
      if (lds > 160 * 1024 || p.A > 65535) { set_error("decode + NMS: %d anchors do not fit the kernel (LDS %d bytes, 16-bit anchor index)", p.A, lds); return VBT_ERR_CAPACITY; }
      const size_t o = (size_t)boff * m->hdr.max_detections;
      postprocess_kernel<<<dim3((unsigned)B), POST_THREADS, lds, st>>>(p, boxes + 4 * o, scores + o, classes + o, counts + boff);
      return VBT_OK;
    }
  }
  return VBT_OK;
}

// VBT_AUTOTUNE_CONCURRENCY=n (default 1): time each candidate with n copies in flight on n streams (same buffers, same
// results) and rank by time per copy, i.e. by throughput under contention - what a pipelined caller (Pipeline depth n)
// experiences - instead of by isolated latency.
static double time_step(vbt_model* m, const Step& s, int B, int reps) {
  static int nconc = -1;
  static hipStream_t cs[4] = {nullptr, nullptr, nullptr, nullptr};
  if (nconc < 0) {
    const char* e = getenv("VBT_AUTOTUNE_CONCURRENCY");
    nconc = e ? std::max(1, std::min(4, atoi(e))) : 1;
    if (nconc > 1)
      for (int i = 0; i < nconc; i++) (void)hipStreamCreateWithFlags(&cs[i], hipStreamNonBlocking);
  }
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return 1e30;
  float ms = 1e30f;
  int rc = VBT_OK;   // a refused launch (nothing enqueued) makes the candidate unusable, not fast
  if (nconc <= 1) {
    rc = launch_step(m, s, B, nullptr, m->frames_stage, m->out_boxes, m->out_scores, m->out_classes, m->out_counts);
    (void)hipEventRecord(e0, nullptr);
    for (int r = 0; r < reps && !rc; r++)
      rc = launch_step(m, s, B, nullptr, m->frames_stage, m->out_boxes, m->out_scores, m->out_classes, m->out_counts);
    (void)hipEventRecord(e1, nullptr);
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) ms = 1e30f;
    ms /= reps;
  } else {
    (void)hipDeviceSynchronize();
    for (int i = 0; i < nconc && !rc; i++)
      rc = launch_step(m, s, B, cs[i], m->frames_stage, m->out_boxes, m->out_scores, m->out_classes, m->out_counts);
    (void)hipDeviceSynchronize();
    auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < reps; r++)
      for (int i = 0; i < nconc && !rc; i++)
        rc = launch_step(m, s, B, cs[i], m->frames_stage, m->out_boxes, m->out_scores, m->out_classes, m->out_counts);
    (void)hipDeviceSynchronize();
    ms = (float)(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / (reps * nconc));
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return rc ? 1e30 : ms;
}

static bool is_fused_tile(int family) { return family == F_MBCONV || family == F_SEPCONV || family == F_NODE; }
// whether `v` resolves to a launch of this step (the depthwise resolver and the families without one take any value)
static bool variant_ok(const vbt_model* m, const Step& st, int v) {
  if (st.family == F_PW) return !st.members.empty() || !resolve_pw(m, st, v, m->max_batch).rc;
  if (is_fused_tile(st.family)) return !resolve_fused(m, st, v, m->max_batch).rc;
  if (st.family == F_BAND) return !resolve_band(m, st, v, m->max_batch).rc;
  return st.family != F_EXPDW || !resolve_expdw(m, st, v, m->max_batch).rc;
}

// Plan-time autotuning: every alternative computes bit-identical tensors, so only speed is at stake.
// Kernel variants the planner offers for a step: what the autotuner times, and (with the rest of the fused tile kernels' flag
// combinations) what a plan file may select: load_plan.  -1 = the launcher's own default.  Only values that resolve are offered.
static std::vector<int> candidate_variants(const vbt_model* m, const Step& st) {
  std::vector<int> cand{-1};
  const OpRec& op = m->ops[st.op];
  if (st.family == F_DW) {
    cand = {0};
    for (int r : {1, 2, 4, 8, 16})
      if (r <= m->tensors[op.output].h) cand.push_back(r);
    if (m->tensors[op.output].c % 8 == 0) { cand.push_back(100); cand.push_back(101); }
  } else if (st.family == F_PW && st.KS64 <= 4) {
    cand = {0, 1};
  } else if (st.family == F_PW) {
    cand = {-1, 2, 3, 4, 5, 6};
  } else if (is_fused_tile(st.family)) {
    cand = {0, 1, 3, 5};   // VALU dw, matrix-pipe dw, matrix-pipe dw + half-height tile, one workgroup per image
    if (st.family == F_MBCONV && st.fa.nch3 > 0 && st.nbp <= 2 && st.fa.KSe >= 1 && st.fa.KSe <= 4) { cand.push_back(9); cand.push_back(11); }  // 48-channel chunks
    if (st.family == F_MBCONV && st.nbp <= 2 && (st.fa.KSe == 1 || st.fa.KSe == 2)) {   // 128-pixel tiles
      cand.push_back(17);
      if (st.fa.nch3 > 0) cand.push_back(25);
    }
    if (st.family == F_MBCONV && st.fa.wtz) cand.insert(cand.end(), {33, 41, 49, 57});   // Toeplitz depthwise on the four DW64 forms
  } else if (st.family == F_MULTI) {
    cand = {0, 1};
  } else if (st.family == F_EXPDW) {
    cand.clear();
    for (int cpw : {1, 2, 3, 4, 6})
      if (cpw <= st.xd.nchunks) cand.push_back(cpw);
    if (st.xd2_ok)
      for (int cpw : {1, 2, 3, 4, 6})
        if (cpw <= st.xd.nchunks) {
          if (st.xd2_gpw > 0) cand.push_back(100 + cpw);
          if (st.xd2_gpw16 > 0) cand.push_back(200 + cpw);
        }
  } else if (st.family == F_BAND) {
    cand = {-1, 0, 1};   // the launch kind's default, two stages, chained (64-channel maps only)
  }
  cand.erase(std::remove_if(cand.begin(), cand.end(), [&](int v) { return !variant_ok(m, st, v); }), cand.end());
  return cand;
}

static void autotune(vbt_model* m) {
  const int B = (m->max_batch + m->n_sub - 1) / m->n_sub, reps = 4;  // the batch one stream actually sees
  for (Group& g : m->groups) {
    bool single = g.alts.size() == 1 && g.alts[0].steps.size() == 1;
    if (single) {
      int f = g.alts[0].steps[0].family;
      if (f != F_DW && f != F_PW) continue;  // nothing to choose
    }
    for (Alt& a : g.alts) {
      a.ms = 0;
      for (Step& st : a.steps) {
        const std::vector<int> cand = candidate_variants(m, st);
        double best = 1e30;
        int bestv = -1;
        for (int v : cand) {
          Step t = st;
          t.variant = v;
          double ms = time_step(m, t, B, reps);
          if (getenv("VBT_AUTOTUNE_VERBOSE") && cand.size() > 1 && atoi(getenv("VBT_AUTOTUNE_VERBOSE")) > 1)
            fprintf(stderr, "[autotune]   op %d %s v%d %.1fus\n", st.op, kFamilyName[st.family], v, ms * 1e3);
          if (ms < best) { best = ms; bestv = v; }
        }
        st.variant = bestv;
        st.tuned_ms = best;
        a.ms += best;
      }
    }
    int bi = 0;
    for (size_t i = 1; i < g.alts.size(); i++)
      if (g.alts[i].ms < g.alts[bi].ms) bi = (int)i;
    g.chosen = bi;
    if (getenv("VBT_AUTOTUNE_VERBOSE")) {
      const Step& f = g.alts[0].steps[0];
      const TensorRec& to = m->tensors[m->ops[g.alts[0].steps.back().op].output];
      fprintf(stderr, "[autotune] op %3d.. out %3dx%3dx%4d :", f.op, to.h, to.w, to.c);
      for (size_t i = 0; i < g.alts.size(); i++) {
        fprintf(stderr, " alt%zu%s %.1fus(", i, (int)i == bi ? "*" : "", g.alts[i].ms * 1e3);
        for (const Step& st : g.alts[i].steps) fprintf(stderr, "%s:v%d=%.1f ", kFamilyName[st.family], st.variant, st.tuned_ms * 1e3);
        fprintf(stderr, ")");
      }
      fprintf(stderr, "\n");
    }
  }
  (void)hipDeviceSynchronize();
}

// Plan cache.  Format 2 (written): "VBTPLAN2 <ngroups>" then per group "<chosen alternative> <nsteps> <family>:<variant> ..." - the
// kernel family of every step of the chosen alternative by NAME, so that a file tuned for another build of the planner (an
// alternative added, removed or re-ordered: the bare indices of format 1 would still load and silently select other kernels) is
// refused and the plan re-tuned.  Format 1 ("<ngroups>" then "<chosen> <nsteps> <variant>...") is still read - the group and step
// counts are all it can be checked against - and re-written in format 2 when VBT_PLAN_CONVERT is set.
// The shape a file may select from: this library's groups, their alternatives, the family of every step and the variants that resolve
// for it (container_parse.h: parse_plan_file refuses everything else, and the model is tuned afresh).  vbt_model_plan_space reports it.
static PlanShape plan_shape(const vbt_model* m) {
  PlanShape shape;
  for (const Group& g : m->groups) {
    std::vector<std::vector<PlanStepShape>> alts;
    for (const Alt& a : g.alts) {
      std::vector<PlanStepShape> steps;
      for (const Step& st : a.steps) {
        PlanStepShape ps;
        ps.family = kFamilyName[st.family];
        ps.variants = candidate_variants(m, st);
        auto add = [&](int v) { if (std::find(ps.variants.begin(), ps.variants.end(), v) == ps.variants.end()) ps.variants.push_back(v); };
        // the fused tile kernels read their variant as a set of flags (resolve_fused): plans searched under load (tools/tune_under_load.py)
        // hold combinations the isolated autotuner does not time, and every combination that resolves is accepted
        for (int v = 0; v < 64 && is_fused_tile(st.family); v++)
          if (variant_ok(m, st, v)) add(v);
        add(-1);
        add(st.variant);   // the heuristic plan's own choice
        steps.push_back(ps);
      }
      alts.push_back(steps);
    }
    shape.groups.push_back(alts);
  }
  return shape;
}
static bool load_plan(vbt_model* m, const char* path) {
  const PlanShape shape = plan_shape(m);
  std::vector<PlanChoice> sel;
  std::string note;
  if (!parse_plan_file(path, shape, &sel, &note)) {
    if (note != "no such file") fprintf(stderr, "[vbt] plan %s: %s - plan refused, re-tuning\n", path, note.c_str());
    return false;
  }
  for (size_t gi = 0; gi < m->groups.size(); gi++) {
    m->groups[gi].chosen = sel[gi].chosen;
    Alt& a = m->groups[gi].alts[(size_t)sel[gi].chosen];
    for (size_t i = 0; i < a.steps.size(); i++) a.steps[i].variant = sel[gi].variants[i];
  }
  return true;
}
static void save_plan(const vbt_model* m, const char* path) {
  FILE* f = fopen(path, "w");
  if (!f) return;
  fprintf(f, "VBTPLAN2 %d\n", (int)m->groups.size());
  for (const Group& g : m->groups) {
    const Alt& a = g.alts[g.chosen];
    fprintf(f, "%d %d", g.chosen, (int)a.steps.size());
    for (const Step& st : a.steps) fprintf(f, " %s:%d", kFamilyName[st.family], st.variant);
    fprintf(f, "\n");
  }
  fclose(f);
}

static int enqueue_forward(vbt_model* m, const uint8_t* frames_dev, int B, hipStream_t st, float* boxes, float* scores,
                           float* classes, int* counts, hipEvent_t* evs) {
  const int nsub = (!evs && m->n_sub > 1 && B >= 2 * m->n_sub) ? m->n_sub : 1;
  if (nsub == 1) {
    int i = 0;
    for (const Step& s : m->steps) {
      if (evs) (void)hipEventRecord(evs[i], st);
      int rc = launch_step(m, s, B, st, frames_dev, boxes, scores, classes, counts);
      if (rc) return rc;
      i++;
    }
    if (evs) (void)hipEventRecord(evs[i], st);
  } else {
    // Independent sub-batches on side streams: the many small, latency-bound kernels of one sub-batch overlap
    // with the other's.  Fork from / join into the caller's stream with events.
    (void)hipEventRecord(m->ev_fork, st);
    const int per = (B + nsub - 1) / nsub;
    for (int k = 0; k < nsub; k++) {
      const int b0 = k * per, bk = std::min(per, B - b0);
      if (bk <= 0) break;
      hipStream_t ss = m->sub_streams[k];
      (void)hipStreamWaitEvent(ss, m->ev_fork, 0);
      for (const Step& s : m->steps) {
        int rc = launch_step(m, s, bk, ss, frames_dev + (size_t)b0 * m->hdr.image_size * m->hdr.image_size * 3, boxes, scores, classes, counts, b0);
        if (rc) return rc;
      }
      (void)hipEventRecord(m->ev_join[k], ss);
      (void)hipStreamWaitEvent(st, m->ev_join[k], 0);
    }
  }
  VBT_HIP_CHECK(hipGetLastError());
  m->last_B = B;
  return VBT_OK;
}

// The network entry: the plan steps up to and including the last one that reads the frames (the stem convolution, alone or fused with
// block 0 - the first plan group of the pinned plans).  Every tensor behind it is materialised, batch-major, in a buffer of its own.
static int entry_steps(const vbt_model* m) {
  int k = 0;
  for (size_t i = 0; i < m->steps.size(); i++)
    if (m->steps[i].family == F_STEM || m->steps[i].family == F_STEMBLK) k = (int)i + 1;
  return k;
}

// Forward = eager launches, or (small batches: the 120-odd launches are host-bound) replay of a captured hipGraph.
static int forward(vbt_model* m, const uint8_t* frames_dev, int B, hipStream_t st, float* boxes, float* scores, float* classes,
                   int* counts) {
  RoctxRange range("vbt:detect");
  if (m->pool_dirty) { const int rc = flush_uploads(m); if (rc) return rc; }   // (never inside a stream capture)
  if (B > m->graph_max_batch || !m->cap_stream) return enqueue_forward(m, frames_dev, B, st, boxes, scores, classes, counts, nullptr);
  vbt_model::GraphKey key{frames_dev, boxes, scores, classes, counts, B};
  auto it = m->graphs.find(key);
  if (it == m->graphs.end()) {
    if (m->graphs.size() >= 256) {  // bounded cache
      for (auto& kv : m->graphs) (void)hipGraphExecDestroy(kv.second);
      m->graphs.clear();
    }
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    if (!m->ran_eager) {
      // The first forward of a model never runs inside a capture: the per-device LDS opt-ins of its kernels (hipFuncSetAttribute) and any
      // failure they report happen here, eagerly, on the caller's stream (same buffers, same results as the replay that follows).
      const int rc0 = enqueue_forward(m, frames_dev, B, st, boxes, scores, classes, counts, nullptr);
      if (rc0) return rc0;
      m->ran_eager = true;
    }
    VBT_HIP_CHECK(hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeThreadLocal));
    int rc = enqueue_forward(m, frames_dev, B, m->cap_stream, boxes, scores, classes, counts, nullptr);
    hipError_t e = hipStreamEndCapture(m->cap_stream, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) { set_error("hipStreamEndCapture failed: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
    e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) { set_error("hipGraphInstantiate failed: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
    it = m->graphs.emplace(key, ge).first;
  }
  VBT_HIP_CHECK(hipGraphLaunch(it->second, st));
  m->last_B = B;
  return VBT_OK;
}

}  // namespace vbt

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

const char* vbt_last_error(void) { return vbt::g_err; }

int vbt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int vbt_model_create(const char* path, int device, int max_batch, vbt_model** out) {
  const char* nf = getenv("VBT_FUSION_FLAGS");  // bit0: no fusion, bit1: no MBConv fusion, bit2: no SeparableConv fusion
  return vbt_model_create_ex(path, device, max_batch, nf ? atoi(nf) : VBT_MODEL_DEFAULT_FLAGS, out);
}

int vbt_model_tensor_materialized(const vbt_model* m, int id) {
  if (!m || id < 0 || id >= (int)m->tensors.size()) { set_error("bad tensor id"); return VBT_ERR_ARG; }
  return m->materialized[id] ? 1 : 0;
}

int vbt_model_num_launches(const vbt_model* m) { return m ? (int)m->steps.size() : VBT_ERR_ARG; }

int vbt_model_plan_space(const vbt_model* m, vbt_plan_step_space* out, int cap, int* n) {
  if (!m || !n || cap < 0 || (cap > 0 && !out)) { set_error("vbt_model_plan_space: bad argument"); return VBT_ERR_ARG; }
  const PlanShape shape = plan_shape(m);
  int total = 0;
  for (const auto& alts : shape.groups)
    for (const auto& steps : alts) total += (int)steps.size();
  *n = total;
  if (total > cap) { set_error("plan space: %d steps, buffer holds %d", total, cap); return VBT_ERR_CAPACITY; }
  int i = 0;
  for (size_t gi = 0; gi < shape.groups.size(); gi++)
    for (size_t ai = 0; ai < shape.groups[gi].size(); ai++)
      for (size_t si = 0; si < shape.groups[gi][ai].size(); si++, i++) {
        const PlanStepShape& ps = shape.groups[gi][ai][si];
        vbt_plan_step_space& o = out[i];
        memset(&o, 0, sizeof(o));
        if (ps.variants.size() > sizeof(o.variants) / sizeof(o.variants[0])) {
          set_error("plan space: group %zu alternative %zu step %zu has %zu variants", gi, ai, si, ps.variants.size());
          return VBT_ERR_CAPACITY;
        }
        o.group = (int)gi; o.alt = (int)ai; o.step = (int)si;
        o.chosen = m->groups[gi].chosen == (int)ai;
        const Step& st = m->groups[gi].alts[ai].steps[si];
        o.variant = st.variant;
        o.first_op = (int)m->ops.size(); o.last_op = -1;
        std::function<void(const Step&)> span = [&](const Step& s) {
          for (int op : {s.op, s.e_op, s.d_op, s.p_op, s.a_op, s.sum_op})
            if (op >= 0) { o.first_op = std::min(o.first_op, op); o.last_op = std::max(o.last_op, op); }
          for (const Step& mb : s.members) span(mb);
        };
        span(st);
        snprintf(o.family, sizeof(o.family), "%s", ps.family.c_str());
        o.n_variants = (int)ps.variants.size();
        std::copy(ps.variants.begin(), ps.variants.end(), o.variants);
      }
  return VBT_OK;
}

int vbt_model_create_ex(const char* path, int device, int max_batch, int flags, vbt_model** out) {
  if (!path || !out || max_batch < 1) { set_error("vbt_model_create: bad argument"); return VBT_ERR_ARG; }
  *out = nullptr;
  vbt_model* m = new vbt_model();
  {
    // reader + structural validation (container_parse.h): every index the planner and the kernels follow is in range before they see it
    ContainerData cd;
    std::string why;
    if (!read_container(path, &cd, &why)) { delete m; set_error("%s", why.c_str()); return VBT_ERR_IO; }
    m->hdr = cd.hdr;
    m->tensors.swap(cd.tensors);
    m->ops.swap(cd.ops);
    m->blob.swap(cd.blob);
  }
  m->device = device;
  m->max_batch = max_batch;
  m->flags = flags;
  if (int drc = use_device("vbt_model_create", device, /*set_current=*/false)) { delete m; return drc; }
  int rc = VBT_OK;
  auto fail = [&](int code) { vbt_model_destroy(m); return code; };
  if (hipSetDevice(device) != hipSuccess) { set_error("hipSetDevice(%d) failed", device); return fail(VBT_ERR_HIP); }
  // activation arena: every graph tensor keeps its own [max_batch][h][w][c] int8 buffer
  size_t total = 0;
  m->telems.resize(m->tensors.size());
  std::vector<size_t> off(m->tensors.size());
  for (size_t i = 0; i < m->tensors.size(); i++) {
    const TensorRec& t = m->tensors[i];
    m->telems[i] = (size_t)t.h * t.w * t.c;
    off[i] = total;
    size_t bytes = (int)i == m->hdr.input_tensor ? 0 : m->telems[i] * max_batch;
    total += (bytes + 255) / 256 * 256 + 256;
  }
  if (fenced_malloc(m, (void**)&m->arena, total + 4096) != hipSuccess) { set_error("hipMalloc(%zu) for activations failed", total); return fail(VBT_ERR_HIP); }
  (void)hipMemset(m->arena, 0, total + 4096);
  m->tptr.resize(m->tensors.size());
  for (size_t i = 0; i < m->tensors.size(); i++) m->tptr[i] = m->arena + off[i];
  size_t fbytes = (size_t)max_batch * m->hdr.image_size * m->hdr.image_size * 3;
  const int md = m->hdr.max_detections;
  m->out_bytes = (size_t)max_batch * (md * 24 + 4);
  if (fenced_malloc(m, (void**)&m->frames_stage, fbytes + 64) != hipSuccess || hipMalloc((void**)&m->out_boxes, m->out_bytes) != hipSuccess ||
      hipHostMalloc((void**)&m->out_host, m->out_bytes, hipHostMallocDefault) != hipSuccess) {
    set_error("hipMalloc for staging buffers failed");
    return fail(VBT_ERR_HIP);
  }
  m->out_scores = m->out_boxes + (size_t)max_batch * md * 4;
  m->out_classes = m->out_scores + (size_t)max_batch * md;
  m->out_counts = (int*)(m->out_classes + (size_t)max_batch * md);
  if ((rc = build_plan(m)) != VBT_OK) return fail(rc);
  for (const OpRec& op : m->ops)
    if (op.type == OP_POSTPROCESS) {
      std::vector<float> an((const float*)(m->blob.data() + op.aux_off), (const float*)(m->blob.data() + op.aux_off) + (size_t)m->hdr.num_anchors * 4);
      if ((size_t)op.aux2_off + VBT_POST_TABLE_BYTES > m->blob.size()) { set_error("post-process tables truncated"); return fail(VBT_ERR_IO); }
      std::vector<unsigned char> lut(m->blob.data() + op.aux2_off, m->blob.data() + op.aux2_off + VBT_POST_TABLE_BYTES);
      const float* sv = (const float*)(lut.data() + 6144);
      if (sv[0] != sv[1] || sv[2] != sv[3]) { set_error("post-process: y_scale != x_scale or h_scale != w_scale"); return fail(VBT_ERR_ARG); }
      {
        // The stored tables are checked, not trusted: every entry is derived again from the quantisation of the class and
        // box tensors (XNNPACK's x8 LOGISTIC table in float32 with glibc expf; DEQUANTIZE as one float32 product; the
        // decode's divisions and exp() in double, detection_postprocess.cc) and a container that differs is refused.
        const int nl = op.n_inputs / 2;
        const TensorRec& tc = m->tensors[op.inputs[0]];
        const TensorRec& tb = m->tensors[op.inputs[nl]];
        for (int l = 1; l < nl; l++) {   // CONCATENATION: one quantisation for all of its inputs
          const TensorRec &c2 = m->tensors[op.inputs[l]], &b2 = m->tensors[op.inputs[nl + l]];
          if (c2.scale != tc.scale || c2.zero_point != tc.zero_point || b2.scale != tb.scale || b2.zero_point != tb.zero_point) {
            set_error("post-process: head outputs of level %d are quantised differently from level 0", l);
            return fail(VBT_ERR_ARG);
          }
        }
        const float* st_score = (const float*)lut.data();
        const float* st_box = st_score + 256;
        const double* st_dq = (const double*)(lut.data() + 2048);
        const double* st_ex = st_dq + 256;
        for (int q = -128; q < 128; q++) {
          const float x = tc.scale * (float)(q - tc.zero_point);
          float y = 256.0f / (1.0f + expf(-x));
          y = y < 0.0f ? 0.0f : (y > 255.0f ? 255.0f : y);
          const float want_score = (1.0f / 256.0f) * (float)lrintf(y);
          const float want_box = tb.scale * (float)(q - tb.zero_point);
          const double want_dq = (double)want_box / (double)sv[0];
          const double want_ex = exp((double)want_box / (double)sv[2]);
          if (st_score[q + 128] != want_score || st_box[q + 128] != want_box || st_dq[q + 128] != want_dq || st_ex[q + 128] != want_ex) {
            set_error("post-process: stored table entry %d differs from the one derived from the tensor scales", q);
            return fail(VBT_ERR_ARG);
          }
        }
      }
      // device tables: scores re-indexed by rank byte, decode tables, class byte -> rank byte
      std::vector<unsigned char> dev(1024 + 2048 + 2048 + 256, 0);
      const float* score = (const float*)lut.data();
      float* score_by_rank = (float*)dev.data();
      signed char* rank = (signed char*)(dev.data() + 5120);
      for (int q = 1; q < 256; q++)
        if (score[q] < score[q - 1]) { set_error("post-process: score table is not monotone"); return fail(VBT_ERR_ARG); }
      int r = 127;   // highest class byte gets rank 127; a strictly lower score steps the rank down
      for (int q = 255; q >= 0; q--) {
        if (q < 255 && score[q] != score[q + 1]) r--;
        rank[q] = (signed char)r;
        score_by_rank[r + 128] = score[q];
      }
      for (int i = -128; i < r; i++) score_by_rank[i + 128] = -1.0f;   // unused rank bytes: below every threshold
      memcpy(dev.data() + 1024, lut.data() + 2048, 4096);
      if ((rc = upload(m, an, &m->d_anchors)) || (rc = upload(m, dev, &m->d_luts))) return fail(rc);
      m->post_tables_host.assign(score_by_rank, score_by_rank + 256);
    }
  {
    const char* ns = getenv("VBT_SUBSTREAMS");
    int want = ns ? atoi(ns) : 1;  // side streams measured no gain on MI355X at B = 64 (the GPU is busy, not starved)
    if (m->flags & VBT_MODEL_SINGLE_STREAM) want = 1;
    m->n_sub = std::max(1, std::min(want, 4));
    if (max_batch < 2 * m->n_sub) m->n_sub = 1;
    if (m->n_sub > 1) {
      bool ok = hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming) == hipSuccess;
      for (int k = 0; k < m->n_sub && ok; k++)
        ok = hipStreamCreateWithFlags(&m->sub_streams[k], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&m->ev_join[k], hipEventDisableTiming) == hipSuccess;
      if (!ok) { set_error("cannot create side streams"); return fail(VBT_ERR_HIP); }
    }
  }
  {
    const char* gm = getenv("VBT_GRAPH_MAX_BATCH");
    m->graph_max_batch = (m->flags & VBT_MODEL_NO_GRAPH) ? 0 : (gm ? atoi(gm) : 8);
    if (m->graph_max_batch > 0 && hipStreamCreateWithFlags(&m->cap_stream, hipStreamNonBlocking) != hipSuccess) m->cap_stream = nullptr;
  }
  if (!(m->flags & VBT_MODEL_NO_AUTOTUNE)) {
    // VBT_PLAN_FILE: reuse a previously tuned plan (keeps profiled and un-profiled runs on the same kernels)
    const char* pf = getenv("VBT_PLAN_FILE");
    char path[1024];
    if (pf) snprintf(path, sizeof(path), "%s.b%d.f%d", pf, max_batch, m->flags);
    if (!pf || !load_plan(m, path)) {
      autotune(m);
      if (pf) save_plan(m, path);
    } else if (getenv("VBT_PLAN_CONVERT")) {
      save_plan(m, path);       // a format-1 file comes back in format 2 (same choices, kernel families by name)
    }
  }
  finalize_plan(m);
  if ((rc = flush_uploads(m)) != VBT_OK) return fail(rc);
  *out = m;
  return VBT_OK;
}

void vbt_model_destroy(vbt_model* m) {
  if (!m) return;
  for (int k = 0; k < 4; k++) {
    if (m->sub_streams[k]) (void)hipStreamDestroy(m->sub_streams[k]);
    if (m->ev_join[k]) (void)hipEventDestroy(m->ev_join[k]);
  }
  if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
  for (auto& kv : m->graphs) (void)hipGraphExecDestroy(kv.second);
  if (m->cap_stream) (void)hipStreamDestroy(m->cap_stream);
  for (void* p : m->owned) (void)hipFree(p);
  (void)hipFree(m->out_boxes);  // (one block: boxes | scores | classes | counts); arena and frames_stage are in `owned`
  if (m->out_host) (void)hipHostFree(m->out_host);
  delete m;
}

int vbt_model_input_shape(const vbt_model* m, int shape[4]) {
  if (!m || !shape) { set_error("bad argument"); return VBT_ERR_ARG; }
  shape[0] = m->max_batch; shape[1] = m->hdr.image_size; shape[2] = m->hdr.image_size; shape[3] = 3;
  return VBT_OK;
}
int vbt_model_num_tensors(const vbt_model* m) { return m ? (int)m->tensors.size() : VBT_ERR_ARG; }
int vbt_model_num_ops(const vbt_model* m) { return m ? (int)m->ops.size() : VBT_ERR_ARG; }
int vbt_model_tensor_shape(const vbt_model* m, int id, int shape[3]) {
  if (!m || !shape || id < 0 || id >= (int)m->tensors.size()) { set_error("bad tensor id"); return VBT_ERR_ARG; }
  shape[0] = m->tensors[id].h; shape[1] = m->tensors[id].w; shape[2] = m->tensors[id].c;
  return VBT_OK;
}

int vbt_detect_async(vbt_model* m, const uint8_t* frames_dev, int B, void* stream, float* boxes, float* scores, float* classes,
                     int32_t* counts) {
  if (!m || !frames_dev || !boxes || !scores || !classes || !counts) { set_error("vbt_detect_async: NULL argument"); return VBT_ERR_ARG; }
  if (B < 1 || B > m->max_batch) { set_error("vbt_detect: batch %d outside 1..%d", B, m->max_batch); return VBT_ERR_CAPACITY; }
  return forward(m, frames_dev, B, (hipStream_t)stream, boxes, scores, classes, counts);
}

int vbt_model_entry_steps(const vbt_model* m) { return m ? entry_steps(m) : VBT_ERR_ARG; }

int vbt_detect_range_async(vbt_model* m, const uint8_t* frames_dev, int img0, int n_img, int step0, int step1, void* stream, float* boxes,
                           float* scores, float* classes, int32_t* counts) {
  if (!m) { set_error("vbt_detect_range_async: NULL model"); return VBT_ERR_ARG; }
  const int ns = (int)m->steps.size();
  if (step1 < 0) step1 = ns;
  if (img0 < 0 || n_img < 1 || (long)img0 + n_img > m->max_batch) { set_error("vbt_detect_range_async: images %d..%ld outside 0..%d", img0, (long)img0 + n_img - 1, m->max_batch - 1); return VBT_ERR_CAPACITY; }
  if (step0 < 0 || step0 >= step1 || step1 > ns) { set_error("vbt_detect_range_async: steps [%d, %d) outside the plan's %d", step0, step1, ns); return VBT_ERR_ARG; }
  if (step0 < entry_steps(m) && !frames_dev) { set_error("vbt_detect_range_async: the range reads the frames, frames_dev is NULL"); return VBT_ERR_ARG; }
  for (int i = step0; i < step1; i++) {
    const Step& s = m->steps[(size_t)i];
    if (s.family == F_POST && (!boxes || !scores || !classes || !counts)) { set_error("vbt_detect_range_async: the range ends in decode + NMS, an output pointer is NULL"); return VBT_ERR_ARG; }
    // grids of several problems carry whole-batch pointers (launch_step)
    if (img0 != 0 && ((s.family == F_PW && !s.members.empty()) || s.family == F_BAND)) { set_error("vbt_detect_range_async: plan step %d (%s) runs from image 0 only", i, kFamilyName[s.family]); return VBT_ERR_ARG; }
  }
  RoctxRange range("vbt:detect");
  if (m->pool_dirty) { const int rc = flush_uploads(m); if (rc) return rc; }
  for (int i = step0; i < step1; i++) {
    const int rc = launch_step(m, m->steps[(size_t)i], n_img, (hipStream_t)stream, frames_dev, boxes, scores, classes, counts, img0);
    if (rc) return rc;
  }
  VBT_HIP_CHECK(hipGetLastError());
  m->last_B = img0 + n_img;
  return VBT_OK;
}

int vbt_detect(vbt_model* m, const uint8_t* frames, int B, int frames_on_device, void* stream, float* boxes, float* scores,
               float* classes, int32_t* counts, int outputs_on_device) {
  if (!m || !frames || !boxes || !scores || !classes || !counts) { set_error("vbt_detect: NULL argument"); return VBT_ERR_ARG; }
  if (B < 1 || B > m->max_batch) { set_error("vbt_detect: batch %d outside 1..%d", B, m->max_batch); return VBT_ERR_CAPACITY; }
  hipStream_t st = (hipStream_t)stream;
  VBT_HIP_CHECK(hipSetDevice(m->device));
  const uint8_t* fd = frames;
  size_t fbytes = (size_t)B * m->hdr.image_size * m->hdr.image_size * 3;
  if (!frames_on_device) {
    VBT_HIP_CHECK(hipMemcpyAsync(m->frames_stage, frames, fbytes, hipMemcpyHostToDevice, st));
    fd = m->frames_stage;
  }
  float *db = boxes, *ds = scores, *dc = classes;
  int* dn = counts;
  if (!outputs_on_device) { db = m->out_boxes; ds = m->out_scores; dc = m->out_classes; dn = m->out_counts; }
  int rc = forward(m, fd, B, st, db, ds, dc, dn);
  if (rc) return rc;
  if (!outputs_on_device) {
    // one copy of the staging block into its pinned mirror, one synchronisation of this stream, then the caller's arrays are
    // filled on the host (four copies into pageable memory used to be four staged transfers)
    const int md = m->hdr.max_detections;
    const size_t mb = (size_t)m->max_batch;
    const unsigned char* d = (const unsigned char*)m->out_boxes;
    unsigned char* h = m->out_host;
    if (B == m->max_batch) {
      VBT_HIP_CHECK(hipMemcpyAsync(h, d, m->out_bytes, hipMemcpyDeviceToHost, st));
    } else {   // only the B-frame prefix of each of the four tensors (an interpreter created for 256 frames and called with 1 moved 615 KB)
      const size_t off[4] = {0, mb * md * 16, mb * md * 20, mb * md * 24}, len[4] = {(size_t)B * md * 16, (size_t)B * md * 4, (size_t)B * md * 4, (size_t)B * 4};
      for (int i = 0; i < 4; i++) VBT_HIP_CHECK(hipMemcpyAsync(h + off[i], d + off[i], len[i], hipMemcpyDeviceToHost, st));
    }
    VBT_HIP_CHECK(hipStreamSynchronize(st));
    memcpy(boxes, h, (size_t)B * md * 16);
    memcpy(scores, h + mb * md * 16, (size_t)B * md * 4);
    memcpy(classes, h + mb * md * 20, (size_t)B * md * 4);
    memcpy(counts, h + mb * md * 24, (size_t)B * 4);
  }
  return VBT_OK;
}

int vbt_model_read_tensor(vbt_model* m, int id, int B, int8_t* host_out) {
  if (!m || !host_out || id < 0 || id >= (int)m->tensors.size() || id == m->hdr.input_tensor) { set_error("bad tensor id"); return VBT_ERR_ARG; }
  if (B < 1 || B > m->max_batch) { set_error("bad batch"); return VBT_ERR_CAPACITY; }
  if (!m->materialized[id]) { set_error("tensor %d lives only in LDS (fused away); create the model with VBT_MODEL_NO_FUSION to read it", id); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipDeviceSynchronize());
  VBT_HIP_CHECK(hipMemcpy(host_out, m->tptr[id], m->telems[id] * B, hipMemcpyDeviceToHost));
  return VBT_OK;
}

// A HIP stream gets its hardware queue at its FIRST command, round-robin over GPU_MAX_HW_QUEUES (rocprofv3 Queue_Id).  Streams
// drawn from a framework's pool may have been used before, so a pipeline's streams can land on one queue and serialise
// (measured: 89 k -> 58 k frames/s).  Streams created here run one empty launch at once: streams created back to back sit on
// consecutive queues.
__global__ void stream_touch_kernel() {}
int vbt_stream_create(int device, void** stream_out) {
  if (!stream_out) { set_error("vbt_stream_create: NULL argument"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(device));
  hipStream_t st = nullptr;
  VBT_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  stream_touch_kernel<<<1, 64, 0, st>>>();
  hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) { (void)hipStreamDestroy(st); set_error("vbt_stream_create: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
  *stream_out = (void*)st;
  return VBT_OK;
}
// Do two streams share a hardware queue?  A single-wave kernel that spins for `us` microseconds on each: side by side they
// take `us`, on one in-order queue 2 x `us`.  (The queue of a stream cannot be queried; GPU otherwise idle when called.)
__global__ void stream_spin_kernel(long ticks) {
  const long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
int vbt_streams_share_queue(void* a, void* b, int us, int* shared) {
  if (!a || !b || !shared || us < 20 || us > 100000) { set_error("vbt_streams_share_queue: bad argument"); return VBT_ERR_ARG; }
  const long ticks = (long)us * 100;   // wall_clock64: 100 MHz
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)a));
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)b));
  auto t0 = std::chrono::steady_clock::now();
  stream_spin_kernel<<<1, 64, 0, (hipStream_t)a>>>(ticks);
  stream_spin_kernel<<<1, 64, 0, (hipStream_t)b>>>(ticks);
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)a));
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)b));
  const double el = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  *shared = el > 1.6 * us ? 1 : 0;
  return VBT_OK;
}
int vbt_stream_destroy(void* stream) {
  if (!stream) return VBT_OK;
  VBT_HIP_CHECK(hipStreamDestroy((hipStream_t)stream));
  return VBT_OK;
}

}  // extern "C"
namespace vbt {
int resize_frames_dev(const uint8_t* src_dev, int B, int H, int W, uint8_t* dst_dev, int h, int w, int swap_rb, int compact, hipStream_t st) {
  if (compact && H < 2) { set_error("resize: compact rows need a source of at least two rows"); return VBT_ERR_ARG; }
  const long total = (long)B * h * w;
  const float sy = (float)H / (float)h, sx = (float)W / (float)w;
  resize_bilinear_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(src_dev, dst_dev, total, H, W, h, w, sy, sx, swap_rb, compact);
  VBT_HIP_CHECK(hipGetLastError());
  return VBT_OK;
}
}  // namespace vbt
extern "C" {

int vbt_resize_frames(const uint8_t* src, int B, int H, int W, int src_on_device, uint8_t* dst, int h, int w, int dst_on_device,
                      int swap_rb, int device, void* stream) {
  if (!src || !dst || B < 1 || H < 1 || W < 1 || h < 1 || w < 1) { set_error("vbt_resize_frames: bad argument"); return VBT_ERR_ARG; }
  if (int rc = use_device("vbt_resize_frames", device)) return rc;
  hipStream_t st = (hipStream_t)stream;
  size_t sb = (size_t)B * H * W * 3, db = (size_t)B * h * w * 3;
  DevBuf<uint8_t> ds, dd;   // freed when the function returns: after the stream synchronisation, or - on an error - by a hipFree that waits
  const uint8_t* sp = src;
  uint8_t* dp = dst;
  if (!src_on_device) {
    VBT_HIP_CHECK(ds.alloc(sb));
    VBT_HIP_CHECK(hipMemcpyAsync(ds.get(), src, sb, hipMemcpyHostToDevice, st));
    sp = ds.get();
  }
  if (!dst_on_device) {
    VBT_HIP_CHECK(dd.alloc(db));
    dp = dd.get();
  }
  hipError_t e = resize_frames_dev(sp, B, H, W, dp, h, w, swap_rb, 0, st) == VBT_OK ? hipSuccess : hipErrorLaunchFailure;
  if (e == hipSuccess && !dst_on_device) e = hipMemcpyAsync(dst, dd.get(), db, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && (ds || dd)) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { set_error("vbt_resize_frames failed: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
  return VBT_OK;
}

#ifdef VBT_POST_PROF
int vbt_post_prof_read(unsigned long long* out16, int reset) {
  if (reset) { unsigned long long z[16] = {0}; VBT_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(vbt::g_post_prof), z, sizeof(z))); return VBT_OK; }
  VBT_HIP_CHECK(hipDeviceSynchronize());
  VBT_HIP_CHECK(hipMemcpyFromSymbol(out16, HIP_SYMBOL(vbt::g_post_prof), 16 * sizeof(unsigned long long)));
  return VBT_OK;
}
#endif

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
  hipStream_t st = (hipStream_t)stream;
  const int ns = (int)m->steps.size();
  std::vector<hipEvent_t> evs(ns + 1);
  for (auto& e : evs) VBT_HIP_CHECK(hipEventCreate(&e));
  for (int i = 0; i < F_COUNT; i++) ms_out[i] = 0.0;
  int rc = VBT_OK;
  for (int r = 0; r < reps && rc == VBT_OK; r++) {
    rc = enqueue_forward(m, frames_dev, B, st, m->out_boxes, m->out_scores, m->out_classes, m->out_counts, evs.data());
    if (rc) break;
    if (hipStreamSynchronize(st) != hipSuccess) { set_error("stream sync failed"); rc = VBT_ERR_HIP; break; }
    for (int i = 0; i < ns; i++) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, evs[i], evs[i + 1]);
      ms_out[m->steps[i].family] += ms;
    }
  }
  for (auto& e : evs) (void)hipEventDestroy(e);
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
  hipEvent_t e0, e1;
  VBT_HIP_CHECK(hipEventCreate(&e0));
  VBT_HIP_CHECK(hipEventCreate(&e1));
  int rc = VBT_OK;
  for (int f = 0; f < F_COUNT && rc == VBT_OK; f++) {
    ms_out[f] = 0.0;
    bool any = false;
    for (const Step& s : m->steps) any |= s.family == f;
    if (!any) continue;
    for (int pass = 0; pass < 2 && rc == VBT_OK; pass++) {   // pass 0: warm (code objects, caches)
      const int n = pass == 0 ? 1 : reps;
      (void)hipEventRecord(e0, st);
      for (int r = 0; r < n && rc == VBT_OK; r++)
        for (const Step& s : m->steps)
          if (s.family == f && rc == VBT_OK) rc = launch_step(m, s, B, st, m->frames_stage, m->out_boxes, m->out_scores, m->out_classes, m->out_counts);
      (void)hipEventRecord(e1, st);
      if (hipStreamSynchronize(st) != hipSuccess) { set_error("stream sync failed"); rc = VBT_ERR_HIP; break; }
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, e0, e1);
      if (pass == 1) ms_out[f] = (double)ms / reps;
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return rc;
}

// Per-launch timing of the plan (one forward in flight, HIP events around every launch): step i of the execution list ->
// family name, index of the last graph op it covers, kernel variant and milliseconds (average over `reps`).
int vbt_model_profile_steps(vbt_model* m, const uint8_t* frames_dev, int B, int reps, void* stream, vbt_step_time* out, int cap, int* n) {
  if (!m || !frames_dev || !out || !n || reps < 1) { set_error("bad argument"); return VBT_ERR_ARG; }
  if (B < 1 || B > m->max_batch) { set_error("bad batch"); return VBT_ERR_CAPACITY; }
  const int ns = (int)m->steps.size();
  if (cap < ns) { set_error("%d plan steps, buffer holds %d", ns, cap); return VBT_ERR_CAPACITY; }
  hipStream_t st = (hipStream_t)stream;
  std::vector<hipEvent_t> evs(ns + 1);
  for (auto& e : evs) VBT_HIP_CHECK(hipEventCreate(&e));
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
  int rc = VBT_OK;
  for (int r = 0; r < reps && rc == VBT_OK; r++) {
    rc = enqueue_forward(m, frames_dev, B, st, m->out_boxes, m->out_scores, m->out_classes, m->out_counts, evs.data());
    if (rc) break;
    if (hipStreamSynchronize(st) != hipSuccess) { set_error("stream sync failed"); rc = VBT_ERR_HIP; break; }
    for (int i = 0; i < ns; i++) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, evs[i], evs[i + 1]);
      out[i].ms += ms / reps;
    }
  }
  for (auto& e : evs) (void)hipEventDestroy(e);
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
  std::vector<hipStream_t> ss(nstreams, nullptr);
  for (auto& st : ss) VBT_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  int rc = VBT_OK;
  for (int i = 0; i < ns && rc == VBT_OK; i++) {
    const Step& s = m->steps[i];
    for (int pass = 0; pass < 2 && rc == VBT_OK; pass++) {
      const int k = pass == 0 ? 1 : nstreams;
      for (int j = 0; j < k && rc == VBT_OK; j++) rc = launch_step(m, s, B, ss[j], m->frames_stage, m->out_boxes, m->out_scores, m->out_classes, m->out_counts);
      if (rc) break;
      VBT_HIP_CHECK(hipDeviceSynchronize());
      auto t0 = std::chrono::steady_clock::now();
      for (int r = 0; r < reps; r++)
        for (int j = 0; j < k; j++) rc = rc ? rc : launch_step(m, s, B, ss[j], m->frames_stage, m->out_boxes, m->out_scores, m->out_classes, m->out_counts);
      VBT_HIP_CHECK(hipDeviceSynchronize());
      const float ms = (float)(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / (reps * k));
      (pass == 0 ? single_ms : conc_ms)[i] = ms;
    }
  }
  for (auto& st : ss) (void)hipStreamDestroy(st);
  *n = ns;
  return rc;
}

}  // extern "C"
