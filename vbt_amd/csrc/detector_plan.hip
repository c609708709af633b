// The detector's model life cycle and plan selection: the parameter pool the planner uploads into, the plan-time autotuner over the
// variants that resolve (detector.hip), the plan files, model creation / destruction and the shape / count getters of the C ABI.
// Host code only: no kernel is instantiated here.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <functional>
#include <string>

#include "detector_model.h"

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
  const size_t G = 2u << 20;
  const size_t total = fence_on() ? (bytes + G - 1) / G * G : bytes;   // (fence off: the buffer starts its allocation)
  DevBuf<char> base;
  const hipError_t e = base.alloc(total);
  if (e != hipSuccess) return e;
  *out = base.get() + ((total - bytes) & ~(size_t)255);   // keep 256-B alignment; the buffer ends <= 255 B before the fence
  m->owned.push_back(std::move(base));
  return hipSuccess;
}

constexpr size_t POOL_CHUNK = 32u << 20;
static int pool_alloc(vbt_model* m, size_t bytes, void** dev, char** host) {
  bytes = (bytes + 255) & ~(size_t)255;   // 256-byte alignment, like hipMalloc
  if (m->pool.empty() || m->pool.back().used + bytes > m->pool.back().host.size()) {
    vbt_model::PoolChunk c;
    c.used = 0; c.flushed = 0;
    const size_t cap = std::max(POOL_CHUNK, bytes);
    VBT_HIP_CHECK(c.dev.alloc(cap));
    c.host.assign(cap, 0);
    m->pool.push_back(std::move(c));
  }
  vbt_model::PoolChunk& c = m->pool.back();
  *dev = c.dev.get() + c.used;
  *host = c.host.data() + c.used;
  c.used += bytes;
  m->pool_dirty = true;
  return VBT_OK;
}
int flush_uploads(vbt_model* m) {
  if (!m->pool_dirty) return VBT_OK;
  for (auto& c : m->pool)
    if (c.used > c.flushed) {
      VBT_HIP_CHECK(hipMemcpy(c.dev.get() + c.flushed, c.host.data() + c.flushed, c.used - c.flushed, hipMemcpyHostToDevice));
      c.flushed = c.used;
    }
  m->pool_dirty = false;
  return VBT_OK;
}

int upload_bytes(vbt_model* m, const void* src, size_t n, void** d) {
  size_t bytes = std::max<size_t>(n, 16);
  if (fence_on()) {
    VBT_HIP_CHECK(fenced_malloc(m, d, bytes + 64));
    if (n) VBT_HIP_CHECK(hipMemcpy(*d, src, n, hipMemcpyHostToDevice));
    return VBT_OK;
  }
  char* host = nullptr;
  int rc = pool_alloc(m, bytes + 64, d, &host);   // (+64: kernels read K-padding bytes past a weight row's end)
  if (rc) return rc;
  if (n) memcpy(host, src, n);
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
  Event e0, e1;
  if (e0.create(hipEventDefault) != hipSuccess || e1.create(hipEventDefault) != hipSuccess) return 1e30;
  float ms = 1e30f;
  int rc = VBT_OK;   // a refused launch (nothing enqueued) makes the candidate unusable, not fast
  if (nconc <= 1) {
    rc = launch_step_staged(m, s, B, nullptr);
    (void)hipEventRecord(e0.get(), nullptr);
    for (int r = 0; r < reps && !rc; r++)
      rc = launch_step_staged(m, s, B, nullptr);
    (void)hipEventRecord(e1.get(), nullptr);
    if (hipEventSynchronize(e1.get()) != hipSuccess || hipEventElapsedTime(&ms, e0.get(), e1.get()) != hipSuccess) ms = 1e30f;
    ms /= reps;
  } else {
    (void)hipDeviceSynchronize();
    for (int i = 0; i < nconc && !rc; i++)
      rc = launch_step_staged(m, s, B, cs[i]);
    (void)hipDeviceSynchronize();
    auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < reps; r++)
      for (int i = 0; i < nconc && !rc; i++)
        rc = launch_step_staged(m, s, B, cs[i]);
    (void)hipDeviceSynchronize();
    ms = (float)(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / (reps * nconc));
  }
  return rc ? 1e30 : ms;
}

static bool is_fused_tile(int family) { return family == F_MBCONV || family == F_SEPCONV || family == F_NODE; }
// whether `v` resolves to a launch of this step (the depthwise resolver and the families without one take any value)
static bool variant_ok(const vbt_model* m, const Step& st, int v) {
  if (st.family == F_PW) return !st.members.empty() || !resolve_pw(m, st, v, m->max_batch).rc;
  if (is_fused_tile(st.family)) return !resolve_fused(m, st, v, m->max_batch).rc;
  if (st.family == F_BAND) return !resolve_band(m, st, v, m->max_batch).rc;
  if (st.family == F_STEMBLK) return !resolve_stemblk(m, st, v, m->max_batch).rc;
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
    cand = {-1, 2, 3, 4, 5, 6, 7, 8, 9, 10};   // (9 / 10 resolve only where the last output block is part-filled: resolve_pw)
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
      for (int cpw : {1, 2, 3, 4, 6, 9, 18})   // (18 chunks at 6 / 9 / 18: three, two, one workgroup and prologue per image)
        if (cpw <= st.xd.nchunks) {
          if (st.xd2_gpw > 0) cand.push_back(100 + cpw);
          if (st.xd2_gpw16 > 0) cand.push_back(200 + cpw);
          if (st.xd2_small) cand.push_back(300 + cpw);
        }
  } else if (st.family == F_BAND) {
    cand = {-1, 0, 1};   // the launch kind's default, two stages, chained (64-channel maps only)
  } else if (st.family == F_STEMBLK) {
    cand = {-1, 0, 1};   // the default (the im2col form), the im2col form, the direct form
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

}  // namespace vbt

using namespace vbt;

extern "C" {

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
        for_each_named_op(st, [&](int op) { o.first_op = std::min(o.first_op, op); o.last_op = std::max(o.last_op, op); });
        snprintf(o.family, sizeof(o.family), "%s", ps.family.c_str());
        o.n_variants = (int)ps.variants.size();
        std::copy(ps.variants.begin(), ps.variants.end(), o.variants);
      }
  return VBT_OK;
}

int vbt_model_step_proj_tail(const vbt_model* m, int group, int alt, int step) {
  if (!m || group < 0 || group >= (int)m->groups.size() || alt < 0 || alt >= (int)m->groups[group].alts.size() || step < 0 ||
      step >= (int)m->groups[group].alts[alt].steps.size()) { set_error("vbt_model_step_proj_tail: no such step"); return VBT_ERR_ARG; }
  const Step& st = m->groups[group].alts[alt].steps[step];
  if (st.family == F_MBCONV) { const FusedPlan p = resolve_fused(m, st, st.variant, m->max_batch); return p.rc ? 0 : p.L.ntl; }
  if (st.family == F_PW && st.members.empty()) { const PwLaunch L = resolve_pw(m, st, st.variant, m->max_batch); return L.rc ? 0 : L.ntl; }
  return 0;
}

int vbt_model_step_fused_params(const vbt_model* m, int group, int alt, int step) {
  if (!m || group < 0 || group >= (int)m->groups.size() || alt < 0 || alt >= (int)m->groups[group].alts.size() || step < 0 ||
      step >= (int)m->groups[group].alts[alt].steps.size()) { set_error("vbt_model_step_fused_params: no such step"); return VBT_ERR_ARG; }
  const Step& st = m->groups[group].alts[alt].steps[step];
  if (st.family != F_MBCONV) return 0;
  const FusedPlan p = resolve_fused(m, st, st.variant, m->max_batch);
  return !p.rc && !p.image && p.L.params;
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
  if (fenced_malloc(m, (void**)&m->frames_stage, fbytes + 64) != hipSuccess || m->out_block.alloc(m->out_bytes) != hipSuccess ||
      m->out_host.alloc(m->out_bytes) != hipSuccess) {
    set_error("hipMalloc for staging buffers failed");
    return fail(VBT_ERR_HIP);
  }
  m->out_boxes = (float*)m->out_block.get();
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
      // the kernel's arguments, all but the head tensor pointers of a launch (launch_step: F_POST)
      PostArgs& p = m->post;
      p.C = m->hdr.num_classes > 0 ? m->hdr.num_classes : 1;
      p.base[0] = 0;
      for (int l = 0; l < 5; l++) {
        const TensorRec& tl = m->tensors[op.inputs[l]];
        p.base[l + 1] = p.base[l] + tl.h * tl.w * tl.c / p.C;
      }
      p.anchors = m->d_anchors;
      p.tables = m->d_luts;
      p.A = m->hdr.num_anchors;
      p.max_det = m->hdr.max_detections;
      p.iou_thr = m->hdr.nms_iou_threshold;
      p.qmin = 128;   // in rank bytes
      for (int q = 127; q >= -128; q--)
        if (score_by_rank[q + 128] >= m->hdr.nms_score_threshold) p.qmin = q; else break;
      m->post_lds = post_lds_bytes(p.A);
    }
  {
    const char* ns = getenv("VBT_SUBSTREAMS");
    int want = ns ? atoi(ns) : 1;  // side streams measured no gain on MI355X at B = 64 (the GPU is busy, not starved)
    if (m->flags & VBT_MODEL_SINGLE_STREAM) want = 1;
    m->n_sub = std::max(1, std::min(want, 4));
    if (max_batch < 2 * m->n_sub) m->n_sub = 1;
    if (m->n_sub > 1) {
      bool ok = m->ev_fork.create(hipEventDisableTiming) == hipSuccess;
      for (int k = 0; k < m->n_sub && ok; k++)
        ok = m->sub_streams[k].create(hipStreamNonBlocking) == hipSuccess && m->ev_join[k].create(hipEventDisableTiming) == hipSuccess;
      if (!ok) { set_error("cannot create side streams"); return fail(VBT_ERR_HIP); }
    }
  }
  {
    const char* gm = getenv("VBT_GRAPH_MAX_BATCH");
    m->graph_max_batch = (m->flags & VBT_MODEL_NO_GRAPH) ? 0 : (gm ? atoi(gm) : 8);
    if (m->graph_max_batch > 0) (void)m->cap_stream.create(hipStreamNonBlocking);   // (a failure leaves it empty: graphs off)
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
  if (m) delete m;   // (~vbt_model: graph execs, streams and events, then the buffers)
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

}  // extern "C"
