// The planner of the int8 detector: graph ops -> Steps (build_plan), groups of alternative realisations (fuse_plan, batch_heads) and
// the execution list of the chosen ones (finalize_plan, merge_side_convs).  Host code only; the weight layouts are in weight_pack.h.
// A unit of its own: build_plan and finalize_plan are what it exports (detector_model.h, with Step / Group / vbt_model / upload()); the
// tile and LDS geometry it shares with the variant resolvers of detector.hip is in plan_geom.h.  No kernel is instantiated here.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <initializer_list>

#include "detector_model.h"
#include "expdw2_geom.h"   // expdw2_choose
#include "tpz_geom.h"
using vbt::v4i;            // weight_pack.h's functions sit at global scope and take the includer's 16-byte int vector
#include "weight_pack.h"   // the weight / bias layouts of every kernel family: one pure host function each

namespace vbt {

// Rq::kb (dev_common.h): the int32 accumulator of this conv, bias included, stays inside (-2^22, 2^22) for EVERY input.  Whatever way a
// kernel folds the zero point into its bias, the value it requantises is sum_k (x_k - z_x) w_k + b with |x_k - z_x| <= 255, so
// 255 * sum_k |w_k| + |b| bounds it per output channel.  VBT_NO_KBIAS: never (the kernels then convert with v_cvt_f32_i32).
static int conv_kb(const vbt_model* m, const OpRec& op) {
  const bool off = getenv("VBT_NO_KBIAS") != nullptr;   // (read per model: tests build both flavours in one process)
  if (off || (op.type != OP_STEM && op.type != OP_PW && op.type != OP_DW)) return 0;
  const TensorRec& tin = m->tensors[op.inputs[0]];
  const TensorRec& tout = m->tensors[op.output];
  const int8_t* w = (const int8_t*)(m->blob.data() + op.w_off);
  const int32_t* bq = (const int32_t*)(m->blob.data() + op.b_off);
  const bool dw = op.type == OP_DW;
  const int N = tout.c, K = dw ? op.k * op.k : op.k * op.k * tin.c;
  for (int co = 0; co < N; co++) {
    long long sa = 0;
    for (int k = 0; k < K; k++) sa += std::abs((int)(dw ? w[(size_t)k * N + co] : w[(size_t)co * K + k]));
    if (255 * sa + std::llabs((long long)bq[co]) >= (1ll << 22) - 1) return 0;
  }
  return 1;
}

// ---- fusion pass: MBConv (pw+relu6 -> dw -> pw [-> add]) and SeparableConv (dw -> pw) -> fused_block_kernel ----
// (choose_tile, fused_tile_lds and band_lds: plan_geom.h)

// sources of a BiFPN node's sum.  pre_add >= 0: the sum is two chained binary ADDs (3-input sums of a TFLite graph):
// sources 0,1 are the inputs of ops[pre_add], source 2 the other input of the final ADD, chain = 1|2 the position of the
// partial sum among the final ADD's inputs (+1).
struct NodeSrc { int n = 0; int tensor[3]; int mode[3]; int rs_op[3] = {-1, -1, -1}; int pre_add = -1; int chain = 0; };

// accounting = compulsory traffic of the constituent graph ops: the listed ops (-1 = absent) and, for a node, the
// resamples / partial sum it absorbs
static Cost cost_of(const vbt_model* m, std::initializer_list<int> ops, const NodeSrc* ns = nullptr) {
  Cost c;
  for (int oi : ops)
    if (oi >= 0) c += m->op_steps[oi].cost;
  if (ns) c += cost_of(m, {ns->rs_op[0], ns->rs_op[1], ns->rs_op[2], ns->pre_add});
  return c;
}

// the node-sum fields FusedArgs and BandArgs share; where the sources are read from (per launch / whole batch) is the caller's
template <typename Args>
static void fill_node_sources(Args& a, const NodeSrc& ns, const vbt_model* m, int sum_op) {
  a.n_src = ns.n;
  for (int j = 0; j < ns.n; j++) {
    const TensorRec& ts = m->tensors[ns.tensor[j]];
    a.sh[j] = ts.h; a.sw[j] = ts.w; a.smode[j] = ns.mode[j];
    if (ns.mode[j] == 2) { a.spt[j] = m->ops[ns.rs_op[j]].pad_t; a.spl[j] = m->ops[ns.rs_op[j]].pad_l; }
  }
  a.sumq = m->op_steps[sum_op].addq;   // resize / max-pool outputs keep their input's quantisation, so the parameters hold for the absorbed sources
  a.chain = 0;
  if (ns.pre_add >= 0) {   // two chained binary ADDs
    a.chain = ns.chain;
    a.preq = m->op_steps[ns.pre_add].addq;
  }
}

// whole-image kernel (image_block.h): one contiguous record per 64-channel chunk - expand weights | expand bias, multipliers |
// depthwise weights [tap][64] | depthwise bias, multipliers | the chunk's two K steps of every projection block
static int make_image_bundle(vbt_model* m, int e_op, int d_op, int p_op, int KSe, ImageBundle* out) {
  const OpRec &eop = m->ops[e_op], &dop = m->ops[d_op], &pop = m->ops[p_op];
  const TensorRec &tin = m->tensors[eop.inputs[0]], &tdin = m->tensors[dop.inputs[0]], &tout = m->tensors[pop.output];
  const int8_t* we = (const int8_t*)(m->blob.data() + eop.w_off);
  const int8_t* wd = (const int8_t*)(m->blob.data() + dop.w_off);
  const int8_t* wpj = (const int8_t*)(m->blob.data() + pop.w_off);
  const int Ce = tdin.c, Cp = (Ce + 63) / 64 * 64, kk = dop.k * dop.k, NB = (tout.c + 63) / 64, nch = Cp / 64;
  std::vector<long> pe, pp;
  pack_weights(we, Ce, tin.c, KSe, nch, nullptr, pe);
  pack_weights(wpj, tout.c, Ce, Cp / 32, NB, nullptr, pp);
  const std::vector<int> be = fold_bias((const int32_t*)(m->blob.data() + eop.b_off), we, Ce, tin.c, tin.zero_point, W_ROWS, Cp);
  const std::vector<int> bd = fold_bias((const int32_t*)(m->blob.data() + dop.b_off), wd, Ce, kk, tdin.zero_point, W_TAPS, Cp);
  const std::vector<float> me = pad_floats((const float*)(m->blob.data() + eop.m_off), Ce, Cp);
  const std::vector<float> md = pad_floats((const float*)(m->blob.data() + dop.m_off), Ce, Cp);
  ImageBundle ib;
  ib.o_be = KSe * 2048; ib.o_me = ib.o_be + 256; ib.o_dw = ib.o_me + 256;
  ib.o_bd = ib.o_dw + ((kk * 64 + 15) & ~15); ib.o_md = ib.o_bd + 256; ib.o_wp = ib.o_md + 256;
  ib.bytes = ib.o_wp + NB * 4096;
  std::vector<unsigned char> rec((size_t)nch * ib.bytes, 0);
  for (int c = 0; c < nch; c++) {
    unsigned char* R = rec.data() + (size_t)c * ib.bytes;
    memcpy(R, pe.data() + (size_t)c * KSe * 4 * 64, (size_t)KSe * 2048);
    memcpy(R + ib.o_be, &be[64 * c], 256);
    memcpy(R + ib.o_me, &me[64 * c], 256);
    memcpy(R + ib.o_bd, &bd[64 * c], 256);
    memcpy(R + ib.o_md, &md[64 * c], 256);
    for (int t = 0; t < kk; t++)
      for (int i = 0; i < 64 && 64 * c + i < Ce; i++) R[ib.o_dw + t * 64 + i] = (unsigned char)wd[(size_t)t * Ce + 64 * c + i];
    for (int nb = 0; nb < NB; nb++)
      for (int k2 = 0; k2 < 2; k2++)
        memcpy(R + ib.o_wp + (size_t)((nb * 2 + k2) * 4) * 512, pp.data() + ((size_t)(nb * (Cp / 32) + 2 * c + k2) * 4) * 64, 4 * 512);
  }
  unsigned char* drec;
  int rc;
  if ((rc = upload(m, rec, &drec))) return rc;
  ib.data = drec;
  *out = ib;
  return VBT_OK;
}

// Per-chunk parameter blocks of an MBConv step (fused_block.h: PLDS; pack_fused_chunk_params): one block for every (chunking, depthwise
// form, panel layout) whose launch is built with the parameters in LDS (fused_params_built) - each from the host images of the arrays the
// other kernel form reads, packed once more by the same packers.  s.fa holds the step's device arrays already: a null pointer there
// means the step has no such array, and no block is made for it.
static int make_fused_params(vbt_model* m, int e_op, int d_op, int p_op, Step* sp) {
  Step& s = *sp;
  const FusedArgs& a = s.fa;
  const OpRec &eop = m->ops[e_op], &dop = m->ops[d_op], &pop = m->ops[p_op];
  const TensorRec &tin = m->tensors[eop.inputs[0]], &tdin = m->tensors[dop.inputs[0]], &tdout = m->tensors[dop.output], &tout = m->tensors[pop.output];
  const int8_t* we = (const int8_t*)(m->blob.data() + eop.w_off);
  const int8_t* wd = (const int8_t*)(m->blob.data() + dop.w_off);
  const int8_t* wpj = (const int8_t*)(m->blob.data() + pop.w_off);
  const int Ce = tdin.c, Cp = (Ce + 63) / 64 * 64, kk = dop.k * dop.k, k = dop.k, S = dop.stride;
  if (!(a.KSe == 1 || a.KSe == 2) || s.nbp > 2 || !(k == 3 || k == 5)) return VBT_OK;
  const std::vector<int> be = fold_bias((const int32_t*)(m->blob.data() + eop.b_off), we, Ce, tin.c, tin.zero_point, W_ROWS, Cp);
  const std::vector<float> me = pad_floats((const float*)(m->blob.data() + eop.m_off), Ce, Cp);
  const std::vector<int> bdm = fold_bias((const int32_t*)(m->blob.data() + dop.b_off), wd, Ce, kk, tdin.zero_point, W_TAPS, Cp);
  const std::vector<float> md = pad_floats((const float*)(m->blob.data() + dop.m_off), Ce, Cp);
  const std::vector<int> bp = fold_bias((const int32_t*)(m->blob.data() + pop.b_off), wpj, tout.c, Ce, tdout.zero_point, W_ROWS, s.nbp * 64);
  const std::vector<float> mp = pad_floats((const float*)(m->blob.data() + pop.m_off), tout.c, s.nbp * 64);
  for (int nt3 = 0; nt3 < 2; nt3++) {
    if (nt3 && !a.nch3) continue;
    const int NT = nt3 ? 3 : 4, nch = nt3 ? a.nch3 : a.nchunks;
    std::vector<long> wex;
    if (nt3) wex = pack_expand48(we, Ce, tin.c, a.KSe);
    else pack_weights(we, Ce, tin.c, a.KSe, nch, nullptr, wex);
    const std::vector<int> kmap = nt3 ? kmap48(Ce) : std::vector<int>();
    for (int form = 0; form < 3; form++) {
      FusedLaunch L{k, S, s.nbp, true, true, bool(nt3), false, form != FPF_MATRIX, 0, 0, form == FPF_TOEPLITZ};
      if (form == FPF_TOEPLITZ ? !a.wtz : form == FPF_DIAG64 ? !a.wd64c : false) continue;
      std::vector<long> dwl;
      std::vector<unsigned> dwt;
      for (int tail = 0; tail < 2; tail++) {
        if (tail && !(nt3 ? a.wpt3 : a.wpt)) continue;
        const int ntl = tail ? s.ntl : 0;
        FusedLaunch L2 = L;   // (8 x 8 and 16 x 8 tiles read the same block: the predicate is asked for either tile)
        L2.ppw2 = true;
        if (!fused_params_built(L, a.KSe, ntl) && !fused_params_built(L2, a.KSe, ntl)) continue;
        if (dwl.empty() && dwt.empty()) {
          if (form == FPF_DIAG64) dwl = pack_dw64_compact(pack_dw64(wd, Ce, k, Cp / 16), k);
          else if (form == FPF_TOEPLITZ) dwt = pack_expdw2_taps(wd, Ce, 0, Cp / 4, k, S);
          else dwl = pack_dw_diag(wd, Ce, kk, nt3 ? 48 : 64);
        }
        std::vector<v4i> panel;
        if (tail) pack_weights64_tail(wpj, tout.c, Ce, nch, s.nbp, panel, nt3 ? &kmap : nullptr);
        else pack_weights64(wpj, tout.c, Ce, nch, s.nbp, panel, nt3 ? &kmap : nullptr);
        const FusedParamsGeom g = fused_params_geom(NT, a.KSe, form, k, S, s.nbp, ntl);
        const FusedParamsSrc src{wex.data(), be.data(), me.data(), form == FPF_TOEPLITZ ? (const void*)dwt.data() : (const void*)dwl.data(), bdm.data(), md.data(),
                                 panel.data(), nch, bp.data(), mp.data()};
        unsigned char* dev;
        int rc;
        if ((rc = upload(m, pack_fused_chunk_params(g, NT, s.nbp, ntl, nch, src), &dev))) return rc;
        s.cpar[nt3][form][tail] = dev;
      }
    }
  }
  return VBT_OK;
}

static int make_fused(vbt_model* m, int e_op, int d_op, int p_op, int a_op, Step* out, int sum_op = -1, const NodeSrc* ns = nullptr) {
  const OpRec& dop = m->ops[d_op];
  const OpRec& pop = m->ops[p_op];
  const bool expand = e_op >= 0;
  const int in_t = expand ? m->ops[e_op].inputs[0] : dop.inputs[0];
  const TensorRec& tin = m->tensors[in_t];
  const TensorRec& tdin = m->tensors[dop.inputs[0]];
  const TensorRec& tdout = m->tensors[dop.output];
  const TensorRec& tout = m->tensors[pop.output];
  const int Ce = tdin.c, Cp = (Ce + 63) / 64 * 64, kk = dop.k * dop.k;
  const int8_t* wd = (const int8_t*)(m->blob.data() + dop.w_off);
  const int32_t* bqd = (const int32_t*)(m->blob.data() + dop.b_off);
  const int8_t* wpj = (const int8_t*)(m->blob.data() + pop.w_off);
  int rc;
  Step s;
  s.family = expand ? F_MBCONV : (sum_op >= 0 ? F_NODE : F_SEPCONV);
  s.sum_op = sum_op;
  s.op = a_op >= 0 ? a_op : p_op;  // the op whose output this step writes
  s.e_op = e_op; s.d_op = d_op; s.p_op = p_op; s.a_op = a_op;
  FusedArgs& a = s.fa;
  memset(&a, 0, sizeof(a));
  a.H = tin.h; a.W = tin.w; a.Cin = tin.c; a.OH = tout.h; a.OW = tout.w; a.Cout = tout.c;
  a.pad_t = dop.pad_t; a.pad_l = dop.pad_l;
  choose_tile(tout.h, tout.w, dop.k, dop.stride, expand, &a.TX, &a.TY);
  a.tiles_x = (tout.w + a.TX - 1) / a.TX;
  a.tiles_y = (tout.h + a.TY - 1) / a.TY;
  a.nchunks = Cp / 64;
  a.zx = tin.zero_point;
  const Step& ps = m->op_steps[p_op];
  // the kernel instantiation covers nbp = {1,2,3,5} projection blocks and reads the weights of all of them: allocate (zero rows)
  // up to nbp, otherwise a 4-block layer (e.g. Cout = 208 in Lite2) reads past the packed array
  s.nbp = ps.NB <= 3 ? ps.NB : 5;
  if (expand) {
    const Step& es = m->op_steps[e_op];
    const OpRec& eop = m->ops[e_op];
    a.we = es.wp; a.be = es.bias; a.me = es.mult; a.KSe = es.KS;
    a.ze = tdin.zero_point; a.loe = eop.act_min; a.hie = eop.act_max;
    a.rqe = make_rq(a.ze, a.loe, a.hie, conv_kb(m, eop));
    // input tile rows hold the real channels (8-byte granules) + 8 bytes of bank spread, not the K padding of the expand
    // (KS * 32): the B-operand reads of the padded K steps run into the next pixel's bytes, which meet zero weights (the
    // last pixel's run into the E tile).  b1: 40 -> 24 bytes, b4 / b5: 72 -> 48 - LDS per workgroup sets the occupancy here.
    a.T0S = ((tin.c + 7) & ~7) + 8;
  } else {
    a.T0S = Cp + 16;
  }
  {  // depthwise parameters padded to Cp channels: the VALU form (accumulates u = x_q + 128), then the matrix-pipe forms
    float* dwf; int* dbias; float* dmult;
    if ((rc = upload(m, dw_weights_f32(wd, Ce, kk, Cp), &dwf)) || (rc = upload(m, fold_bias(bqd, wd, Ce, kk, 128 + tdin.zero_point, W_TAPS, Cp), &dbias)) ||
        (rc = upload(m, pad_floats((const float*)(m->blob.data() + dop.m_off), Ce, Cp), &dmult)))
      return rc;
    a.wd = dwf; a.bd = dbias; a.md = dmult;
    long* dwdm; int* dbm;
    if ((rc = upload(m, pack_dw_diag(wd, Ce, kk, 64), &dwdm)) || (rc = upload(m, fold_bias(bqd, wd, Ce, kk, tdin.zero_point, W_TAPS, Cp), &dbm))) return rc;
    a.wdm = dwdm; a.bdm = dbm;
    if (expand && (dop.k == 3 || dop.k == 5)) {   // 16x16x64 form (FusedArgs::wd64) and its one-byte-per-operand copy
      const std::vector<v4i> w64 = pack_dw64(wd, Ce, dop.k, Cp / 16);
      v4i* d64; long* d64c;
      if ((rc = upload(m, w64, &d64)) || (rc = upload(m, pack_dw64_compact(w64, dop.k), &d64c))) return rc;
      a.wd64 = d64; a.wd64c = d64c;
      if (fused_tpz_built(dop.k, dop.stride, s.nbp, a.KSe, false)) {   // band-Toeplitz form of the same stage: taps of all Cp / 4 quads
        unsigned* dtz;
        if ((rc = upload(m, pack_expdw2_taps(wd, Ce, 0, Cp / 4, dop.k, dop.stride), &dtz))) return rc;
        a.wtz = dtz;
      }
    }
    a.zd = tdout.zero_point; a.lod = dop.act_min; a.hid = dop.act_max;
    a.rqd = make_rq(a.zd, a.lod, a.hid, conv_kb(m, dop));
  }
  {  // project weights re-packed with K padded to Cp
    std::vector<v4i> wp;
    pack_weights64(wpj, tout.c, Ce, Cp / 64, s.nbp, wp);
    v4i* dwp;
    if ((rc = upload(m, wp, &dwp))) return rc;
    a.wp = dwp; a.bp = ps.bias; a.mp = ps.mult; a.KSp = Cp / 64;
    // MBConv with a part-filled last projection block: both panels once more with that block tile-major (the kernels built with a
    // live-tile count, fused_tail_built; resolve_fused decides per launch)
    if (expand && tout.c % 64 != 0 && tout.c % 4 == 0 && s.nbp == (tout.c + 63) / 64) {
      pack_weights64_tail(wpj, tout.c, Ce, Cp / 64, s.nbp, wp);
      if ((rc = upload(m, wp, &dwp))) return rc;
      a.wpt = dwp;
      s.ntl = proj_tail_tiles(tout.c);
    }
    if (expand)
      for (int i = 0; i < d_op; i++) s.block += m->ops[i].type == OP_DW;   // b1 = the block of the graph's second depthwise conv
    a.zo = tout.zero_point; a.lop = pop.act_min; a.hip = pop.act_max;
    a.rqp = make_rq(a.zo, a.lop, a.hip);
  }
  if (a_op >= 0) {   // fuse_plan guarantees inputs = (project output, block input)
    a.has_res = 1;
    a.resq = m->op_steps[a_op].addq;
  }
  if (sum_op >= 0) {
    fill_node_sources(a, *ns, m, sum_op);
    for (int j = 0; j < ns->n; j++) s.src_tensor[j] = ns->tensor[j];   // (the launch passes this sub-batch's pointers)
  }
  s.lds_bytes = fused_tile_lds(a, dop.k, dop.stride, a.TX, a.TY, expand ? FB_EST : 0, 1, s.nbp);
  s.cost = cost_of(m, {e_op, d_op, p_op, a_op, sum_op}, ns);
  if (expand && Ce % 48 == 0 && Ce % 64 != 0) {
    // 48-channel chunking of the same block (fused_block.h, template NT = 3): no padded channels
    const int8_t* we = (const int8_t*)(m->blob.data() + m->ops[e_op].w_off);
    const int nch3 = Ce / 48;
    const std::vector<int> kmap = kmap48(Ce);
    std::vector<v4i> wp3;
    pack_weights64(wpj, tout.c, Ce, nch3, s.nbp, wp3, &kmap);
    long *d1, *d2;
    v4i* d3;
    if ((rc = upload(m, pack_expand48(we, Ce, tin.c, a.KSe), &d1)) || (rc = upload(m, pack_dw_diag(wd, Ce, kk, 48), &d2)) || (rc = upload(m, wp3, &d3))) return rc;
    a.we3 = d1; a.wdm3 = d2; a.wp3 = d3; a.nch3 = nch3; a.KSp3 = nch3;
    if (s.ntl) {
      pack_weights64_tail(wpj, tout.c, Ce, nch3, s.nbp, wp3, &kmap);
      if ((rc = upload(m, wp3, &d3))) return rc;
      a.wpt3 = d3;
    }
  }
  if (expand && (rc = make_fused_params(m, e_op, d_op, p_op, &s))) return rc;
  if (expand && tin.h * tin.w <= 400 && tout.h * tout.w <= 400 && (rc = make_image_bundle(m, e_op, d_op, p_op, a.KSe, &s.ib))) return rc;
  *out = s;
  return VBT_OK;
}

// the alternative of a group that runs it as ONE tile-kernel launch (fused_block.h), or nullptr
static const Alt* tile_alt(const Group& g, int family) {
  for (int i = (int)g.alts.size() - 1; i >= 0; i--)
    if (g.alts[i].steps.size() == 1 && g.alts[i].steps[0].family == family) return &g.alts[i];
  return nullptr;
}
static const Alt* band_alt(const Group& g) {
  for (int i = (int)g.alts.size() - 1; i >= 0; i--)
    if (g.alts[i].steps.size() == 1 && g.alts[i].steps[0].family == F_BAND && g.alts[i].steps[0].members.empty()) return &g.alts[i];
  return nullptr;
}

// ---- SeparableConv / BiFPN node on row bands (band_block.h) ----
static bool band_ok(const vbt_model* m, int d_op, int p_op) {
  if (m->flags & VBT_MODEL_NO_BAND) return false;
  if (const char* ns = getenv("VBT_SUBSTREAMS")) if (atoi(ns) > 1) return false;   // the problem list holds whole-batch pointers
  const OpRec& d = m->ops[d_op];
  const OpRec& p = m->ops[p_op];
  const TensorRec& ti = m->tensors[d.inputs[0]];
  const TensorRec& to = m->tensors[p.output];
  return d.k == 3 && d.stride == 1 && d.pad_t == 1 && d.pad_l == 1 && ti.c % 8 == 0 && ti.c >= 16 && ti.c <= 128 && to.c <= 128 && to.h == ti.h &&
         to.w == ti.w && ti.w <= 160;
}
static int make_band(vbt_model* m, int d_op, int p_op, int sum_op, const NodeSrc* ns, Step* out) {
  const OpRec& dop = m->ops[d_op];
  const OpRec& pop = m->ops[p_op];
  const TensorRec& tin = m->tensors[dop.inputs[0]];
  const TensorRec& td = m->tensors[dop.output];
  const TensorRec& to = m->tensors[pop.output];
  Step s;
  s.family = F_BAND;
  s.op = p_op;
  s.d_op = d_op;
  s.p_op = p_op;
  s.sum_op = sum_op;
  BandArgs& a = s.bd_args;
  memset(&a, 0, sizeof(a));
  a.H = tin.h; a.W = tin.w; a.Cout = to.c;
  const int C = tin.c;
  a.C = C;
  a.CS = ((C + 15) / 16 | 1) * 16;
  a.NCG = (C + 15) / 16;
  a.KS = (C + 63) / 64;
  // pixels per band: 320 fills a workgroup's sixteen waves with units (a batch of 64 brings enough bands to fill the GPU); a small
  // batch leaves most CUs idle, so there a map is cut into more, shorter bands (latency of one band ~ its pixel groups per wave)
  static const int band_px_env = getenv("VBT_BAND_PX") ? atoi(getenv("VBT_BAND_PX")) : 0;
  const int band_px = band_px_env > 0 ? band_px_env : (m->max_batch <= 8 ? 64 : 320);   // (batch 1 / 8, four forwards in flight: 64 px +3-5 % over 320, tools/band_px_sweep.sh)
  const int nb = std::max(1, (tin.h * tin.w + band_px - 1) / band_px);
  a.rows = (tin.h + nb - 1) / nb;
  a.nbands = (tin.h + a.rows - 1) / a.rows;
  a.zx4 = (unsigned)(tin.zero_point & 255) * 0x01010101u;
  const int8_t* wd = (const int8_t*)(m->blob.data() + dop.w_off);
  v4i *dpd, *dpp, *dpc = nullptr;
  int* dbd;
  float* dmd;
  int rc;
  if ((rc = upload(m, pack_band_dw(wd, C), &dpd)) || (rc = upload(m, pack_band_pw((const int8_t*)(m->blob.data() + pop.w_off), to.c, C), &dpp)) ||
      (rc = upload(m, fold_bias((const int32_t*)(m->blob.data() + dop.b_off), wd, C, 9, tin.zero_point, W_TAPS, a.NCG * 16), &dbd)) ||
      (rc = upload(m, pad_floats((const float*)(m->blob.data() + dop.m_off), C, a.NCG * 16), &dmd)))
    return rc;
  // the chained form's panel beside the natural-order one: both forms stay launchable (detector.hip: resolve_band)
  unsigned* dpdc = nullptr;
  if (C == 64 && to.c <= 64 && ((rc = upload(m, pack_band_pw_chain((const int8_t*)(m->blob.data() + pop.w_off), to.c, C), &dpc)) ||
                                (rc = upload(m, pack_band_dw_compact(wd, C), &dpdc))))
    return rc;
  a.wd = dpd; a.wdc = dpdc; a.wp = dpp; a.wpc = dpc; a.bd = dbd; a.md = dmd;
  a.bp = m->op_steps[p_op].bias;   // folded with the depthwise output's zero point, padded to 64
  a.mp = m->op_steps[p_op].mult;
  a.rqd = make_rq(td.zero_point, dop.act_min, dop.act_max, conv_kb(m, dop));
  a.rqp = make_rq(to.zero_point, pop.act_min, pop.act_max, conv_kb(m, pop));
  a.x = m->tptr[dop.inputs[0]];
  a.out = m->tptr[pop.output];
  if (sum_op >= 0) {
    fill_node_sources(a, *ns, m, sum_op);
    a.x = nullptr;
    for (int j = 0; j < ns->n; j++) a.src[j] = m->tptr[ns->tensor[j]];   // (the problem list holds whole-batch pointers)
  }
  s.band_tiles = a.nbands;
  s.lds_bytes = band_lds(a);
  std::vector<BandArgs> one{a};
  if ((rc = upload(m, one, &s.d_band))) return rc;
  s.cost = cost_of(m, {d_op, p_op, sum_op}, ns);
  *out = s;
  return VBT_OK;
}

// The box / class heads run the same SeparableConv chain on 5 pyramid levels (x 2 heads): layer j of every
// chain is independent of layer j of the others, so all of them go out as ONE grid (fused_block_multi_kernel).
static int batch_heads(vbt_model* m) {
  struct Info { int gi, chain, depth; };
  std::vector<Info> heads;
  std::map<int, std::pair<int, int>> by_tensor;  // output tensor -> (chain, depth)
  int nchains = 0, first = -1;
  for (int gi = 0; gi < (int)m->groups.size(); gi++) {
    const Group& g = m->groups[gi];
    const Alt* fap = tile_alt(g, F_SEPCONV);
    if (!fap) continue;
    const Step& st = fap->steps[0];
    if (m->ops[st.d_op].level < 0) continue;
    int tin = m->ops[st.d_op].inputs[0], tout = m->ops[st.p_op].output;
    auto it = by_tensor.find(tin);
    int chain = it == by_tensor.end() ? nchains++ : it->second.first;
    int depth = it == by_tensor.end() ? 0 : it->second.second + 1;
    by_tensor[tout] = {chain, depth};
    heads.push_back({gi, chain, depth});
    if (first < 0) first = gi;
  }
  if (heads.size() < 2) return VBT_OK;
  int maxd = 0;
  for (auto& h : heads) maxd = std::max(maxd, h.depth);
  // Depth d may only be merged if every deeper layer is merged too: an unmerged successor sits right behind its
  // own predecessor in list order, i.e. ahead of the merged launch that would produce its input.
  auto members_of = [&](int d) {
    std::vector<int> mem;
    for (auto& h : heads)
      if (h.depth == d) mem.push_back(h.gi);
    return mem;
  };
  auto mergeable = [&](const std::vector<int>& mem) {
    if (mem.size() < 2 || mem.size() > 12) return false;
    const Step& s0 = tile_alt(m->groups[mem[0]], F_SEPCONV)->steps[0];
    if (!((s0.nbp == 1 || s0.nbp == 2) && m->ops[s0.d_op].k == 3 && m->ops[s0.d_op].stride == 1)) return false;  // the instantiations built below
    for (int gi : mem) {
      const Step& st = tile_alt(m->groups[gi], F_SEPCONV)->steps[0];
      if (st.nbp != s0.nbp || m->ops[st.d_op].k != 3 || m->ops[st.d_op].stride != 1) return false;
    }
    return true;
  };
  int d0 = maxd + 1;
  while (d0 > 0 && mergeable(members_of(d0 - 1))) d0--;
  if (d0 > maxd) return VBT_OK;
  std::map<int, Group> at;  // position (index of the last member) -> merged group
  std::vector<char> consumed(m->groups.size(), 0);
  for (int d = d0; d <= maxd; d++) {
    std::vector<int> mem = members_of(d);
    const Step& s0 = tile_alt(m->groups[mem[0]], F_SEPCONV)->steps[0];
    Group g;
    Alt unf, each, multi, bandm;
    Step ms, bs;
    bs.family = F_BAND;
    bs.op = s0.op;
    bs.d_op = s0.d_op;
    std::vector<BandArgs> bargs;
    bool all_band = true;
    ms.family = F_MULTI;
    ms.op = s0.op;
    ms.d_op = s0.d_op;
    ms.nbp = s0.nbp;
    std::vector<FusedArgs> hargs;
    int last = 0;
    for (int gi : mem) {
      const Group& src = m->groups[gi];
      for (const Step& st : src.alts[0].steps) unf.steps.push_back(st);
      const Alt* ta = tile_alt(src, F_SEPCONV);
      const Step& fs = ta->steps[0];
      each.steps.push_back(fs);
      for (int t : ta->hidden) { each.hidden.push_back(t); multi.hidden.push_back(t); bandm.hidden.push_back(t); }
      const Alt* ba = band_alt(src);
      if (ba && ba->steps[0].bd_args.n_src == 0) {   // (the multi-problem band kernels are built without the node-sum path)
        Step b1 = ba->steps[0];
        {   // the head grid runs 8-wave workgroups on shorter bands (band_block.h)
          BandArgs& ha = b1.bd_args;
          const int nbh = std::max(1, (ha.H * ha.W + BD_HEAD_MAXPX - 1) / BD_HEAD_MAXPX);
          ha.rows = (ha.H + nbh - 1) / nbh;
          ha.nbands = (ha.H + ha.rows - 1) / ha.rows;
          b1.band_tiles = ha.nbands;
          b1.lds_bytes = band_lds(ha);
        }
        bs.members.push_back(b1);
        bargs.push_back(b1.bd_args);
        bs.lds_bytes = std::max(bs.lds_bytes, b1.lds_bytes);
        bs.cost += b1.cost;
      } else {
        all_band = false;
      }
      ms.members.push_back(fs);
      ms.lds_bytes = std::max(ms.lds_bytes, fs.lds_bytes);
      ms.cost += fs.cost;
      FusedArgs a = fs.fa;
      a.x = m->tptr[m->ops[fs.d_op].inputs[0]];
      a.out = m->tptr[m->ops[fs.op].output];
      hargs.push_back(a);
      consumed[gi] = 1;
      last = std::max(last, gi);
    }
    int rc = upload(m, hargs, &ms.d_multi);
    if (rc) return rc;
    multi.steps.push_back(ms);
    g.alts.push_back(unf);
    g.alts.push_back(each);
    g.alts.push_back(multi);
    g.chosen = 2;
    if (all_band && bargs.size() <= 12) {   // the same layer of every chain on row bands, one grid
      int rcb = upload(m, bargs, &bs.d_band);
      if (rcb) return rcb;
      bandm.steps.push_back(bs);
      g.alts.push_back(bandm);
      g.chosen = 3;
    }
    at[last] = g;
  }
  std::vector<Group> out;
  for (int gi = 0; gi < (int)m->groups.size(); gi++) {
    if (!consumed[gi]) out.push_back(m->groups[gi]);
    auto it = at.find(gi);
    if (it != at.end()) out.push_back(it->second);
  }
  m->groups.swap(out);
  return VBT_OK;
}

// ---- network entry: STEM(3x3/2, 3 -> 32) -> DW(3x3/1) -> PW(32 -> <=16) as one kernel (stem_block.h) ----
static bool stem_block_ok(const vbt_model* m, int si, const std::vector<int>& consumers) {
  const int no = (int)m->ops.size();
  if (si + 2 >= no) return false;
  const OpRec& st = m->ops[si];
  const OpRec& d = m->ops[si + 1];
  const OpRec& p = m->ops[si + 2];
  if (st.type != OP_STEM || d.type != OP_DW || p.type != OP_PW) return false;
  const TensorRec& ti = m->tensors[st.inputs[0]];
  const TensorRec& ts = m->tensors[st.output];
  const TensorRec& td = m->tensors[d.output];
  const TensorRec& to = m->tensors[p.output];
  return st.k == 3 && st.stride == 2 && ti.c == 3 && ts.c == 32 && ti.w % 4 == 0 && d.inputs[0] == st.output && consumers[st.output] == 1 &&
         d.k == 3 && d.stride == 1 && d.pad_t == 1 && d.pad_l == 1 && td.c == 32 && p.inputs[0] == d.output && consumers[d.output] == 1 &&
         to.c <= 16 && to.c % 4 == 0;
}

static int make_stem_block(vbt_model* m, int si, Step* out) {
  const OpRec& st = m->ops[si];
  const OpRec& d = m->ops[si + 1];
  const OpRec& p = m->ops[si + 2];
  const TensorRec& ti = m->tensors[st.inputs[0]];
  const TensorRec& ts = m->tensors[st.output];
  const TensorRec& td = m->tensors[d.output];
  const TensorRec& to = m->tensors[p.output];
  Step s;
  s.op = si + 2;
  s.family = F_STEMBLK;
  s.e_op = si;
  s.d_op = si + 1;
  s.p_op = si + 2;
  StemBlockArgs& a = s.sb;
  a.frames = nullptr; a.out = nullptr;
  a.H = ti.h; a.W = ti.w; a.SH = ts.h; a.SW = ts.w; a.Cout = to.c;
  a.spad_t = st.pad_t; a.spad_l = st.pad_l;
  a.tiles_x = (ts.w + 15) / 16; a.tiles_y = (ts.h + 15) / 16;
  a.in_pad4 = (unsigned)((ti.zero_point + 128) & 255) * 0x01010101u;
  a.zs4 = (unsigned)(ts.zero_point & 255) * 0x01010101u;
  a.rqs = make_rq(ts.zero_point, st.act_min, st.act_max, conv_kb(m, st));
  a.rqd = make_rq(td.zero_point, d.act_min, d.act_max, conv_kb(m, d));
  a.rqp = make_rq(to.zero_point, p.act_min, p.act_max, conv_kb(m, p));
  int rc;
  {  // stem: 27 -> 32
    const int8_t* w = (const int8_t*)(m->blob.data() + st.w_off);
    long* dws; int* dbs; float* dms;
    if ((rc = upload(m, pack_stem_block_stem(w), &dws)) || (rc = upload(m, fold_bias((const int32_t*)(m->blob.data() + st.b_off), w, 32, 27, ti.zero_point, W_ROWS), &dbs)) ||
        (rc = upload(m, pad_floats((const float*)(m->blob.data() + st.m_off), 32, 32), &dms)))
      return rc;
    a.ws = dws; a.bs = dbs; a.ms = dms;
    v4i* dws64;   // the direct form (variant 1): kernel rows straight from the raw rows, 16x16x64
    if ((rc = upload(m, pack_stem_block_stem64(w), &dws64))) return rc;
    a.ws64 = dws64;
    a.in_pad4s = a.in_pad4 ^ 0x80808080u;
  }
  const Step& ds = m->op_steps[si + 1];  // matrix-pipe depthwise bias / multipliers of the dw op
  a.bdm = ds.bdm; a.mdm = ds.mdm;
  v4i* d64;   // depthwise weights in the 16x16x64 form, two groups of 16 channels
  if ((rc = upload(m, pack_dw64((const int8_t*)(m->blob.data() + d.w_off), 32, 3, 2), &d64))) return rc;
  a.wd64 = d64;
  {  // project: row i = cout i, K = 32
    const int8_t* w = (const int8_t*)(m->blob.data() + p.w_off);
    long* dwp; int* dbp; float* dmp;
    if ((rc = upload(m, pack_stem_block_proj(w, to.c), &dwp)) || (rc = upload(m, fold_bias((const int32_t*)(m->blob.data() + p.b_off), w, to.c, 32, td.zero_point, W_ROWS, 16), &dbp)) ||
        (rc = upload(m, pad_floats((const float*)(m->blob.data() + p.m_off), to.c, 16), &dmp)))
      return rc;
    a.wp = dwp; a.bp = dbp; a.mp = dmp;
    long* dwpc;   // the direct form: K in the order of the depthwise registers
    if ((rc = upload(m, pack_stem_block_proj_chain(w, to.c), &dwpc))) return rc;
    a.wpc = dwpc;
  }
  s.cost = cost_of(m, {si, si + 1, si + 2});
  *out = s;
  return VBT_OK;
}

// ---- expand + depthwise on whole images (expdw_block.h) ----
// LDS of the whole-image / row-band expand + depthwise kernel for `nbands` bands: T0 (input rows of the tallest band) | E | D
struct ExpDwGeom { int nbands, brows, t0_bytes, e_bytes, d_bytes; };
static ExpDwGeom expdw_geom(int H, int W, int OH, int OW, int k, int stride, int pad_t, int pad_l, int T0S, int nbands) {
  ExpDwGeom g;
  g.nbands = nbands;
  g.brows = (OH + nbands - 1) / nbands;
  g.nbands = (OH + g.brows - 1) / g.brows;
  const int PW = std::max((OW - 1) * stride + k, pad_l + W);
  int in_rows = 0;
  for (int b = 0; b < g.nbands; b++) {
    const int oy0 = b * g.brows, oy1 = std::min(oy0 + g.brows, OH);
    const int PHb = (oy1 - oy0 - 1) * stride + k;
    const int lo = std::max(oy0 * stride - pad_t, 0), hi = std::min(oy0 * stride - pad_t + PHb, H);
    in_rows = std::max(in_rows, hi - lo);
  }
  const int PHmax = (g.brows - 1) * stride + k;
  g.t0_bytes = (in_rows * W * T0S + 15) & ~15;
  g.e_bytes = PHmax * PW * XD_EST;
  g.d_bytes = ((g.brows * OW + 15) / 16) * 16 * XD_EST;
  return g;
}
// whole image when the map has at most 400 pixels and fits (every block of Lite0: the round-2 plan is unchanged); otherwise the
// fewest bands whose workgroup stays below 96 KB (one and a half workgroups' worth of a CU)
static ExpDwGeom expdw_choose(int H, int W, int OH, int OW, int k, int stride, int pad_t, int pad_l, int T0S) {
  const int budget = 96 * 1024;
  ExpDwGeom g = expdw_geom(H, W, OH, OW, k, stride, pad_t, pad_l, T0S, 1);
  if (H * W <= 400 && OH * OW <= 400 && g.t0_bytes + g.e_bytes + g.d_bytes <= 160 * 1024) return g;
  for (int nb = 2; nb <= OH; nb++) {
    g = expdw_geom(H, W, OH, OW, k, stride, pad_t, pad_l, T0S, nb);
    if (g.t0_bytes + g.e_bytes + g.d_bytes <= budget) return g;
  }
  return g;
}
static bool expdw_ok(const vbt_model* m, int e_op, int d_op) {
  const OpRec& e = m->ops[e_op];
  const OpRec& d = m->ops[d_op];
  const TensorRec& tin = m->tensors[e.inputs[0]];
  const TensorRec& tout = m->tensors[d.output];
  const int KS64 = (tin.c + 63) / 64;
  const bool shape = (d.k == 3 && d.stride == 1) || (d.k == 5 && (d.stride == 1 || d.stride == 2));
  if (!(shape && tin.h * tin.w <= 1024 && tin.c % 8 == 0 && tout.c % 16 == 0 && KS64 >= 2 && KS64 <= 4)) return false;
  const ExpDwGeom g = expdw_choose(tin.h, tin.w, tout.h, tout.w, d.k, d.stride, d.pad_t, d.pad_l, ((tin.c + 15) / 16 | 1) * 16);
  return g.t0_bytes + g.e_bytes + g.d_bytes <= 160 * 1024;
}
static int make_expdw2(vbt_model* m, int e_op, int d_op, Step* s, const std::vector<v4i>& pe, const std::vector<int>& be, const std::vector<float>& me,
                       const std::vector<int>& bd, const std::vector<float>& md);
static int make_expdw(vbt_model* m, int e_op, int d_op, Step* out) {
  const OpRec& eop = m->ops[e_op];
  const OpRec& dop = m->ops[d_op];
  const TensorRec& tin = m->tensors[eop.inputs[0]];
  const TensorRec& te = m->tensors[eop.output];
  const TensorRec& td = m->tensors[dop.output];
  Step s;
  s.family = F_EXPDW;
  s.op = d_op;
  s.e_op = e_op;
  s.d_op = d_op;
  ExpDwArgs& a = s.xd;
  memset(&a, 0, sizeof(a));
  a.H = tin.h; a.W = tin.w; a.Cin = tin.c; a.OH = td.h; a.OW = td.w; a.Ce = te.c;
  a.pad_t = dop.pad_t; a.pad_l = dop.pad_l;
  a.PH = std::max((a.OH - 1) * dop.stride + dop.k, a.pad_t + a.H);
  a.PW = std::max((a.OW - 1) * dop.stride + dop.k, a.pad_l + a.W);
  const int K = tin.c, Ce = te.c, nch = (Ce + 63) / 64, kk = dop.k * dop.k;
  // input rows hold the real channels (16-byte granules), not the K padding: the B-operand reads of the padded K run into the
  // next pixel's bytes and meet zero weights (the last pixel's into the E tile).  An odd number of 16-byte granules per row
  // makes the 16-pixel b128 reads bank-conflict-free (80, 112, 208 bytes for 80, 112, 192 channels; was 160 / 224): the
  // 20x20 blocks free 32 KB of LDS per CU for the other forwards in flight.
  a.T0S = ((tin.c + 15) / 16 | 1) * 16;
  a.nchunks = nch;
  a.cpw = 1;
  const ExpDwGeom geo = expdw_choose(a.H, a.W, a.OH, a.OW, dop.k, dop.stride, a.pad_t, a.pad_l, a.T0S);
  a.nbands = geo.nbands; a.brows = geo.brows; a.t0_bytes = geo.t0_bytes; a.e_bytes = geo.e_bytes;
  const int8_t* we = (const int8_t*)(m->blob.data() + eop.w_off);
  const int8_t* wd = (const int8_t*)(m->blob.data() + dop.w_off);
  const std::vector<v4i> pe = pack_expdw_expand(we, Ce, K);
  const std::vector<int> be = fold_bias((const int32_t*)(m->blob.data() + eop.b_off), we, Ce, K, tin.zero_point, W_ROWS, nch * 64);
  const std::vector<int> bd = fold_bias((const int32_t*)(m->blob.data() + dop.b_off), wd, Ce, kk, te.zero_point, W_TAPS, nch * 64);
  const std::vector<float> me = pad_floats((const float*)(m->blob.data() + eop.m_off), Ce, nch * 64);
  const std::vector<float> md = pad_floats((const float*)(m->blob.data() + dop.m_off), Ce, nch * 64);
  v4i* dpe;
  long* dpd;
  int *dbe, *dbd;
  float *dme, *dmd;
  int rc;
  if ((rc = upload(m, pe, &dpe)) || (rc = upload(m, pack_expdw_taps(wd, Ce, kk), &dpd)) || (rc = upload(m, be, &dbe)) || (rc = upload(m, bd, &dbd)) ||
      (rc = upload(m, me, &dme)) || (rc = upload(m, md, &dmd)))
    return rc;
  a.we = dpe; a.wdc = dpd; a.be = dbe; a.bd = dbd; a.me = dme; a.md = dmd;
  a.rqe = make_rq(te.zero_point, eop.act_min, eop.act_max, conv_kb(m, eop));
  a.rqd = make_rq(td.zero_point, dop.act_min, dop.act_max, conv_kb(m, dop));
  a.zeb = (unsigned)(te.zero_point & 255) * 0x01010101u;
  s.lds_bytes = geo.t0_bytes + geo.e_bytes + geo.d_bytes;
  s.cost = cost_of(m, {e_op, d_op});
  if ((rc = make_expdw2(m, e_op, d_op, &s, pe, be, me, bd, md))) return rc;
  *out = s;
  return VBT_OK;
}

// ---- second form of the expand + depthwise kernel (expdw2_block.h): stride 1, Cin % 16 == 0 ----
// (geometry: expdw2_geom.h)
// fills s->xd2 from the finished first-form arguments s->xd and the host images of its expand weights / biases / multipliers
static int make_expdw2(vbt_model* m, int e_op, int d_op, Step* s, const std::vector<v4i>& pe, const std::vector<int>& be, const std::vector<float>& me,
                       const std::vector<int>& bd, const std::vector<float>& md) {
  const OpRec& dop = m->ops[d_op];
  const ExpDwArgs& a1 = s->xd;
  s->xd2_ok = false;
  const int KS64 = (a1.Cin + 63) / 64;
  if ((dop.stride != 1 && dop.stride != 2) || (dop.k != 3 && dop.k != 5) || a1.Cin % 8 != 0 || KS64 < 2 || KS64 > 4) return VBT_OK;
  const ExpDw2Geom geo = expdw2_choose(a1.H, a1.W, a1.OH, a1.OW, dop.k, dop.stride, a1.pad_t, KS64);
  if (!geo.ok) return VBT_OK;
  ExpDw2Args& a = s->xd2;
  memset(&a, 0, sizeof(a));
  a.H = a1.H; a.W = a1.W; a.Cin = a1.Cin; a.OH = a1.OH; a.OW = a1.OW; a.Ce = a1.Ce;
  a.pad_t = a1.pad_t; a.pad_l = a1.pad_l;
  a.nchunks = a1.nchunks; a.cpw = 1; a.nbands = geo.nbands; a.brows = geo.brows;
  a.XB = geo.XB; a.EQS = geo.EQS; a.EYS = geo.EYS; a.e_bytes = geo.e_bytes; a.PS = geo.PS; a.pe_off = geo.pe_off; a.pd_off = geo.pd_off;
  a.rqe = a1.rqe; a.zeb = a1.zeb; a.rqd = a1.rqd;
  const TensorRec& te = m->tensors[m->ops[e_op].output];
  const int Ce = te.c, nch = a.nchunks, kk = dop.k, S = dop.stride, KT2 = (S * (S - 1) + kk + 1) / 2;
  const int NE = KS64 * 256 + 32, ND = KT2 * 256 + 32;
  const int8_t* wd = (const int8_t*)(m->blob.data() + dop.w_off);
  std::vector<v4i> ppe((size_t)nch * NE), ppd((size_t)nch * ND);
  for (int c = 0; c < nch; c++) {
    v4i* e = &ppe[(size_t)c * NE];
    memcpy(e, &pe[(size_t)c * KS64 * 256], sizeof(v4i) * KS64 * 256);
    memcpy(e + KS64 * 256, &be[c * 64], 256);
    memcpy(e + KS64 * 256 + 16, &me[c * 64], 256);
    v4i* d = &ppd[(size_t)c * ND];
    const std::vector<unsigned> tab = pack_expdw2_taps(wd, Ce, 64 * c, 16, kk, S);
    memcpy(d, tab.data(), tab.size() * sizeof(unsigned));
    memcpy(d + KT2 * 256, &bd[c * 64], 256);
    memcpy(d + KT2 * 256 + 16, &md[c * 64], 256);
  }
  v4i *dpe, *dpd;
  int rc;
  if ((rc = upload(m, ppe, &dpe)) || (rc = upload(m, ppd, &dpd))) return rc;
  a.pe = dpe; a.pd = dpd;
  s->xd2_ok = true;
  s->xd2_lds = geo.lds;
  s->xd2_gpw = geo.gpw;
  s->xd2_gpw16 = geo.gpw16;
  s->xd2_small = geo.small;
  return VBT_OK;
}

// the projection conv `p_op` with the block's residual ADD `a_op` = ADD(conv output, skip) evaluated in its epilogue
static Step pw_with_residual(const vbt_model* m, int p_op, int a_op) {
  Step s = m->op_steps[p_op];
  s.op = a_op;
  s.p_op = p_op;
  s.res_op = a_op;
  s.addq = m->op_steps[a_op].addq;
  s.cost += m->op_steps[a_op].cost;   // (an ADD has neither weights nor MACs)
  return s;
}

// ---- fuse_plan: the op list cut into groups; one builder per pattern, each returning the group's alternatives in a fixed order
// (plan files select alternatives by index) ----
struct PlanCtx {
  std::vector<int> consumers, producer;   // per tensor: number of reading ops, producing op (-1: none)
  bool fuse_mb, fuse_sep, fuse_node;
};
static PlanCtx plan_ctx(const vbt_model* m) {
  PlanCtx cx;
  cx.consumers.assign(m->tensors.size(), 0);
  cx.producer.assign(m->tensors.size(), -1);
  for (int i = 0; i < (int)m->ops.size(); i++) {
    for (int k = 0; k < m->ops[i].n_inputs; k++) cx.consumers[m->ops[i].inputs[k]]++;
    cx.producer[m->ops[i].output] = i;
  }
  cx.fuse_mb = !(m->flags & 1) && !(m->flags & 2);
  cx.fuse_sep = !(m->flags & 1) && !(m->flags & 4);
  cx.fuse_node = cx.fuse_sep && !(m->flags & VBT_MODEL_NO_NODE_FUSION);
  return cx;
}
// DW(3|5, stride 1|2) -> PW at op di, the depthwise output read by nobody else
static bool sep_ok(const vbt_model* m, const PlanCtx& cx, int di) {
  if (di + 1 >= (int)m->ops.size()) return false;
  const OpRec& d = m->ops[di];
  const OpRec& p = m->ops[di + 1];
  return d.type == OP_DW && (d.k == 3 || d.k == 5) && (d.stride == 1 || d.stride == 2) && p.type == OP_PW && p.inputs[0] == d.output &&
         cx.consumers[d.output] == 1 && m->tensors[d.inputs[0]].c % 8 == 0 && (m->tensors[p.output].c + 63) / 64 <= 5;
}
// PW -> DW -> PW at op i (an MBConv block; the residual ADD is found by mbconv_group)
static bool mbconv_ok(const vbt_model* m, const PlanCtx& cx, int i) {
  const OpRec& op = m->ops[i];
  return op.type == OP_PW && i + 2 < (int)m->ops.size() && m->ops[i + 1].inputs[0] == op.output && cx.consumers[op.output] == 1 && sep_ok(m, cx, i + 1) &&
         m->tensors[op.inputs[0]].c % 8 == 0;
}

// BiFPN nodes: ADD(2|3 inputs) -> DW -> PW where some ADD inputs come from a RESIZE / MAXPOOL used only here
struct Nodes { std::vector<NodeSrc> node_of; std::vector<char> is_node, absorbed; };
static Nodes find_nodes(const vbt_model* m, const PlanCtx& cx) {
  const int no = (int)m->ops.size();
  Nodes nd;
  nd.node_of.resize(no);
  nd.is_node.assign(no, 0);
  nd.absorbed.assign(no, 0);
  if (!cx.fuse_node) return nd;
  for (int i = 0; i < no; i++) {
    const OpRec& ad = m->ops[i];
    if (ad.type != OP_ADD || ad.n_inputs != 2 || !sep_ok(m, cx, i + 1) || m->ops[i + 1].inputs[0] != ad.output ||
        cx.consumers[ad.output] != 1 || m->tensors[ad.output].c % 4 != 0)
      continue;
    NodeSrc ns;
    auto absorb = [&](int j, int t) {   // source j = tensor t, read through the resize / max pool that produced it when possible
      const int pj = cx.producer[t];
      ns.tensor[j] = t; ns.mode[j] = 0; ns.rs_op[j] = -1;
      const bool same_q = pj >= 0 && m->tensors[m->ops[pj].inputs[0]].scale == m->tensors[t].scale && m->tensors[m->ops[pj].inputs[0]].zero_point == m->tensors[t].zero_point;
      if (pj >= 0 && same_q && cx.consumers[t] == 1 && (m->ops[pj].type == OP_RESIZE_NN || (m->ops[pj].type == OP_MAXPOOL && m->ops[pj].k == 3 && m->ops[pj].stride == 2))) {
        ns.tensor[j] = m->ops[pj].inputs[0];
        ns.mode[j] = m->ops[pj].type == OP_RESIZE_NN ? 1 : 2;
        ns.rs_op[j] = pj;
        nd.absorbed[pj] = 1;
      }
    };
    int pre = -1, pos = 0;
    if (i >= 1)
      for (int j = 0; j < 2; j++) {
        const int pj = cx.producer[ad.inputs[j]];
        if (pj == i - 1 && m->ops[pj].type == OP_ADD && m->ops[pj].n_inputs == 2 && cx.consumers[ad.inputs[j]] == 1) { pre = pj; pos = j; }
      }
    if (pre >= 0) {
      ns.n = 3;
      ns.pre_add = pre;
      ns.chain = pos + 1;
      absorb(0, m->ops[pre].inputs[0]);
      absorb(1, m->ops[pre].inputs[1]);
      absorb(2, ad.inputs[1 - pos]);
      nd.absorbed[pre] = 1;
    } else {
      ns.n = 2;
      for (int j = 0; j < 2; j++) absorb(j, ad.inputs[j]);
    }
    nd.node_of[i] = ns;
    nd.is_node[i] = 1;
  }
  return nd;
}

// appends an alternative (steps + the tensors it keeps out of HBM) to a group; _if_fits: when its kernel's LDS fits `lds_limit`
static void add_alt(Group& g, std::vector<Step> steps, std::vector<int> hidden = {}) {
  Alt a;
  a.steps = std::move(steps);
  a.hidden = std::move(hidden);
  g.alts.push_back(std::move(a));
}
static bool add_alt_if_fits(Group& g, int lds_bytes, int lds_limit, std::vector<Step> steps, std::vector<int> hidden) {
  if (lds_bytes > lds_limit) return false;
  add_alt(g, std::move(steps), std::move(hidden));
  return true;
}
static std::vector<Step> op_steps_of(const vbt_model* m, int first, int n) { return std::vector<Step>(m->op_steps.begin() + first, m->op_steps.begin() + first + n); }
static std::vector<Step> operator+(std::vector<Step> a, const std::vector<Step>& b) { a.insert(a.end(), b.begin(), b.end()); return a; }

constexpr int LDS_STATIC = 64 * 1024, LDS_OPT_IN = 160 * 1024;   // what a tile kernel / an opted-in (band, whole-image) kernel may use

static int node_group(vbt_model* m, int i, const NodeSrc& ns, Group* g) {
  std::vector<Step> pre;          // the resamples / partial sum the node absorbs, as launches of their own
  std::vector<int> hidden;        // ... and their outputs, which the node kernels never write
  for (int j = 0; j < ns.n; j++)
    if (ns.rs_op[j] >= 0) { pre.push_back(m->op_steps[ns.rs_op[j]]); hidden.push_back(m->ops[ns.rs_op[j]].output); }
  if (ns.pre_add >= 0) { pre.push_back(m->op_steps[ns.pre_add]); hidden.push_back(m->ops[ns.pre_add].output); }
  hidden.push_back(m->ops[i].output);
  hidden.push_back(m->ops[i + 1].output);
  add_alt(*g, pre + op_steps_of(m, i, 3));
  Step s1, s2, s3;
  int rc;
  if ((rc = make_fused(m, -1, i + 1, i + 2, -1, &s1))) return rc;   // the sum as its own ADD, dw + project fused
  add_alt_if_fits(*g, s1.lds_bytes, LDS_STATIC, pre + std::vector<Step>{m->op_steps[i], s1}, {m->ops[i + 1].output});
  if ((rc = make_fused(m, -1, i + 1, i + 2, -1, &s2, i, &ns))) return rc;
  if (add_alt_if_fits(*g, s2.lds_bytes, LDS_STATIC, {s2}, hidden) && band_ok(m, i + 1, i + 2)) {   // the same node on row bands (band_block.h)
    if ((rc = make_band(m, i + 1, i + 2, i, &ns, &s3))) return rc;
    add_alt_if_fits(*g, s3.lds_bytes, LDS_OPT_IN, {s3}, hidden);
  }
  return VBT_OK;
}

static int stem_group(vbt_model* m, int i, Group* g) {
  add_alt(*g, op_steps_of(m, i, 3));
  Step s1, s2;
  int rc;
  if ((rc = make_fused(m, -1, i + 1, i + 2, -1, &s1))) return rc;
  add_alt_if_fits(*g, s1.lds_bytes, LDS_STATIC, {m->op_steps[i], s1}, {m->ops[i + 1].output});
  if ((rc = make_stem_block(m, i, &s2))) return rc;
  add_alt(*g, {s2}, {m->ops[i].output, m->ops[i + 1].output});
  return VBT_OK;
}

static int mbconv_group(vbt_model* m, const PlanCtx& cx, int i, Group* g, int* span) {
  const OpRec &op = m->ops[i], &d = m->ops[i + 1], &p = m->ops[i + 2];
  int a_op = -1, rc;
  if (i + 3 < (int)m->ops.size()) {
    const OpRec& ad = m->ops[i + 3];
    if (ad.type == OP_ADD && ad.n_inputs == 2 && ad.inputs[0] == p.output && ad.inputs[1] == op.inputs[0] &&
        cx.consumers[p.output] == 1 && d.stride == 1 && m->tensors[op.inputs[0]].c == m->tensors[p.output].c)
      a_op = i + 3;
  }
  *span = a_op >= 0 ? 4 : 3;
  const std::vector<Step> add = a_op >= 0 ? op_steps_of(m, a_op, 1) : std::vector<Step>();
  const bool res_in_pw = a_op >= 0 && m->tensors[p.output].c % 8 == 0;   // the residual ADD fits the projection's epilogue
  add_alt(*g, op_steps_of(m, i, *span));
  if (res_in_pw && cx.fuse_sep)   // one kernel per conv, the residual ADD in the projection's epilogue
    add_alt(*g, {m->op_steps[i], m->op_steps[i + 1], pw_with_residual(m, i + 2, a_op)}, {p.output});
  if (cx.fuse_sep) {  // expand as its own kernel, dw+project fused; the residual stays a separate ADD (its skip input is not in T0)
    Step s;
    if ((rc = make_fused(m, -1, i + 1, i + 2, -1, &s))) return rc;
    add_alt_if_fits(*g, s.lds_bytes, LDS_STATIC, std::vector<Step>{m->op_steps[i], s} + add, {d.output});
  }
  if (cx.fuse_mb) {
    Step s;
    if ((rc = make_fused(m, i, i + 1, i + 2, a_op, &s))) return rc;
    std::vector<int> hidden{op.output, d.output};
    if (a_op >= 0) hidden.push_back(p.output);
    add_alt_if_fits(*g, s.lds_bytes, LDS_STATIC, {s}, hidden);
  }
  if (cx.fuse_mb && !(m->flags & VBT_MODEL_NO_EXPDW) && expdw_ok(m, i, i + 1)) {
    // low-resolution blocks: expand + depthwise on whole images (channel-split grid), projection as a pointwise GEMM with
    // the residual in its epilogue
    Step sx;
    if ((rc = make_expdw(m, i, i + 1, &sx))) return rc;
    if (res_in_pw) add_alt_if_fits(*g, sx.lds_bytes, LDS_OPT_IN, {sx, pw_with_residual(m, i + 2, a_op)}, {op.output, p.output});
    else add_alt_if_fits(*g, sx.lds_bytes, LDS_OPT_IN, std::vector<Step>{sx, m->op_steps[i + 2]} + add, {op.output});
  }
  return VBT_OK;
}

static int sepconv_group(vbt_model* m, int i, Group* g) {
  add_alt(*g, op_steps_of(m, i, 2));
  Step s, s3;
  int rc;
  if ((rc = make_fused(m, -1, i, i + 1, -1, &s))) return rc;
  if (add_alt_if_fits(*g, s.lds_bytes, LDS_STATIC, {s}, {m->ops[i].output}) && band_ok(m, i, i + 1)) {
    if ((rc = make_band(m, i, i + 1, -1, nullptr, &s3))) return rc;
    add_alt_if_fits(*g, s3.lds_bytes, LDS_OPT_IN, {s3}, {m->ops[i].output});
  }
  return VBT_OK;
}

static void single_group(const vbt_model* m, int i, Group* g) { add_alt(*g, op_steps_of(m, i, 1)); }

static int fuse_plan(vbt_model* m) {
  const PlanCtx cx = plan_ctx(m);
  const Nodes nd = find_nodes(m, cx);
  const int no = (int)m->ops.size();
  for (int i = 0; i < no;) {
    if (nd.absorbed[i]) { i++; continue; }  // emitted with its node
    Group g;
    int span = 1, rc = VBT_OK;
    if (nd.is_node[i]) { rc = node_group(m, i, nd.node_of[i], &g); span = 3; }
    else if (cx.fuse_sep && !(m->flags & VBT_MODEL_NO_STEM_FUSION) && stem_block_ok(m, i, cx.consumers)) { rc = stem_group(m, i, &g); span = 3; }
    else if (mbconv_ok(m, cx, i) && (cx.fuse_mb || cx.fuse_sep)) rc = mbconv_group(m, cx, i, &g, &span);
    else if (cx.fuse_sep && sep_ok(m, cx, i)) { rc = sepconv_group(m, i, &g); span = 2; }
    else single_group(m, i, &g);
    if (rc) return rc;
    g.chosen = (int)g.alts.size() - 1;  // without autotuning: the most fused alternative
    m->groups.push_back(g);
    i += span;
  }
  if (cx.fuse_sep && !(m->flags & VBT_MODEL_NO_HEAD_BATCHING)) return batch_heads(m);
  return VBT_OK;
}

// Pointwise convs that read nothing but tensors already there when the first of them runs are merged into one launch
// (pw_multi_kernel): in an EfficientDet graph the P6 conv and the five lateral convs of the first BiFPN cell all read backbone
// outputs.  The anchor is the stand-alone pointwise conv with the most followers; a conv followed by the two 3x3/2 max pools
// that make P6 and P7 takes them along.  Every merged tensor is still written, by the same arithmetic.
static bool pwm_mergeable(const vbt_model* m, const Step& s) {
  if (s.family != F_PW || s.res_op >= 0 || !s.members.empty() || !s.wp64) return false;
  const OpRec& op = m->ops[s.op];
  return op.type == OP_PW && m->tensors[op.output].c % 4 == 0 && s.KS64 >= 1;
}
static void merge_side_convs(vbt_model* m) {
  static const bool off = getenv("VBT_NO_PW_MERGE") != nullptr;
  if (off || (m->flags & (VBT_MODEL_NO_FUSION | VBT_MODEL_NO_PW_MERGE))) return;
  // sub-batch streams: the merged launch's problem list holds whole-batch pointers (the guard band_ok() has; n_sub is final by now)
  if (m->n_sub > 1) return;
  const int ns = (int)m->steps.size(), no = (int)m->ops.size();
  // which step runs which graph op: the ops a step names, then (absorbed resamples / partial sums) the step of their consumer
  std::vector<int> step_of(no, -1);
  for (int i = 0; i < ns; i++)
    for_each_named_op(m->steps[i], [&](int o) { if (o < no) step_of[o] = i; });
  std::vector<std::vector<int>> readers(m->tensors.size());
  std::vector<int> producer(m->tensors.size(), -1);
  for (int o = 0; o < no; o++) {
    producer[m->ops[o].output] = o;
    for (int k = 0; k < m->ops[o].n_inputs; k++) readers[m->ops[o].inputs[k]].push_back(o);
  }
  for (int o = no - 1; o >= 0; o--)
    if (step_of[o] < 0) {
      int best = ns;
      for (int r : readers[m->ops[o].output]) if (step_of[r] >= 0) best = std::min(best, step_of[r]);
      step_of[o] = best < ns ? best : -1;
    }
  for (int o = 0; o < no; o++) if (step_of[o] < 0) return;    // an op nobody runs: leave the plan alone
  auto made_at = [&](int tensor) { return producer[tensor] >= 0 ? step_of[producer[tensor]] : -1; };
  auto first_read = [&](int tensor, int except_op = -1) {
    int f = ns;
    for (int r : readers[tensor]) if (r != except_op) f = std::min(f, step_of[r]);
    return f;
  };
  // the P6 / P7 chain: a conv whose output feeds a 3x3/2 max pool that feeds another one (steps of their own)
  auto pools_of = [&](int conv_step, int* k1, int* k2) {
    const int t0 = m->ops[m->steps[conv_step].op].output;
    for (int r1 : readers[t0]) {
      const OpRec& p1 = m->ops[r1];
      if (p1.type != OP_MAXPOOL || p1.k != 3 || p1.stride != 2 || m->steps[step_of[r1]].family != F_MAXPOOL) continue;
      for (int r2 : readers[p1.output]) {
        const OpRec& p2 = m->ops[r2];
        if (p2.type != OP_MAXPOOL || p2.k != 3 || p2.stride != 2 || m->steps[step_of[r2]].family != F_MAXPOOL) continue;
        const TensorRec &to = m->tensors[t0], &t1 = m->tensors[p1.output];
        if (to.c % 16 != 0 || (size_t)((to.h * to.w * to.c + 15) & ~15) + (size_t)t1.h * t1.w * t1.c > 64 * 1024) continue;
        *k1 = step_of[r1]; *k2 = step_of[r2];
        return true;
      }
    }
    return false;
  };
  // every stand-alone conv as the anchor (the slot the merged launch takes): member j fits when its input exists before the anchor
  // and nobody reads its output before the anchor has run
  int best = -1, best_chain = -1, bk1 = -1, bk2 = -1;
  std::vector<int> best_set;
  for (int a = 0; a < ns; a++) {
    if (!pwm_mergeable(m, m->steps[a])) continue;
    std::vector<int> set;
    int chain = -1, k1 = -1, k2 = -1;
    for (int j = 0; j < ns && (int)set.size() < PW_MERGE_MAX; j++) {
      if (!pwm_mergeable(m, m->steps[j])) continue;
      const OpRec& cj = m->ops[m->steps[j].op];
      if (j > a && made_at(cj.inputs[0]) >= a) continue;            // hoisted to the anchor: its input must exist by then
      int c1, c2;
      if (chain < 0 && pools_of(j, &c1, &c2)) {
        // the pools come along: the conv's other readers and the pools' readers must all run after the anchor
        const OpRec &p1 = m->ops[m->steps[c1].op], &p2 = m->ops[m->steps[c2].op];
        if (first_read(cj.output, m->steps[c1].op) > a && first_read(p1.output, m->steps[c2].op) > a && first_read(p2.output) > a) {
          chain = j; k1 = c1; k2 = c2;
          set.push_back(j);
          continue;
        }
      }
      if (first_read(cj.output) > a) set.push_back(j);               // (sunk or hoisted: nobody reads its output before the anchor has run)
    }
    // no member may read another member's output (they run side by side)
    for (bool again = true; again;) {
      again = false;
      for (size_t q = 0; q < set.size(); q++) {
        const int src = made_at(m->ops[m->steps[set[q]].op].inputs[0]);
        if (src >= 0 && std::find(set.begin(), set.end(), src) != set.end()) {
          if (set[q] == chain) chain = -1;
          set.erase(set.begin() + q);
          again = true;
          break;
        }
      }
    }
    if (std::find(set.begin(), set.end(), a) == set.end()) continue;
    const int score = (int)set.size() + (chain >= 0 ? 2 : 0);
    const int best_score = (int)best_set.size() + (best_chain >= 0 ? 2 : 0);
    if (set.size() >= 2 && score >= best_score) { best = a; best_set = set; best_chain = chain; bk1 = k1; bk2 = k2; }
  }
  if (best < 0) return;
  if (best_chain >= 0) {   // the chain problem goes first (pw_multi_kernel: problem 0)
    best_set.erase(std::find(best_set.begin(), best_set.end(), best_chain));
    best_set.insert(best_set.begin(), best_chain);
  }
  Step merged = m->steps[best_set[0]];
  merged.members.clear();
  merged.cost = Cost();
  merged.nbp = 0;   // (1: problem 0 carries its two pools)
  std::vector<char> drop(ns, 0);
  for (int j : best_set) {
    merged.members.push_back(m->steps[j]);
    merged.cost += m->steps[j].cost;
    drop[j] = 1;
  }
  if (best_chain >= 0) {
    const TensorRec &to = m->tensors[m->ops[m->steps[best_chain].op].output], &t1 = m->tensors[m->ops[m->steps[bk1].op].output];
    merged.nbp = 1;
    merged.lds_bytes = (int)(((to.h * to.w * to.c + 15) & ~15) + t1.h * t1.w * t1.c);
    for (int k : {bk1, bk2}) {
      merged.members.push_back(m->steps[k]);
      merged.cost += m->steps[k].cost;   // (a max pool has neither weights nor MACs)
      drop[k] = 1;
    }
  }
  std::vector<Step> out;
  for (int i = 0; i < ns; i++) {
    if (i == best) out.push_back(merged);
    else if (!drop[i]) out.push_back(m->steps[i]);
  }
  m->steps.swap(out);
}

void finalize_plan(vbt_model* m) {
  m->steps.clear();
  m->materialized.assign(m->tensors.size(), 1);
  for (const Group& g : m->groups) {
    const Alt& a = g.alts[g.chosen];
    for (const Step& s : a.steps) m->steps.push_back(s);
    for (int t : a.hidden) m->materialized[t] = 0;
  }
  merge_side_convs(m);
}

int build_plan(vbt_model* m) {
  const int no = (int)m->ops.size();
  for (int oi = 0; oi < no; oi++) {
    const OpRec& op = m->ops[oi];
    const TensorRec& to = m->tensors[op.output];
    Step s;
    s.op = oi;
    double in_el = 0;
    for (int i = 0; i < op.n_inputs; i++) {
      const TensorRec& ti = m->tensors[op.inputs[i]];
      in_el += (double)ti.h * ti.w * ti.c;
    }
    double out_el = (double)to.h * to.w * to.c;
    s.cost.alg_bytes_per_frame = in_el + out_el;
    if (op.type == OP_STEM || op.type == OP_PW || op.type == OP_DW) {
      const TensorRec& ti = m->tensors[op.inputs[0]];
      const int8_t* w = (const int8_t*)(m->blob.data() + op.w_off);
      const int32_t* bq = (const int32_t*)(m->blob.data() + op.b_off);
      const float* mu = (const float*)(m->blob.data() + op.m_off);
      const int N = to.c;
      const int zx = ti.zero_point;
      if (op.type == OP_DW) {
        s.family = F_DW;
        const int C = N, kk = op.k * op.k;
        if (C % 4 != 0 || !((op.k == 3 || op.k == 5) && (op.stride == 1 || op.stride == 2))) {
          set_error("unsupported depthwise conv: C=%d k=%d s=%d", C, op.k, op.stride);
          return VBT_ERR_ARG;
        }
        int rc;
        if ((rc = upload(m, dw_weights_f32(w, C, kk, C), &s.wf)) || (rc = upload(m, fold_bias(bq, w, C, kk, 128 + zx, W_TAPS), &s.bias)) ||   // acc uses u = x_q + 128, pad u = 128 + z_x
            (rc = upload(m, pad_floats(mu, C, C), &s.mult)))
          return rc;
        const int Cp = (C + 63) / 64 * 64;   // matrix-pipe form: raw int8 inputs, padded to 64 channels
        if ((rc = upload(m, pack_dw_diag(w, C, kk, 64), &s.wdm)) || (rc = upload(m, fold_bias(bq, w, C, kk, zx, W_TAPS, Cp), &s.bdm)) ||
            (rc = upload(m, pad_floats(mu, C, Cp), &s.mdm)))
          return rc;
        s.cost.weight_bytes = (double)kk * C;
        s.cost.macs_per_frame = out_el * kk;
      } else {
        const bool stem = op.type == OP_STEM;
        s.family = stem ? F_STEM : F_PW;
        const int K = stem ? op.k * op.k * ti.c : ti.c;
        if (stem && (op.k != 3 || ti.c != 3 || op.stride != 2)) { set_error("unsupported stem conv"); return VBT_ERR_ARG; }
        if (!stem && (K % 8) != 0) { set_error("pointwise conv needs Cin %% 8 == 0 (got %d)", K); return VBT_ERR_ARG; }
        s.KS = (K + 31) / 32;
        s.NB = (N + 63) / 64;
        const std::vector<int> kmap = stem_kmap();
        std::vector<long> wp;
        pack_weights(w, N, K, s.KS, s.NB, stem ? &kmap : nullptr, wp);
        int rc;
        if ((rc = upload(m, wp, &s.wp)) || (rc = upload(m, fold_bias(bq, w, N, K, zx, W_ROWS, s.NB * 64), &s.bias)) ||   // acc = sum x_q*w ; (x_q - z_x) folded here
            (rc = upload(m, pad_floats(mu, N, s.NB * 64), &s.mult)))
          return rc;
        if (!stem) {
          s.KS64 = (K + 63) / 64;
          std::vector<v4i> wp64;
          pack_weights64(w, N, K, s.KS64, s.NB, wp64);
          if ((rc = upload(m, wp64, &s.wp64))) return rc;
          // the all-blocks form with a tile-major part-filled last block (pw_f_kernel, variants 9 / 10): a second panel
          if (s.KS64 > 4 && N % 64 != 0 && N % 4 == 0 && pw_f_tail_built(s.NB, proj_tail_tiles(N))) {
            pack_weights64_tail(w, N, K, s.KS64, s.NB, wp64);
            if ((rc = upload(m, wp64, &s.wp64t))) return rc;
            s.ntl = proj_tail_tiles(N);
          }
        }
        s.cost.weight_bytes = (double)N * K;
        s.cost.macs_per_frame = out_el * K;
      }
    } else if (op.type == OP_ADD) {
      s.family = F_ADD;
      if (((long)to.h * to.w * to.c) % 4 != 0 || op.n_inputs != 2) { set_error("unsupported add (binary int8 ADD on a multiple of 4 elements expected)"); return VBT_ERR_ARG; }
      const TensorRec& ta = m->tensors[op.inputs[0]];
      const TensorRec& tb = m->tensors[op.inputs[1]];
      AddParams ap;
      if (!xnn_add_params(ta.scale, tb.scale, to.scale, ta.zero_point, tb.zero_point, &ap)) {
        set_error("op %d: ADD input/output scale ratio outside [2^-10, 2^8) (XNNPACK refuses it too)", oi);
        return VBT_ERR_ARG;
      }
      if (ap.bias != op.add_q[0] || ap.am != op.add_q[1] || ap.bm != op.add_q[2] || ap.shift != op.add_q[3]) {
        set_error("op %d: ADD parameters stored in the container (%d,%d,%d,%d) differ from those derived from the tensor scales (%d,%d,%d,%d)",
                  oi, op.add_q[0], op.add_q[1], op.add_q[2], op.add_q[3], ap.bias, ap.am, ap.bm, ap.shift);
        return VBT_ERR_ARG;
      }
      s.addq = make_addq(ap, to.zero_point, op.act_min, op.act_max);
      // survey accounting: a 3-input BiFPN sum is one add; the partial sum between its two binary ADDs is not traffic
      auto sole_add_consumer = [&](int t) {
        int n = 0, add = 0;
        for (const OpRec& o2 : m->ops)
          for (int i = 0; i < o2.n_inputs; i++)
            if (o2.inputs[i] == t) { n++; add += o2.type == OP_ADD; }
        return n == 1 && add == 1;
      };
      if (sole_add_consumer(op.output)) s.cost.alg_bytes_per_frame -= out_el;
      for (int i = 0; i < 2; i++) {
        bool from_add = false;
        for (int o2 = 0; o2 < oi; o2++) from_add |= m->ops[o2].type == OP_ADD && m->ops[o2].output == op.inputs[i];
        if (from_add && sole_add_consumer(op.inputs[i])) s.cost.alg_bytes_per_frame -= (double)m->tensors[op.inputs[i]].h * m->tensors[op.inputs[i]].w * m->tensors[op.inputs[i]].c;
      }
    } else if (op.type == OP_MAXPOOL) {
      s.family = F_MAXPOOL;
      if (to.c % 4 != 0 || op.k != 3 || op.stride != 2) { set_error("unsupported maxpool"); return VBT_ERR_ARG; }
    } else if (op.type == OP_RESIZE_NN) {
      s.family = F_RESIZE;
      if (to.c % 4 != 0) { set_error("unsupported resize"); return VBT_ERR_ARG; }
      // TFLite's kernel computes src = min(floor(dst * (float)in / out), in - 1) in float32; the kernels here use the
      // integer form floor(dst * in / out): refuse a geometry on which the two differ
      const TensorRec& ti = m->tensors[op.inputs[0]];
      for (int ax = 0; ax < 2; ax++) {
        const int in = ax ? ti.w : ti.h, out = ax ? to.w : to.h;
        const float scale = (float)in / (float)out;
        for (int d = 0; d < out; d++)
          if (std::min((int)floorf((float)d * scale), in - 1) != (d * in) / out) {
            set_error("op %d: nearest-neighbour resize %d -> %d is not mapped", oi, in, out);
            return VBT_ERR_ARG;
          }
      }
    } else if (op.type == OP_POSTPROCESS) {
      s.family = F_POST;
      if (op.n_inputs != 10 || m->hdr.max_detections != VBT_MAX_DETECTIONS || m->hdr.num_anchors > 65535) {
        set_error("unsupported postprocess configuration");
        return VBT_ERR_ARG;
      }
      s.cost.alg_bytes_per_frame = in_el + m->hdr.max_detections * 24.0;
      s.cost.weight_bytes = (double)m->hdr.num_anchors * 16;
    } else {
      set_error("unknown op type %d", op.type);
      return VBT_ERR_ARG;
    }
    m->op_steps.push_back(s);
  }
  return fuse_plan(m);
}

}  // namespace vbt
