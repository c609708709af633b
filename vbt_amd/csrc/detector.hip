// EfficientDet-Lite int8 detector on gfx950 (MI355X): variant resolution, launches, the forward (eager or hipGraph replay) and the
// detect entry points of the C ABI.  Host code: every kernel - the single-op ones (k_pointwise.hip, k_ops.hip, k_postprocess.hip) and
// the fused families - lives in a translation unit of its own (k_*.hip) and is reached through launchers.h.  The model handle and what
// the detector's units share: detector_model.h; the planner: planner.hip (weight layouts: weight_pack.h); parameter pool, autotuner, plan
// files and model life cycle: detector_plan.hip; diagnostic timings: detector_profile.hip; error text, device check and LDS opt-in:
// runtime.hip; the frame resize in front of the detector: frames.hip.
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
//   * decode + NMS: one workgroup per frame, 256-bin score histogram -> the top candidates sorted in LDS (by counting; a bitonic
//     network only above 1 024 candidates) -> greedy suppression by one wavefront with ballot / readlane.
#include <algorithm>
#include <cmath>
#include <string>

#include "detector_model.h"
#include "tpz_geom.h"   // the Toeplitz form's LDS geometry (resolve_fused)

namespace vbt {

// ---- variant resolution: one pure host function per launch family turns (step, variant, batch; -1 = heuristic default) into the
// launch it stands for, or refuses it.  The launches, the autotuner's candidates and the plan-file check all ask these.
// (Result structs: detector_model.h.) ----

// pointwise conv (one conv; the merged launch of merge_side_convs has no variants)
PwLaunch resolve_pw(const vbt_model* m, const Step& s, int variant, int B) {
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
  // (a forced 7 / 8 leaves the convs that form refuses - one output block, or more than PW_F_MAX_NB - on the plan's variant)
  // (9 / 10 moreover the convs without a tile-major last block: N % 64 == 0, or a width no shipped model has - pw_f_tail_built)
  const bool f_fits = s.NB >= 2 && s.NB <= PW_F_MAX_NB, ft_fits = f_fits && s.wp64t && pw_f_tail_built(s.NB, s.ntl);
  if (pw_force != -100 && (pw_force == 9 || pw_force == 10 ? ft_fits : (f_fits || (pw_force != 7 && pw_force != 8)))) variant = pw_force;
  if (variant >= 7 && variant <= 10) {   // 64 (7) or 128 (8) pixels per workgroup for ALL output blocks: activations fetched once (pw_f_kernel)
    const bool tail = variant >= 9;      // 9 / 10: the same two with a tile-major part-filled last block (pack_weights64_tail)
    L.form = PW_F;
    L.ms = tail ? variant - 8 : variant - 6;
    L.ntl = tail ? s.ntl : 0;
    L.lds = tail ? (4 * (s.NB - 1) + s.ntl) * 2048 : s.NB * 8192;   // static: two stages of the K-step's weight tiles
    L.grid = dim3((unsigned)((M + 64 * L.ms - 1) / (64 * L.ms)), 1);
    if (s.NB < 2) L.refuse(VBT_ERR_ARG, "pw_conv: one output block - nothing for the all-blocks form to share");
    else if (s.NB > PW_F_MAX_NB) L.refuse(VBT_ERR_ARG, "pw_conv: %d output blocks exceed the %d whose accumulators the all-blocks form holds", s.NB, PW_F_MAX_NB);
    else if (tail && !ft_fits) L.refuse(VBT_ERR_ARG, "pw_conv: no tile-major last block for %d output blocks with %d tail tiles", s.NB, s.ntl);
  } else if (variant >= 3 && variant <= 6) {   // 64 (3 / 5) or 128 (4 / 6) pixels per workgroup; weights shared through LDS (3 / 4: pw_d_kernel)
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
  PwArgs a;
  a.x = x; a.wp = L.ntl ? s.wp64t : s.wp64; a.out = out;
  a.e = Epi{s.bias, s.mult, tpo.zero_point, pop.act_min, pop.act_max, make_rq(tpo.zero_point, pop.act_min, pop.act_max)};
  a.ra = ResArgs{res, s.addq};
  a.M = (long)B * tpo.h * tpo.w;
  a.K = m->tensors[pop.inputs[0]].c; a.KS64 = s.KS64; a.N = tpo.c; a.NB = s.NB; a.nb_per_y = L.nb_per_y;
  return launch_pw(a, L, L.grid, L.lds, st);
}

// stand-alone depthwise conv: 0 = one output row x 4 columns per lane, 100 / 101 = LDS tiles, chunk-parallel (101: depthwise on the
// matrix pipe), anything else = column walker with `variant` output rows per lane (-1: rows chosen by the map size)
DwLaunch resolve_dw(const vbt_model* m, const Step& s, int variant, int B) {
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
  DwArgs a;
  a.x = x; a.wf = s.wf; a.e = e; a.out = out; a.total = L.total;
  a.H = ti.h; a.W = ti.w; a.C = to.c; a.OH = to.h; a.OW = to.w; a.pad_t = op.pad_t; a.pad_l = op.pad_l;
  a.pad4 = pb | (pb << 8) | (pb << 16) | (pb << 24);
  a.rows = L.form == DW_ROW ? 0 : L.rows; a.nseg = L.nseg;
  return launch_dw(a, op.k, op.stride, L.grid, st);
}

// fused MBConv / SeparableConv / BiFPN node on LDS tiles (fused_block.h) or, MBConv on a low-resolution map, one workgroup per image
// (image_block.h).  Variant bits: 1 = depthwise on the matrix pipe (else VALU), 2 = half-height tile, 4 = whole image, 8 = 48-channel
// chunks, 16 = 128-pixel (16 x 8) tiles, 32 = band-Toeplitz depthwise (fused_block.h: TPZ); a bit whose conditions the step does not
// meet is ignored, except that the whole-image and 128-pixel kernels refuse a step they do not fit and that bit 32 resolves only as
// 33, 41, 49 or 57 on a step where each of its other bits holds.
// VBT_PROJ_TAIL (developers; read once per process): "0" = every fused MBConv launch keeps the block-major last projection block, a list
// such as "b1,b3" = only those blocks run it tile-major (a per-block A/B inside one library); unset: every block that has such a launch
static bool proj_tail_on(int block) {
  static const std::string knob = getenv("VBT_PROJ_TAIL") ? std::string(",") + getenv("VBT_PROJ_TAIL") + "," : std::string();
  if (knob.empty()) return true;
  return knob.find(",b" + std::to_string(block) + ",") != std::string::npos;
}
// VBT_FUSED_PARAMS (developers; read once per process), the same syntax: which blocks fetch their chunk parameters once per workgroup,
// through LDS (fused_block.h: PLDS); unset: every block whose resolved launch is built that way and whose tile fits with the parameter area
static bool fused_params_on(int block) {
  static const std::string knob = getenv("VBT_FUSED_PARAMS") ? std::string(",") + getenv("VBT_FUSED_PARAMS") + "," : std::string();
  if (knob.empty()) return true;
  return knob.find(",b" + std::to_string(block) + ",") != std::string::npos;
}
// the parameter block of a resolved launch (Step::cpar), or nullptr
static const unsigned char* fused_params_of(const Step& s, const FusedLaunch& L) { return s.cpar[L.nt3][fused_params_form(L)][L.ntl > 0]; }
FusedPlan resolve_fused(const vbt_model* m, const Step& s, int variant, int B) {
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
  // a part-filled last projection block runs tile-major wherever the step has the panels and the resolved launch is built with a live-tile
  // count: a property of the step, no variant bit (plan files do not change)
  if (s.ntl && proj_tail_on(s.block) && (nt3 ? a.wpt3 : a.wpt) && fused_tail_built(p.L, a.KSe, s.ntl)) p.L.ntl = s.ntl;
  // the chunk parameters once per workgroup, through LDS: again a property of the step - wherever the resolved launch is built that way,
  // the step has its block, and the tile with the parameter area passes the 64 KB the refusals below hold the other form to and still leaves
  // the CU's 160 KB of LDS as many workgroups as the kernel's registers do (else the area would cost a wave per SIMD)
  if (const int wgs = ex && fused_params_on(s.block) && fused_params_of(s, p.L) ? fused_params_built(p.L, a.KSe, p.L.ntl) : 0) {
    const int lds = p.L.lds_bytes + fused_params_lds(fused_params_geom(nt3 ? 3 : 4, a.KSe, fused_params_form(p.L), k, stride, s.nbp, p.L.ntl));
    if (lds <= 64 * 1024 && wgs * lds <= 160 * 1024) { p.L.params = true; p.L.lds_bytes = lds; }
  }
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
  a.cpar = p.L.params ? fused_params_of(s, p.L) : nullptr;
  return launch_fused_block(a, p.L, st);
}

// expand + depthwise on whole images or row bands.  Variant: chunks per workgroup on the first form of the kernel (expdw_block.h),
// 100 + chunks per workgroup on the second (expdw2_block.h) with 8 waves, 200 + chunks with 16 waves, 300 + chunks on its small-map
// instantiation (two workgroups per CU; 10 x 10 maps only); -1: heuristic default
ExpDwLaunch resolve_expdw(const vbt_model*, const Step& s, int variant, int B) {
  // VBT_XD_VARIANT (tests): that variant for every step that supports it, whatever the plan says
  static const int xd_force = getenv("VBT_XD_VARIANT") ? atoi(getenv("VBT_XD_VARIANT")) : -100;
  if (xd_force != -100 && (xd_force < 100 || (s.xd2_ok && (xd_force < 200 ? s.xd2_gpw > 0 : xd_force < 300 ? s.xd2_gpw16 > 0 : s.xd2_small)))) variant = std::min(xd_force, xd_force / 100 * 100 + s.xd.nchunks);
  ExpDwLaunch L;
  if (s.xd2_ok && (variant >= 100 || variant < 0)) {
    if (variant >= 300 && !s.xd2_small) { L.refuse(VBT_ERR_ARG, "expand + depthwise: plan asks for the small-map form on a step that does not support it"); return L; }
    if (variant >= 200 && variant < 300 && s.xd2_gpw16 == 0) { L.refuse(VBT_ERR_ARG, "expand + depthwise: plan asks for the 16-wave form on a step that does not support it"); return L; }
    if (variant >= 100 && variant < 200 && s.xd2_gpw == 0) { L.refuse(VBT_ERR_ARG, "expand + depthwise: plan asks for the 8-wave form on a step that does not support it"); return L; }
    const ExpDw2Args& a = s.xd2;   // the second form
    L.second = true;
    L.small = variant >= 300;
    L.nw = L.small ? XD2S_WAVES : (variant >= 200 || (variant < 0 && s.xd2_gpw16 > 0)) ? 16 : 8;
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
    return launch_expdw2(a, dop.k, dop.stride, (a.Cin + 63) / 64, L.nw, L.gpw, L.small, L.grid, L.lds, st);
  }
  ExpDwArgs a = s.xd;
  a.x = x; a.out = out; a.cpw = L.cpw;
  return launch_expdw(a, dop.k, dop.stride, (a.Cin + 63) / 64, L.grid, L.lds, st);
}

// SeparableConv / BiFPN node / head layer on row bands.  Variant: 0 = depthwise and projection as two stages around the LDS tile D,
// 1 = chained (band_block.h; 64-channel maps with at most 64 output channels), -1: chained where it resolves and max_batch > 8, else two stages.  A step of several
// problems carries one variant for all its members.
static bool band_chainable(const Step& s) {
  if (s.members.empty()) return s.bd_args.wpc != nullptr;
  for (const Step& ms : s.members)
    if (!ms.bd_args.wpc) return false;
  return true;
}
BandLaunch resolve_band(const vbt_model* m, const Step& s, int variant, int) {
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

// Network entry (stem_block.h).  Variant: 0 = the im2col form (P and D tiles in LDS), 1 = the direct form (stem conv straight from the
// raw rows, projection from the depthwise registers), -1 = the im2col form.  Both forms take every map the planner builds the step for.
StemLaunch resolve_stemblk(const vbt_model*, const Step&, int variant, int) {
  StemLaunch L;
  if (variant < -1 || variant > 1) { L.refuse(VBT_ERR_ARG, "fused_stem_block: no kernel form %d", variant); return L; }
  L.direct = variant == 1;
  return L;
}

// Launches one plan step for frames [boff, boff + B) of the batch (every tensor is batch-major): the batch-offset pointers here, the
// variant and the launch in the family's own function above.  `frames` = frame boff, the first one of the range; the output pointers
// are those of the whole batch.
int launch_step(vbt_model* m, const Step& s, int B, hipStream_t st, const uint8_t* frames, float* boxes, float* scores, float* classes,
                int* counts, int boff) {
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
      return launch_stem(StemArgs{frame0, s.wp, e, out, (long)B * to.h * to.w, ti.h, ti.w, to.h, to.w, to.c, op.pad_t, op.pad_l, ti.zero_point}, st);
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
      for (int i = nconv + 1; i <= PW_MERGE_MAX; i++) pm.start[i] = acc;
      return launch_pw_multi(pm, (unsigned)acc, s.nbp ? s.lds_bytes : 0, st);
    }
    case F_DW:
      return launch_dw_step(m, s, B, st, TP(op.inputs[0]), out, e);
    case F_ADD:
      return launch_add(TP(op.inputs[0]), TP(op.inputs[1]), s.addq, out, (long)B * to.h * to.w * to.c / 4, st);
    case F_MAXPOOL:
    case F_RESIZE: {
      const TensorRec& ti = m->tensors[op.inputs[0]];
      const MapArgs a{TP(op.inputs[0]), out, (long)B * to.h * to.w * (to.c / 4), ti.h, ti.w, ti.c, to.h, to.w, op.pad_t, op.pad_l};
      return s.family == F_MAXPOOL ? launch_maxpool(a, st) : launch_resize_nn(a, st);
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
      const StemLaunch L = resolve_stemblk(m, s, s.variant, B);
      if (L.rc) return L.report();
      return launch_stem_block(a, L.direct, (unsigned)((long)B * a.tiles_x * a.tiles_y), st);
    }
    case F_POST: {
      PostArgs p = m->post;   // everything but the head tensors: built once, with the tables (detector_plan.hip)
      for (int l = 0; l < 5; l++) {
        p.cls[l] = TP(op.inputs[l]);
        p.box[l] = TP(op.inputs[5 + l]);
      }
      if (m->post_lds > 160 * 1024 || p.A > 65535) { set_error("decode + NMS: %d anchors do not fit the kernel (LDS %d bytes, 16-bit anchor index)", p.A, m->post_lds); return VBT_ERR_CAPACITY; }
      const size_t o = (size_t)boff * m->hdr.max_detections;
      return launch_postprocess(p, m->post_lds, B, boxes + 4 * o, scores + o, classes + o, counts + boff, st);
    }
  }
  return VBT_OK;
}

int enqueue_forward(vbt_model* m, const uint8_t* frames_dev, int B, hipStream_t st, float* boxes, float* scores, float* classes, int* counts,
                    const Event* evs) {
  const int nsub = (!evs && m->n_sub > 1 && B >= 2 * m->n_sub) ? m->n_sub : 1;
  if (nsub == 1) {
    int i = 0;
    for (const Step& s : m->steps) {
      if (evs) (void)hipEventRecord(evs[i].get(), st);
      int rc = launch_step(m, s, B, st, frames_dev, boxes, scores, classes, counts);
      if (rc) return rc;
      i++;
    }
    if (evs) (void)hipEventRecord(evs[i].get(), st);
  } else {
    // Independent sub-batches on side streams: the many small, latency-bound kernels of one sub-batch overlap
    // with the other's.  Fork from / join into the caller's stream with events.
    (void)hipEventRecord(m->ev_fork.get(), st);
    const int per = (B + nsub - 1) / nsub;
    for (int k = 0; k < nsub; k++) {
      const int b0 = k * per, bk = std::min(per, B - b0);
      if (bk <= 0) break;
      hipStream_t ss = m->sub_streams[k].get();
      (void)hipStreamWaitEvent(ss, m->ev_fork.get(), 0);
      for (const Step& s : m->steps) {
        int rc = launch_step(m, s, bk, ss, frames_dev + (size_t)b0 * m->hdr.image_size * m->hdr.image_size * 3, boxes, scores, classes, counts, b0);
        if (rc) return rc;
      }
      (void)hipEventRecord(m->ev_join[k].get(), ss);
      (void)hipStreamWaitEvent(st, m->ev_join[k].get(), 0);
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
    if (m->graphs.size() >= 256) m->clear_graphs();  // bounded cache
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    if (!m->ran_eager) {
      // The first forward of a model never runs inside a capture: the per-device LDS opt-ins of its kernels (hipFuncSetAttribute) and any
      // failure they report happen here, eagerly, on the caller's stream (same buffers, same results as the replay that follows).
      const int rc0 = enqueue_forward(m, frames_dev, B, st, boxes, scores, classes, counts, nullptr);
      if (rc0) return rc0;
      m->ran_eager = true;
    }
    VBT_HIP_CHECK(hipStreamBeginCapture(m->cap_stream.get(), hipStreamCaptureModeThreadLocal));
    int rc = enqueue_forward(m, frames_dev, B, m->cap_stream.get(), boxes, scores, classes, counts, nullptr);
    hipError_t e = hipStreamEndCapture(m->cap_stream.get(), &g);
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

using namespace vbt;

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int vbt_detect_async(vbt_model* m, const uint8_t* frames_dev, int B, void* stream, float* boxes, float* scores, float* classes,
                     int32_t* counts) {
  if (!m || !frames_dev || !boxes || !scores || !classes || !counts) { set_error("vbt_detect_async: NULL argument"); return VBT_ERR_ARG; }
  if (B < 1 || B > m->max_batch) { set_error("vbt_detect: batch %d outside 1..%d", B, m->max_batch); return VBT_ERR_CAPACITY; }
  return forward(m, frames_dev, B, (hipStream_t)stream, boxes, scores, classes, counts);
}

int vbt_model_entry_steps(const vbt_model* m) { return m ? entry_steps(m) : VBT_ERR_ARG; }

// grids of several problems carry whole-batch pointers (launch_step): such a step runs from image 0 only
static bool image0_only(const Step& s) { return (s.family == F_PW && !s.members.empty()) || s.family == F_BAND; }

int vbt_model_plan_steps(const vbt_model* m, vbt_plan_step_info* out, int cap, int* n) {
  if (!m || !n || cap < 0 || (cap > 0 && !out)) { set_error("vbt_model_plan_steps: bad argument"); return VBT_ERR_ARG; }
  const int ns = (int)m->steps.size();
  *n = ns;
  if (ns > cap) { set_error("plan steps: %d steps, buffer holds %d", ns, cap); return VBT_ERR_CAPACITY; }
  for (int i = 0; i < ns; i++) {
    const Step& s = m->steps[(size_t)i];
    vbt_plan_step_info& o = out[i];
    memset(&o, 0, sizeof(o));
    snprintf(o.family, sizeof(o.family), "%s", kFamilyName[s.family]);
    o.variant = s.variant;
    o.reads_frames = s.family == F_STEM || s.family == F_STEMBLK;
    o.image0_only = image0_only(s);
    o.n_members = (int)s.members.size();
    o.first_op = (int)m->ops.size(); o.last_op = -1;
    for_each_named_op(s, [&](int op) { o.first_op = std::min(o.first_op, op); o.last_op = std::max(o.last_op, op); });
    // the step of a chosen alternative this one is a copy of (finalize_plan); the launch merge_side_convs put together has none
    o.group = o.step = -1;
    for (size_t gi = 0; gi < m->groups.size() && o.group < 0; gi++) {
      const Alt& a = m->groups[gi].alts[(size_t)m->groups[gi].chosen];
      for (size_t si = 0; si < a.steps.size(); si++)
        if (a.steps[si].op == s.op && a.steps[si].family == s.family && a.steps[si].members.size() == s.members.size()) { o.group = (int)gi; o.step = (int)si; break; }
    }
  }
  return VBT_OK;
}

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
    if (img0 != 0 && image0_only(s)) { set_error("vbt_detect_range_async: plan step %d (%s) runs from image 0 only", i, kFamilyName[s.family]); return VBT_ERR_ARG; }
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
    unsigned char* h = m->out_host.get();
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

int vbt_model_write_tensor(vbt_model* m, int id, int B, const int8_t* host_in) {
  if (!m || !host_in || id < 0 || id >= (int)m->tensors.size() || id == m->hdr.input_tensor) { set_error("bad tensor id"); return VBT_ERR_ARG; }
  if (B < 1 || B > m->max_batch) { set_error("bad batch"); return VBT_ERR_CAPACITY; }
  if (!m->materialized[id]) { set_error("tensor %d lives only in LDS (fused away); create the model with VBT_MODEL_NO_FUSION to write it", id); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipDeviceSynchronize());
  VBT_HIP_CHECK(hipMemcpy(m->tptr[id], host_in, m->telems[id] * B, hipMemcpyHostToDevice));
  return VBT_OK;
}

}  // extern "C"
