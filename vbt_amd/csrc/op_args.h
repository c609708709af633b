// Argument structs of the single-op kernels (k_pointwise.hip, k_ops.hip, k_postprocess.hip) and what selects their instantiations:
// what launch_step (detector.hip) fills and the launchers (launchers.h) take.  No kernel body lives here.
#pragma once
#include "dev_types.h"

namespace vbt {

// ---- pointwise conv (k_pointwise.hip) ----
// Epilogue: requantisation, optionally followed by the block's residual ADD (integer, XNNPACK qs8-vadd) with `res`.
struct ResArgs {
  const int8_t* res;  // nullptr: no residual; else the second ADD input, same [M][N] layout as the output
  AddQ q;
};
// which kernel form and instantiation a launch runs (resolve_pw's result, detector_model.h, embeds it)
enum PwForm { PW_A, PW_B, PW_C, PW_D, PW_E, PW_F };
struct PwKernel {
  PwForm form = PW_B;
  int ms = 1;    // pixel groups per wave (PW_A, PW_C) / 64-pixel groups per workgroup (PW_D, PW_E, PW_F): 1 or 2
  int nbt = 1;   // PW_B: 64-channel blocks per wave, 1 .. 4
  int ntl = 0;   // PW_F: live tiles of a tile-major part-filled last block (wp = pack_weights64_tail's panel); 0: block-major
};
constexpr int PW_F_MAX_NB = 6;   // output blocks whose accumulators one workgroup of the all-blocks form holds (N <= 384)
// the (output blocks, live tiles of the last block) the all-blocks form is built for with a tile-major last block (variants 9 / 10): the
// large-K projections of the shipped models - Lite0 80 = 64 + 16 and 112 = 64 + 48, Lite2 88 = 64 + 24, 120 = 64 + 56 (four tiles, the
// last one part-filled), 208 = 3 x 64 + 16 and 352 = 5 x 64 + 32.  Another width needs a line here and one in launch_pw (k_pointwise.hip).
static inline bool pw_f_tail_built(int NB, int ntl) { return (NB == 2 && ntl >= 1 && ntl <= 4) || (NB == 4 && ntl == 1) || (NB == 6 && ntl == 2); }
struct PwArgs {
  const int8_t* x;   // [M][K]
  const v4i* wp;     // packed weights [nb][ks][t][lane] x 16 bytes (pack_weights64; PwKernel::ntl > 0: pack_weights64_tail)
  Epi e;
  ResArgs ra;
  int8_t* out;       // [M][N]
  long M;
  int K, KS64, N, NB;
  int nb_per_y;      // PW_A: output blocks per grid row
};

// Several independent pointwise convs in one launch (pw_multi_kernel): as many as merge_side_convs (planner.hip) puts together
constexpr int PW_MERGE_MAX = 8;
struct PwProb {
  const int8_t* x;
  const v4i* wp;
  const int* bias;
  const float* mult;
  int8_t* out;
  Rq rq;
  int M, K, KS, N, NB;     // M = pixels of the whole batch (chain: of one image)
  // chain (pool1 != nullptr): conv output H x W per image, pooled to H1 x W1 (pad pt1 / pl1) and again to H2 x W2
  int8_t* pool1;
  int8_t* pool2;
  int H, W, H1, W1, pt1, pl1, H2, W2, pt2, pl2;
};
struct PwMulti {
  int n;
  int start[PW_MERGE_MAX + 1];   // first workgroup of every problem
  PwProb p[PW_MERGE_MAX];
};

// ---- stem conv, depthwise walkers, ADD, max pool, nearest-neighbour resize (k_ops.hip) ----
struct StemArgs {
  const uint8_t* frames;   // [B][H][W][3]
  const long* wp;
  Epi e;
  int8_t* out;             // [M][N], M = B * OH * OW
  long M;
  int H, W, OH, OW, N, pad_t, pad_l, zx;
};
struct DwArgs {
  const int8_t* x;
  const float* wf;         // weights as float [k*k][C]
  Epi e;
  int8_t* out;
  long total;              // lanes of the launch
  int H, W, C, OH, OW, pad_t, pad_l;
  unsigned pad4;           // out-of-image input byte (uint8 domain) x 4
  int rows, nseg;          // column walker: output rows per lane, row segments per map; rows == 0: the row form (dw_kernel)
};
struct MapArgs {           // max pool 3x3/2 and nearest-neighbour resize: one lane per 4 channels of an output pixel
  const int8_t* x;
  int8_t* out;
  long total;
  int H, W, C, OH, OW, pad_t, pad_l;   // (pads: max pool only)
};

// ---- TFLite_Detection_PostProcess (k_postprocess.hip) ----
struct PostArgs {
  const int8_t* cls[5];
  const int8_t* box[5];
  int base[6];         // first anchor index of each level, base[5] = A
  const float* anchors;  // [A][4] ycenter, xcenter, h, w
  // device tables built at model load from the container's (vbt_amd/quant.py): score f32[256] indexed by RANK byte + 128 |
  // dq f64[256] | ex f64[256] indexed by box byte + 128 | rank int8[256] indexed by class byte + 128.
  // rank byte: class bytes with EQUAL scores (plateaus of the LOGISTIC table) share one, higher score = higher rank byte,
  // so that sorting by (rank desc, anchor asc) is the reference's stable sort on the float scores.
  const unsigned char* tables;
  int A, max_det, qmin;  // qmin: lowest RANK byte whose score >= nms_score_threshold (128 = none)
  float iou_thr;
  int C;                 // class columns per anchor: the class tensors are [h][w][anchors_per_location * C], anchor a's bytes are contiguous
};

}  // namespace vbt
