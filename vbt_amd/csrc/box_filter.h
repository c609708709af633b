// The box filter and box geometry under both trackers' steps: the 7-state constant-velocity Kalman filter on (cx, cy, s, r) in its
// decoupled closed form (tracker.hip's header comment), state -> box, IoU.  Device code.  All arithmetic is FP64 with contraction off in
// the op order of the numpy formulation: that order is the contract with the references, nothing here may be reordered or re-associated.
#pragma once
#include "tracker_state.h"

namespace vbt {

// The filter state proper as a LOCAL value: x, the three 2x2 covariance blocks and the variance of r.  predict / update work on a copy
// in registers that is loaded from the track once and stored back once: through a `Trk&` into LDS or global memory the compiler has to
// assume that every store may change what the next load reads (the detection, the observation history and the state are all plain
// double arrays), so the filter arithmetic ran as a chain of store -> wait -> load.
struct KfCore {
  double x[7];
  double B[3][4];
  double Pr;
};
__device__ __forceinline__ void core_load(KfCore& c, const Trk& k) {
#pragma unroll
  for (int i = 0; i < 7; i++) c.x[i] = k.x[i];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) c.B[i][j] = k.B[i][j];
  c.Pr = k.Pr;
}
__device__ __forceinline__ void core_store(Trk& k, const KfCore& c) {
#pragma unroll
  for (int i = 0; i < 7; i++) k.x[i] = c.x[i];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) k.B[i][j] = c.B[i][j];
  k.Pr = c.Pr;
}
__device__ __forceinline__ void kf_predict(KfCore& k, double q44, double q66) {
#pragma unroll
  for (int i = 0; i < 3; i++) k.x[i] = k.x[i] + k.x[i + 4];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    double a = k.B[i][0], b = k.B[i][1], c = k.B[i][2], d = k.B[i][3];
    double qv = i == 2 ? q66 : q44;
    k.B[i][0] = ((a + c) + (b + d)) + 1.0;
    k.B[i][1] = (b + d) + 0.0;
    k.B[i][2] = (c + d) + 0.0;
    k.B[i][3] = d + qv;
  }
  k.Pr = k.Pr + 1.0;
}

__device__ __forceinline__ void kf_update_math(KfCore& k, const double z[4]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double Rc = i == 2 ? 10.0 : 1.0;
    double a = k.B[i][0], b = k.B[i][1], c = k.B[i][2], d = k.B[i][3];
    double y = z[i] - k.x[i];
    double S = a + Rc;
    double si = 1.0 / S;
    double kp = a * si, kv = c * si;
    k.x[i] = k.x[i] + kp * y;
    k.x[i + 4] = k.x[i + 4] + kv * y;
    double omk = 1.0 - kp, nkv = 0.0 - kv;
    double M00 = omk * a, M01 = omk * b, M10 = nkv * a + c, M11 = nkv * b + d;
    double N00 = M00 * omk, N01 = M00 * nkv + M01, N10 = M10 * omk, N11 = M10 * nkv + M11;
    double KRp = kp * Rc, KRv = kv * Rc;
    k.B[i][0] = N00 + KRp * kp;
    k.B[i][1] = N01 + KRp * kv;
    k.B[i][2] = N10 + KRv * kp;
    k.B[i][3] = N11 + KRv * kv;
  }
  double y = z[3] - k.x[3];
  double S = k.Pr + 10.0;
  double si = 1.0 / S;
  double kk = k.Pr * si;
  k.x[3] = k.x[3] + kk * y;
  double omk = 1.0 - kk;
  k.Pr = (omk * k.Pr) * omk + (kk * 10.0) * kk;
}

__device__ inline void x_to_bbox(const double* x, double o[4]) {
  double w = sqrt(x[2] * x[3]);
  double h = x[2] / w;
  o[0] = x[0] - w / 2.0; o[1] = x[1] - h / 2.0; o[2] = x[0] + w / 2.0; o[3] = x[1] + h / 2.0;
}

__device__ inline double iou_xyxy(const double* a, const double* b) {
  double xx1 = fmax(a[0], b[0]), yy1 = fmax(a[1], b[1]), xx2 = fmin(a[2], b[2]), yy2 = fmin(a[3], b[3]);
  double w = fmax(0.0, xx2 - xx1), h = fmax(0.0, yy2 - yy1);
  double wh = w * h;
  return wh / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - wh);
}

}  // namespace vbt
