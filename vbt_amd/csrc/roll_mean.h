// pandas' rolling mean (roll_mean: Kahan add / remove, the run of equal values, the sign counts), as host + device statements: the
// rep analysis (rep_analysis.h) and the rep figure (figure_core.h) smooth their series with it, and a host program can too.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
#define __host__
#define __device__
#endif

namespace vbt {

struct RollMean {  // pandas roll_mean state (Kahan add / remove)
  double sum, c_add, c_rem, prev;
  long nobs, neg, same;
  __host__ __device__ void init() { sum = 0; c_add = 0; c_rem = 0; prev = __builtin_nan(""); nobs = 0; neg = 0; same = 0; }
  __host__ __device__ void add(double v) {
    nobs += 1;
    double y = v - c_add;
    double t = sum + y;
    c_add = (t - sum) - y;
    sum = t;
    if (__builtin_signbit(v)) neg += 1;
    if (v == prev) same += 1; else same = 1;
    prev = v;
  }
  __host__ __device__ void remove(double v) {
    nobs -= 1;
    double y = -v - c_rem;
    double t = sum + y;
    c_rem = (t - sum) - y;
    sum = t;
    if (__builtin_signbit(v)) neg -= 1;
  }
  __host__ __device__ double mean() const {
    double r = sum / (double)nobs;
    if (same >= nobs) r = prev;
    else if (neg == 0 && r < 0) r = 0.0;
    else if (neg == nobs && r > 0) r = 0.0;
    return r;
  }
};

}  // namespace vbt
