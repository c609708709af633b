// Wave-parallel linear assignment with scipy's tie rule, shared by the trackers (step_phases.h: gate_and_assign of both steps;
// ocsort_step.h: the second association) and the detector evaluation (evaluate.hip).  Device code only; one wavefront (64 lanes) per problem.
#pragma once
#include <hip/hip_runtime.h>

namespace vbt {

constexpr int MAXT = 64;  // rows / columns of an assignment problem (tracks per clip, boxes per image)

// ------------------------------------------------------------------------------------------
// wave-parallel rectangular linear assignment (nr rows <= nc cols <= 64, lanes = columns).
// cost(i, j) = tr ? C[j*ld + i] : C[i*ld + j].  Writes row2col[0..nr).
// OC-SORT's second association compares detections with never-observed trackers whose placeholder
// boxes are identical, so exact cost ties are routine and the result depends on the solver's tie
// rule.  This is therefore a faithful lane-parallel port of the solver the oracle uses
// [EXTERNAL: scipy.optimize.linear_sum_assignment = Crouse's shortest augmenting path,
// rectangular_lsap.cpp]: same `remaining` order (reverse fill, swap-with-last removal), same
// selection rule (lowest cost; among equals the LAST unassigned column scanned, else the first),
// same dual updates and the same floating-point expression ((minVal + c) - u) - v.
// ------------------------------------------------------------------------------------------
// Wave-wide reductions on the DPP path (row shifts inside rows of 16 lanes, then the GFX9 row broadcasts; lane 63 ends with the
// result, which comes back over the scalar path): six dependent steps of two or three VALU instructions instead of six shuffles
// through the LDS crossbar per 32-bit half.  The values met are the ones the shuffles met, so every result is unchanged.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_f64(double old, double x) {
  const unsigned long long o = (unsigned long long)__double_as_longlong(old), v = (unsigned long long)__double_as_longlong(x);
  const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)o, (int)(unsigned)v, CTRL, ROWMASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(unsigned)(o >> 32), (int)(unsigned)(v >> 32), CTRL, ROWMASK, 0xf, false);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo));
}
__device__ __forceinline__ double bcast63_f64(double x) {
  const unsigned long long v = (unsigned long long)__double_as_longlong(x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double wave_min_f64(double x) {
  const double I = __builtin_inf();
  x = fmin(x, dpp_f64<0x111, 0xf>(I, x));
  x = fmin(x, dpp_f64<0x112, 0xf>(I, x));
  x = fmin(x, dpp_f64<0x114, 0xf>(I, x));
  x = fmin(x, dpp_f64<0x118, 0xf>(I, x));
  x = fmin(x, dpp_f64<0x142, 0xa>(I, x));
  x = fmin(x, dpp_f64<0x143, 0xc>(I, x));
  return bcast63_f64(x);
}
__device__ __forceinline__ double wave_max_f64(double x) {
  const double I = -__builtin_inf();
  x = fmax(x, dpp_f64<0x111, 0xf>(I, x));
  x = fmax(x, dpp_f64<0x112, 0xf>(I, x));
  x = fmax(x, dpp_f64<0x114, 0xf>(I, x));
  x = fmax(x, dpp_f64<0x118, 0xf>(I, x));
  x = fmax(x, dpp_f64<0x142, 0xa>(I, x));
  x = fmax(x, dpp_f64<0x143, 0xc>(I, x));
  return bcast63_f64(x);
}
__device__ __forceinline__ int wave_max_i32(int x) {
  constexpr int I = -2147483647 - 1;
  x = max(x, __builtin_amdgcn_update_dpp(I, x, 0x111, 0xf, 0xf, false));
  x = max(x, __builtin_amdgcn_update_dpp(I, x, 0x112, 0xf, 0xf, false));
  x = max(x, __builtin_amdgcn_update_dpp(I, x, 0x114, 0xf, 0xf, false));
  x = max(x, __builtin_amdgcn_update_dpp(I, x, 0x118, 0xf, 0xf, false));
  x = max(x, __builtin_amdgcn_update_dpp(I, x, 0x142, 0xa, 0xf, false));
  x = max(x, __builtin_amdgcn_update_dpp(I, x, 0x143, 0xc, 0xf, false));
  return __builtin_amdgcn_readlane(x, 63);
}

#ifdef VBT_NO_LAP_SMALL
__device__ __forceinline__ bool lap_small_off() { return true; }
#else
__device__ __forceinline__ bool lap_small_off() { return false; }
#endif

struct LapShared {
  double u[MAXT];
  double spc[MAXT];
  int col4row[MAXT];
  int row4col[MAXT];
  int path[MAXT];
  int remaining[MAXT];
};

// The same solver for 2..4 rows (a frame of the reference holds at most 3 plates; the second association sees even fewer rows) with
// every array in registers: the per-row state (duals u, col4row) is wave-uniform, the per-column state (dual v, row4col, path,
// shortest path cost, position in `remaining`) belongs to the column's lane, `remaining[index]` is "the lane whose position is
// index" (a ballot), and a value of another lane comes over the scalar path (v_readlane).  No LDS array, no barrier inside; the
// arithmetic - ((minVal + c) - u) - v, the dual updates, the tie rule - is the general solver's, statement for statement.
__device__ __forceinline__ double readlane_f64(double x, int l) {
  const unsigned long long v = (unsigned long long)__double_as_longlong(x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ void lap_small(const double* C, int ld, bool tr, int nr, int nc, int* row2col, int lane) {
  const double INF = __builtin_inf();
  const bool col = lane < nc;
  double cst[4];
#pragma unroll
  for (int q = 0; q < 4; q++) cst[q] = (col && q < nr) ? (tr ? C[lane * ld + q] : C[q * ld + lane]) : INF;
  double u[4] = {0.0, 0.0, 0.0, 0.0};
  int c4r[4] = {-1, -1, -1, -1};
  double v = 0.0;
  int r4c = -1, path = -1;
  auto sel_d = [](const double a[4], int i) { return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3]; };
  for (int cur = 0; cur < nr; cur++) {
    double minVal = 0.0;
    int num_rem = nc;
    int pos = col ? nc - 1 - lane : -1;
    double spc = INF;
    unsigned sr = 0u;
    int i = cur, sink = -1;
    while (sink == -1) {
      sr |= 1u << i;
      const double ui = sel_d(u, i);
      const bool active = col && pos >= 0;
      if (active) {
        const double c = sel_d(cst, i);
        const double r = ((minVal + c) - ui) - v;
        if (r < spc) { path = i; spc = r; }
      }
      const double lowest = wave_min_f64(active ? spc : INF);
      const bool cand = active && spc == lowest;
      const unsigned long long un = __ballot(cand && r4c == -1);
      int key;  // choose: unassigned candidates -> max position, else min position
      if (un) key = (cand && r4c == -1) ? pos : -1;
      else key = cand ? -pos : -(1 << 20);
      key = wave_max_i32(key);
      const int index = un ? key : -key;
      minVal = lowest;
      const int j = __ffsll((long long)__ballot(active && pos == index)) - 1;     // remaining[index]
      const int jrow = __builtin_amdgcn_readlane(r4c, j);
      if (jrow == -1) sink = j; else i = jrow;
      num_rem -= 1;
      const int jl = __ffsll((long long)__ballot(active && pos == num_rem)) - 1;  // remaining[num_rem]
      if (lane == j) pos = -1;
      if (lane == jl && jl != j) pos = index;
    }
    // ---- dual updates ----
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (q >= nr) continue;
      if (q == cur) u[q] += minVal;
      else if ((sr >> q) & 1u) u[q] += minVal - readlane_f64(spc, c4r[q]);
    }
    if (col && pos < 0) v -= minVal - spc;
    // ---- augment ----
    int j = sink;
    while (true) {
      const int ii = __builtin_amdgcn_readlane(path, j);
      if (lane == j) r4c = ii;
      const int t = ii == 0 ? c4r[0] : ii == 1 ? c4r[1] : ii == 2 ? c4r[2] : c4r[3];
#pragma unroll
      for (int q = 0; q < 4; q++) if (q == ii) c4r[q] = j;
      j = t;
      if (ii == cur) break;
    }
  }
  if (lane < nr) row2col[lane] = lane == 0 ? c4r[0] : lane == 1 ? c4r[1] : lane == 2 ? c4r[2] : c4r[3];
  __syncthreads();
}

__device__ void lap_solve(const double* C, int ld, bool tr, int nr, int nc, int* row2col, LapShared& S, int lane) {
  const double INF = __builtin_inf();
  if (nr >= 2 && nr <= 4 && !lap_small_off()) { lap_small(C, ld, tr, nr, nc, row2col, lane); return; }
  if (nr == 1) {
    // One row (OC-SORT's second association usually has one unmatched detection): the first augmenting path of the solver
    // ends at the cheapest column; among equal costs it takes the LAST one it scans, and it scans remaining[] = nc-1 ... 0,
    // i.e. the lowest column index.  No dual update can change a one-row result.
    double c = lane < nc ? (tr ? C[lane * ld] : C[lane]) : INF;
    const double lowest = wave_min_f64(c);
    const unsigned long long cand = __ballot(lane < nc && c == lowest);
    if (lane == 0) row2col[0] = __ffsll((long long)cand) - 1;
    __syncthreads();
    return;
  }
  double v = 0.0;
  if (lane < nr) { S.u[lane] = 0.0; S.col4row[lane] = -1; }
  if (lane < nc) { S.row4col[lane] = -1; S.path[lane] = -1; }
  __syncthreads();
  for (int cur = 0; cur < nr; cur++) {
    // ---- augmenting_path ----
    double minVal = 0.0;
    int num_rem = nc;
    int pos = lane < nc ? nc - 1 - lane : -1;   // remaining[it] = nc - it - 1
    if (lane < nc) S.remaining[nc - 1 - lane] = lane;
    double spc = INF;
    unsigned long long sr = 0ull;
    int i = cur, sink = -1;
    __syncthreads();
    while (sink == -1) {
      sr |= 1ull << i;
      const double ui = S.u[i];
      const bool active = lane < nc && pos >= 0;
      const int r4c = lane < nc ? S.row4col[lane] : 0;
      if (active) {
        double c = tr ? C[lane * ld + i] : C[i * ld + lane];
        double r = ((minVal + c) - ui) - v;
        if (r < spc) { S.path[lane] = i; spc = r; }
      }
      const double lowest = wave_min_f64(active ? spc : INF);
      const bool cand = active && spc == lowest;
      const unsigned long long un = __ballot(cand && r4c == -1);
      int key;  // choose: unassigned candidates -> max position, else min position
      if (un) key = (cand && r4c == -1) ? pos : -1;
      else key = cand ? -pos : -(1 << 20);
      key = wave_max_i32(key);
      const int index = un ? key : -key;
      minVal = lowest;
      const int j = S.remaining[index];
      const int jrow = S.row4col[j];
      __syncthreads();
      if (jrow == -1) sink = j; else i = jrow;
      // SC[j] = true ; remaining[index] = remaining[--num_remaining]
      num_rem -= 1;
      const int jl = S.remaining[num_rem];
      __syncthreads();
      if (lane == j) pos = -1;
      if (lane == jl && jl != j) pos = index;
      if (lane == 0) S.remaining[index] = jl;
      __syncthreads();
    }
    // ---- dual updates ----
    if (lane < nc) S.spc[lane] = spc;
    __syncthreads();
    if (lane < nr) {
      if (lane == cur) S.u[lane] += minVal;
      else if ((sr >> lane) & 1ull) S.u[lane] += minVal - S.spc[S.col4row[lane]];
    }
    if (lane < nc && pos < 0) v -= minVal - spc;
    __syncthreads();
    // ---- augment ----
    if (lane == 0) {
      int j = sink;
      while (true) {
        int ii = S.path[j];
        S.row4col[j] = ii;
        int t = S.col4row[ii];
        S.col4row[ii] = j;
        j = t;
        if (ii == cur) break;
      }
    }
    __syncthreads();
  }
  if (lane < nr) row2col[lane] = S.col4row[lane];
  __syncthreads();
}

}  // namespace vbt
