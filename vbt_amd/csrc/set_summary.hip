// vbt_set_summary: the report of a set from the phases and rep metrics of one id.  Host code only - no device call, no kernel - so a
// process without a GPU can use it.
#include <cmath>

#include "common.h"

using namespace vbt;

extern "C" int vbt_set_summary(const double* phases6, const double* metrics8, int P, double stop_loss_pct, vbt_set_report* out, double* loss_pct,
                               int cap) {
  if (!out || P < 0 || cap < 0 || (P > 0 && (!phases6 || !metrics8)) || (cap > 0 && !loss_pct)) { set_error("vbt_set_summary: bad argument"); return VBT_ERR_ARG; }
  if (!std::isfinite(stop_loss_pct)) { set_error("vbt_set_summary: stop_loss_pct must be finite"); return VBT_ERR_ARG; }
  vbt_set_report r{};
  double best = -INFINITY, s_mv = 0.0, s_pv = 0.0, s_xd = 0.0;
  for (int i = 0; i < P; i++) {
    const double* ph = phases6 + (size_t)i * 6;
    const double* m = metrics8 + (size_t)i * VBT_REP_METRICS;
    if (ph[5] == 1.0) r.eccentric_s += ph[1] - ph[0];
    if (ph[5] != 0.0) continue;
    r.concentric_s += ph[1] - ph[0];
    const int k = ++r.n_reps;
    const double mv = m[VBT_RM_MV], pv = m[VBT_RM_PV];
    if (mv > best) { best = mv; r.best_rep = k; }
    const double loss = best > 0 ? 100.0 * (1.0 - mv / best) : 0.0;
    if (k <= cap) loss_pct[k - 1] = loss;
    if (stop_loss_pct > 0 && r.stop_rep == 0 && loss >= stop_loss_pct) r.stop_rep = k;
    s_mv += mv;
    s_pv += pv;
    s_xd += m[VBT_RM_X_DEV];
    if (pv > r.max_pv) r.max_pv = pv;
    r.last_mv = mv;
    r.loss_last_pct = loss;
  }
  if (r.n_reps > 0) {
    const double n = (double)r.n_reps;
    r.best_mv = best;
    r.mean_mv = s_mv / n;
    r.mean_pv = s_pv / n;
    r.mean_x_dev = s_xd / n;
  }
  *out = r;
  return VBT_OK;
}
