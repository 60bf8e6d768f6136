// Host-only pieces of scipy 1.15.3's trf_no_bounds that the drivers of the scipy-faithful solvers share
// (optim_trf.hip for optim_points, optim_possible.hip for optim_points_possible); oracle/trf.py states the same
// in numpy.  The 2-D subproblem itself is mq_trust_region_2d (optim_trf.hip).
#pragma once
#include <cmath>

namespace mq {

// np.diff's coefficients of order n: row i = sum_m c[m] x[i + m]
inline void trf_diff_coefficients(int n, double c[4]) {
  c[0] = c[1] = c[2] = c[3] = 0.0;
  int binom = 1;
  for (int m = 0; m <= n; ++m) {
    c[m] = (((n - m) & 1) ? -1.0 : 1.0) * binom;
    binom = binom * (n - m) / (m + 1);
  }
}

// `regularize` (trf.py:480-484): lsmr's damping from the 1-D quadratic along -g inside the trust region;
// a = 0.5 |J g|^2, gnorm2 = |g|^2
inline double trf_regularize_damp(double a, double gnorm2, double Delta) {
  const double bq = -gnorm2;
  const double to_tr = Delta / std::sqrt(gnorm2);
  double ag = 0.0 * (a * 0.0 + bq);
  const double y1 = to_tr * (a * to_tr + bq);
  if (y1 < ag) ag = y1;
  if (a != 0) {
    const double ext = -0.5 * bq / a;
    if (0 < ext && ext < to_tr) {
      const double y2 = ext * (a * ext + bq);
      if (y2 < ag) ag = y2;
    }
  }
  const double reg = -ag / (Delta * Delta);
  return std::sqrt(0.0 + reg);
}

// common.py update_tr_radius: the new radius, and the ratio of actual to predicted reduction
inline double trf_update_tr_radius(double Delta, double actual, double predicted, double step_norm, bool bound_hit,
                                   double& ratio) {
  if (predicted > 0) ratio = actual / predicted;
  else if (predicted == actual && actual == 0) ratio = 1;
  else ratio = 0;
  if (ratio < 0.25) return 0.25 * step_norm;
  if (ratio > 0.75 && bound_hit) return Delta * 2.0;
  return Delta;
}

// common.py check_termination: 0 = go on, else scipy's status (2 ftol, 3 xtol, 4 both)
inline int trf_check_termination(double dF, double F, double dx_norm, double x_norm, double ratio, double ftol,
                                 double xtol) {
  const bool ft = dF < ftol * F && ratio > 0.25;
  const bool xt = dx_norm < xtol * (xtol + x_norm);
  return (ft && xt) ? 4 : ft ? 2 : xt ? 3 : 0;
}

}  // namespace mq
