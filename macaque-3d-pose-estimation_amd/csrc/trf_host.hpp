// Host-only pieces of scipy 1.15.3's trf_no_bounds (optimize/_lsq/trf.py:401-540) for the drivers of the
// scipy-faithful solvers; oracle/trf.py states the same in numpy.  Nothing here makes a HIP call, so
// tests/trf_core_check.cpp runs it on a dense toy problem without a GPU:
//   * `regularize`, update_tr_radius, check_termination and the np.diff coefficients as plain functions, used by
//     optim_trf.hip (optim_points) and optim_possible.hip (optim_points_possible);
//   * solve_trust_region_2d, and TrfAnimal: one problem's state in the loop and the steps the loop takes between a
//     driver's launches.  A driver owns its launches, transfers and buffers, and fills the struct's inputs from its
//     own partials.  optim_trf.hip's driver runs on it; optim_possible.hip keeps its own statement of the loop and
//     reaches the 2-D solver through the exported mq_trust_region_2d (profiles/trf_core_ab.txt says why).
// lsmr's scalar core is lsmr_dev.hpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

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

// The 2-D trust-region subproblem (common.py solve_trust_region_2d; mq_trust_region_2d in optim_trf.hip is the
// exported wrapper with the argument checks).  np.roots of the quartic is replaced by its real roots found by
// bracketing between the critical points (the roots of the derivative, recursively) and bisecting; a root the
// polynomial only touches is not bracketed (numpy's companion eigenvalues of such a root are a near-real complex
// pair, excluded there too unless exactly real).
inline double poly_eval(const double* c, int d, double t) {
  double v = c[0];
  for (int i = 1; i <= d; ++i) v = v * t + c[i];
  return v;
}

inline void poly_real_roots(const double* cin, int din, std::vector<double>& out) {
  out.clear();
  int s = 0;
  while (s <= din && cin[s] == 0.0) ++s;  // leading zeros (np.roots strips them)
  const int d = din - s;
  if (d <= 0) return;
  const double* c = cin + s;
  if (d == 1) {
    out.push_back(-c[1] / c[0]);
    return;
  }
  if (d == 2) {
    const double disc = c[1] * c[1] - 4 * c[0] * c[2];
    if (disc < 0) return;
    const double q = -0.5 * (c[1] + (c[1] >= 0 ? std::sqrt(disc) : -std::sqrt(disc)));
    if (q != 0) {
      out.push_back(q / c[0]);
      out.push_back(c[2] / q);
    } else {
      out.push_back(0.0);
      out.push_back(0.0);
    }
    std::sort(out.begin(), out.end());
    return;
  }
  double dc[8];
  for (int i = 0; i < d; ++i) dc[i] = c[i] * (d - i);
  std::vector<double> crit;
  poly_real_roots(dc, d - 1, crit);
  double R = 0.0;
  for (int i = 1; i <= d; ++i) R = std::max(R, std::fabs(c[i] / c[0]));
  R += 1.0;
  std::vector<double> pts;
  pts.push_back(-R);
  for (double x : crit)
    if (x > -R && x < R) pts.push_back(x);
  pts.push_back(R);
  std::sort(pts.begin(), pts.end());
  for (size_t i = 0; i + 1 < pts.size(); ++i) {
    double a = pts[i], b = pts[i + 1];
    double fa = poly_eval(c, d, a), fb = poly_eval(c, d, b);
    if (fa == 0.0) {
      if (out.empty() || out.back() != a) out.push_back(a);
      continue;
    }
    if (fb == 0.0 || (fa < 0) == (fb < 0)) continue;
    for (int it = 0; it < 200; ++it) {
      const double m = 0.5 * (a + b);
      if (m <= a || m >= b) break;
      const double fm = poly_eval(c, d, m);
      if (fm == 0.0) {
        a = b = m;
        break;
      }
      if ((fm < 0) == (fa < 0)) {
        a = m;
        fa = fm;
      } else {
        b = m;
      }
    }
    out.push_back(0.5 * (a + b));
  }
  if (poly_eval(c, d, pts.back()) == 0.0) out.push_back(pts.back());
}

inline void solve_trust_region_2d(const double B[3], const double g[2], double Delta, double p[2]) {
  // cho_factor (upper) + cho_solve, p = -B^-1 g, if B is positive definite and p lies inside
  const double b00 = B[0], b01 = B[1], b11 = B[2];
  if (b00 > 0) {
    const double r00 = std::sqrt(b00), r01 = b01 / r00, s = b11 - r01 * r01;
    if (s > 0) {
      const double r11 = std::sqrt(s);
      const double y0 = g[0] / r00, y1 = (g[1] - r01 * y0) / r11;  // R^T y = g
      const double q1 = y1 / r11, q0 = (y0 - r01 * q1) / r00;      // R q = y
      const double pn0 = -q0, pn1 = -q1;
      if (pn0 * pn0 + pn1 * pn1 <= Delta * Delta) {
        p[0] = pn0;
        p[1] = pn1;
        return;
      }
    }
  }
  const double a = b00 * Delta * Delta, b = b01 * Delta * Delta, c = b11 * Delta * Delta;
  const double d = g[0] * Delta, f = g[1] * Delta;
  const double co[5] = {-b + d, 2 * (a - c + f), 6 * b, 2 * (-a + c + f), -b - d};
  std::vector<double> ts;
  poly_real_roots(co, 4, ts);
  if (ts.empty()) {
    // No sign change (numpy's companion eigenvalues would all be complex here, and scipy's argmin over an empty
    // set raises): the quartic's touching points -- critical points where it is zero to rounding -- are the
    // boundary candidates; failing those, the Cauchy point -Delta g / |g|.
    const double dco[4] = {4 * co[0], 3 * co[1], 2 * co[2], co[3]};
    std::vector<double> crit;
    poly_real_roots(dco, 3, crit);
    double scale = 0.0;
    for (double v : co) scale = std::max(scale, std::fabs(v));
    for (double tt : crit) {
      double mag = 0.0;  // |c_i t^(4-i)| summed: the rounding scale of the polynomial's value at t
      for (int i = 0; i <= 4; ++i) mag += std::fabs(co[i]) * std::pow(std::fabs(tt), 4 - i);
      if (std::fabs(poly_eval(co, 4, tt)) <= 64 * 2.220446049250313e-16 * (mag > 0 ? mag : scale)) ts.push_back(tt);
    }
    if (ts.empty()) {
      const double gn = std::sqrt(g[0] * g[0] + g[1] * g[1]);
      p[0] = gn > 0 ? -Delta * g[0] / gn : 0.0;
      p[1] = gn > 0 ? -Delta * g[1] / gn : -Delta;
      return;
    }
  }
  double best = std::numeric_limits<double>::infinity();
  p[0] = 0.0;
  p[1] = -Delta;
  bool any = false;
  for (double tt : ts) {
    const double q0 = Delta * (2 * tt / (1 + tt * tt)), q1 = Delta * ((1 - tt * tt) / (1 + tt * tt));
    const double val = 0.5 * (q0 * (b00 * q0 + b01 * q1) + q1 * (b01 * q0 + b11 * q1)) + (g[0] * q0 + g[1] * q1);
    if (!any || val < best) {
      best = val;
      p[0] = q0;
      p[1] = q1;
      any = true;
    }
  }
}

constexpr double TRF_XTOL = 1e-8, TRF_GTOL = 1e-8;  // least_squares' defaults (the reference sets ftol alone)

// One problem (animal) in the trf_no_bounds loop.  The driver writes cost .. areg after every evaluation it keeps
// (x0 and each accepted point) and B_S, g_S after each lsmr run; the rest is the loop's own.
struct TrfAnimal {
  bool running = true;  // the outer loop has not ended (trf.py:461-467)
  bool trial = false;   // inside the current iteration's trial loop (trf.py:496)
  int status = 0;       // scipy's: 0 max_nfev, 1 gtol, 2 ftol, 3 xtol, 4 ftol and xtol
  long long nfev = 1, njev = 1, max_nfev = 0;
  // at x: 0.5 |f|^2, |g|^2, max |g|, rows m, |x|, 0.5 |J g|^2
  double cost = 0.0, gnorm2 = 0.0, ginf = 0.0, rows = 0.0, xnorm = 0.0, areg = 0.0;
  double Delta = 0.0;
  double B_S[3] = {0.0, 0.0, 0.0}, g_S[2] = {0.0, 0.0};  // (J S)^T (J S) as b00, b01, b11; S^T g
  double pred = 0.0, actual = -1.0;                      // predicted and actual reduction of the last trial
  int lsmr_total = 0, lsmr_max = 0;

  // after the evaluation at x0 (trf.py:417-447)
  void start(long long max_nfev_) {
    Delta = xnorm == 0 ? 1.0 : xnorm;
    max_nfev = max_nfev_;
  }
  // the top of the outer loop: the gtol and evaluation-limit stops (trf.py:461-467).  True: the animal iterates.
  bool begin_iteration() {
    trial = false;
    actual = -1;
    if (!running) return false;
    if (ginf < TRF_GTOL) status = 1;
    if (status != 0 || nfev == max_nfev) return running = false;
    return trial = true;
  }
  // lsmr's damping (`regularize`, trf.py:480-484) and its maxiter min(m, n)
  void lsmr_setup(double nparam, double& damp, double& maxiter) const {
    damp = trf_regularize_damp(areg, gnorm2, Delta);
    maxiter = std::min(rows, nparam);
  }
  void record_lsmr(double itn) {
    const int it = (int)itn;
    lsmr_total += it;
    lsmr_max = std::max(lsmr_max, it);
  }
  // The next trial step in the subspace, p, with its predicted reduction (trf.py:497-503).  False: the animal's
  // trial loop is over.  (Delta goes to the solver unchecked, as scipy passes it.)
  bool propose_trial(double p[2]) {
    trial = trial && actual <= 0 && nfev < max_nfev;  // the trial loop's condition (trf.py:496)
    if (!trial) return false;
    solve_trust_region_2d(B_S, g_S, Delta, p);
    const double q = p[0] * (B_S[0] * p[0] + B_S[1] * p[1]) + p[1] * (B_S[1] * p[0] + B_S[2] * p[1]);
    pred = -(0.5 * q + (p[0] * g_S[0] + p[1] * g_S[1]));
    return true;
  }
  // the trial's outcome from |step| and the cost at the trial point (trf.py:508-531)
  void judge_trial(double step_norm, double cost_new, double ftol) {
    nfev++;
    if (!std::isfinite(cost_new)) {
      Delta = 0.25 * step_norm;
      actual = -1;
      return;
    }
    actual = cost - cost_new;
    double ratio;
    const double Dn = trf_update_tr_radius(Delta, actual, pred, step_norm, step_norm > 0.95 * Delta, ratio);
    const int term = trf_check_termination(actual, cost, step_norm, xnorm, ratio, ftol, TRF_XTOL);
    if (term) {
      status = term;
      trial = false;
      return;
    }
    Delta = Dn;
  }
  // after the trial loop (trf.py:533-540): true when the last trial is the new x; the driver then refills
  // cost .. areg from that trial's evaluation
  bool accept() {
    if (!running || !(actual > 0)) return false;
    njev++;
    return true;
  }
  // st[1..7]: final cost, iterations (njev - 1), status, nfev, njev, lsmr iterations in total, longest run (st[0],
  // the initial cost, is the driver's to write after start())
  void write_stats(double* st) const {
    st[1] = cost;
    st[2] = (double)(njev - 1);
    st[3] = status;
    st[4] = (double)nfev;
    st[5] = (double)njev;
    st[6] = lsmr_total;
    st[7] = lsmr_max;
  }
};

}  // namespace mq
