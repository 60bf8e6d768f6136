// Host check of the mode-2 derivative blocks of csrc/bundle_dev.hpp (the CameraGroup.bundle_adjust
// parametrisation: rvec, tvec, f, k1, k2 per camera, a model per camera): ba_obs_jac<2> against central
// differences of ba_obs_res<2>, for each camera model, at generic points and at r -> 0 (the point on the optical
// axis, where the fisheye model switches to theta_d / r = 1).  Built by tests/test_cg_ba_ref.py with
// -fsanitize=address,undefined and run directly; prints the largest error per model and returns non-zero on failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "bundle_dev.hpp"

using namespace mq;

namespace {

double urand() { return (double)rand() / RAND_MAX * 2.0 - 1.0; }

void residual(const double* row, const double* X, const double* ob, double* r) {
  double R[9];
  ba_rodrigues(row, R);
  ba_obs_res<2>(row, R, X, ob, r);
}

// largest |analytic - central difference| over the 2 x 9 and 2 x 3 blocks, relative to max(1, |entry|)
double check(const double* row, const double* X, bool* finite) {
  const double ob[2] = {3.0, -2.0};
  double R[9], dR[27], r[2], A[2 * BA_GP], B[6], r0[2];
  ba_rotation_jac(row, R, dR);
  ba_obs_jac<2>(row, R, dR, X, ob, r, A, B);
  residual(row, X, ob, r0);
  double worst = fmax(fabs(r[0] - r0[0]), fabs(r[1] - r0[1]));
  for (int k = 0; k < 2 * BA_GP + 6; ++k)
    if (!std::isfinite(k < 2 * BA_GP ? A[k] : B[k - 2 * BA_GP])) *finite = false;
  for (int p = 0; p < BA_GP + 3; ++p) {
    double rowp[BA_GROW], Xp[3], rp[2], rm[2];
    const bool cam = p < BA_GP;
    const double at = cam ? row[p] : X[p - BA_GP];
    const double h = 1e-6 * fmax(1.0, fabs(at));
    for (int sgn = 0; sgn < 2; ++sgn) {
      for (int k = 0; k < BA_GROW; ++k) rowp[k] = row[k];
      for (int k = 0; k < 3; ++k) Xp[k] = X[k];
      (cam ? rowp[p] : Xp[p - BA_GP]) = at + (sgn ? -h : h);
      residual(rowp, Xp, ob, sgn ? rm : rp);
    }
    for (int e = 0; e < 2; ++e) {
      const double fd = (rp[e] - rm[e]) / (2.0 * h);
      const double an = cam ? A[e * BA_GP + p] : B[e * 3 + (p - BA_GP)];
      worst = fmax(worst, fabs(an - fd) / fmax(1.0, fabs(an)));
    }
  }
  return worst;
}

void make_row(int model, double* row) {
  for (int k = 0; k < BA_GROW; ++k) row[k] = 0.0;
  for (int k = 0; k < 3; ++k) row[k] = 0.4 * urand();
  row[3] = 50.0 * urand(), row[4] = 50.0 * urand(), row[5] = 1500.0 + 200.0 * urand();
  row[6] = 900.0 + 100.0 * urand();
  row[7] = 0.1 * urand();
  row[8] = 0.05 * urand();
  row[BA_GP] = model;
  double* g = row + BA_GP + 1;
  if (model == BA_CAM_OMNIDIR) {
    g[0] = 1100.0 + 50.0 * urand(), g[1] = 0.5 * urand(), g[2] = 640.0 + 10.0 * urand();
    g[3] = 1100.0 + 50.0 * urand(), g[4] = 512.0 + 10.0 * urand(), g[5] = 1.0 + 0.3 * urand();
    g[6] = 0.2 * urand(), g[7] = 0.1 * urand(), g[8] = 0.01 * urand(), g[9] = 0.01 * urand();
  } else {
    g[0] = 640.0 + 10.0 * urand(), g[1] = 512.0 + 10.0 * urand();
  }
}

}  // namespace

int main() {
  srand(7);
  const char* names[3] = {"omnidir", "pinhole", "fisheye"};
  int bad = 0;
  for (int model = 0; model < 3; ++model) {
    double generic = 0.0, axis = 0.0;
    bool finite = true;
    for (int it = 0; it < 50; ++it) {
      double row[BA_GROW], X[3] = {600.0 * urand(), 600.0 * urand(), 300.0 * urand()};
      make_row(model, row);
      generic = fmax(generic, check(row, X, &finite));
      // r -> 0: the world point that lands on the optical axis, X = R^T ((0, 0, z) - t), exactly and 1e-9 off it
      double R[9];
      ba_rodrigues(row, R);
      const double z = 1000.0 + 300.0 * urand();
      const double q[3] = {-row[3], -row[4], z - row[5]};
      for (int k = 0; k < 3; ++k) X[k] = R[k] * q[0] + R[3 + k] * q[1] + R[6 + k] * q[2];
      axis = fmax(axis, check(row, X, &finite));
      if (it == 0) {  // exactly on the axis: the identity rotation, so that Xc = (0, 0, z) has no rounding
        row[0] = row[1] = row[2] = 0.0;
        const double X0[3] = {-row[3], -row[4], z - row[5]};
        axis = fmax(axis, check(row, X0, &finite));
      }
    }
    // central differences with h = 1e-6 |x|: truncation ~ h^2 f''', rounding ~ 1e-16 |r| / h ~ 1e-7 relative
    const bool ok = finite && generic < 2e-5 && axis < 2e-5;
    printf("%s: generic %.3e axis %.3e finite %d %s\n", names[model], generic, axis, (int)finite, ok ? "ok" : "FAIL");
    bad += !ok;
  }
  return bad ? 1 : 0;
}
