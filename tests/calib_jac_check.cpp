// Host check of csrc/calib_dev.hpp: cal_obs_jac against central differences of cal_project for both models (every
// intrinsic slot and the six pose columns, at 50 generic points, on the optical axis and at rvec = 0), and the
// closed-form starts on noise-free points (known answers).  Prints one "<name> ok" line per check and the largest
// relative Jacobian error; exit status 1 on a failure.  Built by tests/test_calib_ref.py with
// -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "calib_dev.hpp"

using namespace mq;

static std::mt19937_64 rng(7);
static double uni(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }

template <int MODEL>
static void project(const double* prm, const double* X, double* uv) {
  double R[9];
  ba_rodrigues(prm + CAL_NI, R);
  cal_project<MODEL>(prm, R, prm + CAL_NI + 3, X, uv[0], uv[1]);
}

// largest |analytic - numeric| / max(|numeric|, column scale) over the 2 x 16 Jacobian at one point
template <int MODEL>
static double jac_error(const double* prm, const double* X) {
  double R[9], dR[27], r[2], A[2 * CAL_NC];
  const double ob[2] = {0.0, 0.0};
  ba_rotation_jac(prm + CAL_NI, R, dR);
  cal_obs_jac<MODEL>(prm, R, dR, prm + CAL_NI + 3, X, ob, r, A);
  double uv[2];
  project<MODEL>(prm, X, uv);
  if (r[0] != uv[0] || r[1] != uv[1]) {
    std::printf("residual of cal_obs_jac differs from cal_project: %.17g %.17g vs %.17g %.17g\n", r[0], r[1], uv[0], uv[1]);
    return 1.0;
  }
  double worst = 0.0;
  for (int c = 0; c < CAL_NC; ++c) {
    if (MODEL == CAL_PINHOLE && c == 9) {
      if (A[c] != 0.0 || A[CAL_NC + c] != 0.0) return 1.0;
      continue;
    }
    double p[CAL_NC], m[CAL_NC];
    for (int k = 0; k < CAL_NC; ++k) p[k] = m[k] = prm[k];
    // the projection is linear in every intrinsic slot but xi, so a wide step costs nothing there; xi, rvec
    // and tvec take the step that balances truncation (h^2) against rounding (1e-16 * 2000 px / h)
    const bool is_xi = MODEL == CAL_OMNIDIR && c == 5;
    const double h = c >= CAL_NI + 3 ? 1e-2 : (c >= CAL_NI || is_xi) ? 1e-5 : 1e-2 * std::fmax(1.0, std::fabs(prm[c]));
    p[c] += h, m[c] -= h;
    double up[2], um[2];
    project<MODEL>(p, X, up);
    project<MODEL>(m, X, um);
    double col = 0.0, num[2];
    for (int row = 0; row < 2; ++row) {
      num[row] = (up[row] - um[row]) / (2.0 * h);
      col = std::fmax(col, std::fabs(num[row]));
    }
    for (int row = 0; row < 2; ++row)
      worst = std::fmax(worst, std::fabs(A[row * CAL_NC + c] - num[row]) / std::fmax(col, 1e-3));
  }
  return worst;
}

static void generic_params(int model, double* prm) {
  if (model == CAL_PINHOLE) {
    const double k[CAL_NI] = {1800 + uni(-50, 50), 1790 + uni(-50, 50), 1020 + uni(-20, 20), 770 + uni(-20, 20),
                              uni(-0.2, 0.2), uni(-0.1, 0.1), uni(-0.01, 0.01), uni(-0.01, 0.01), uni(-0.05, 0.05), 0};
    for (int i = 0; i < CAL_NI; ++i) prm[i] = k[i];
  } else {
    const double k[CAL_NI] = {3700 + uni(-50, 50), 3690 + uni(-50, 50), uni(-2, 2), 1020 + uni(-20, 20), 770 + uni(-20, 20),
                              uni(0.8, 4.4), uni(-0.2, 0.2), uni(-0.1, 0.1), uni(-0.01, 0.01), uni(-0.01, 0.01)};
    for (int i = 0; i < CAL_NI; ++i) prm[i] = k[i];
  }
  for (int i = 0; i < 3; ++i) prm[CAL_NI + i] = uni(-0.6, 0.6);
  prm[CAL_NI + 3] = uni(-100, 100), prm[CAL_NI + 4] = uni(-100, 100), prm[CAL_NI + 5] = uni(450, 900);
}

template <int MODEL>
static bool check_model(const char* name, double& worst_all) {
  double worst = 0.0;
  for (int i = 0; i < 50; ++i) {  // generic points
    double prm[CAL_NC];
    generic_params(MODEL, prm);
    const double X[3] = {uni(-150, 150), uni(-100, 100), uni(-50, 50)};
    worst = std::fmax(worst, jac_error<MODEL>(prm, X));
  }
  {  // on the optical axis: X = -R^T t + R^T (0, 0, z)  =>  Xc = (0, 0, z)
    double prm[CAL_NC], R[9];
    generic_params(MODEL, prm);
    ba_rodrigues(prm + CAL_NI, R);
    const double d[3] = {-prm[CAL_NI + 3], -prm[CAL_NI + 4], 0.0};
    const double X[3] = {R[0] * d[0] + R[3] * d[1] + R[6] * d[2], R[1] * d[0] + R[4] * d[1] + R[7] * d[2],
                         R[2] * d[0] + R[5] * d[1] + R[8] * d[2]};
    worst = std::fmax(worst, jac_error<MODEL>(prm, X));
  }
  {  // rvec = 0: the first-order branch of ba_rodrigues
    double prm[CAL_NC];
    generic_params(MODEL, prm);
    prm[CAL_NI] = prm[CAL_NI + 1] = prm[CAL_NI + 2] = 0.0;
    const double X[3] = {uni(-150, 150), uni(-100, 100), uni(-50, 50)};
    worst = std::fmax(worst, jac_error<MODEL>(prm, X));
  }
  std::printf("%s jacobian: largest relative error %.3e\n", name, worst);
  worst_all = std::fmax(worst_all, worst);
  if (!(worst < 1e-6)) return false;
  std::printf("%s jacobian ok\n", name);
  return true;
}

static double rot_dist(const double* ra, const double* rb) {
  double A[9], B[9], d = 0.0;
  ba_rodrigues(ra, A);
  ba_rodrigues(rb, B);
  for (int e = 0; e < 9; ++e) d = std::fmax(d, std::fabs(A[e] - B[e]));
  return d;
}

// rvec -> R -> rvec, including the half-turn branch
static bool check_rvec() {
  double worst = 0.0;
  for (int i = 0; i < 200; ++i) {
    double rv[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)}, R[9], back[3];
    const double n = std::sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
    const double th = i < 100 ? uni(0.0, 3.1) : i < 150 ? 3.141592653589793 - uni(0.0, 1e-7) : uni(0.0, 1e-7);
    for (int k = 0; k < 3; ++k) rv[k] *= th / n;
    ba_rodrigues(rv, R);
    cal_rvec_from_R(R, back);
    worst = std::fmax(worst, rot_dist(rv, back));
  }
  std::printf("rvec round trip: largest |dR| %.3e\n", worst);
  if (!(worst < 1e-9)) return false;
  std::printf("rvec ok\n");
  return true;
}

// Zhang start on noise-free pinhole views of a board that does not lie in z = 0, and the pose of each view
static bool check_planar_start() {
  const double fx = 1800, fy = 1750, cx = 1023.5, cy = 767.5;
  const double k[CAL_NI] = {fx, fy, cx, cy, 0, 0, 0, 0, 0, 0};
  // the board's own frame: a rotation and an offset, so that the plane is generic
  const double brv[3] = {0.4, -0.3, 0.2}, boff[3] = {30, -20, 500};
  double Rb[9];
  ba_rodrigues(brv, Rb);
  std::vector<double> obj;
  for (int y = 0; y < 6; ++y)
    for (int x = 0; x < 9; ++x) {
      const double q[3] = {30.0 * x, 30.0 * y, 0.0};
      for (int i = 0; i < 3; ++i) obj.push_back(Rb[i * 3] * q[0] + Rb[i * 3 + 1] * q[1] + Rb[i * 3 + 2] * q[2] + boff[i]);
    }
  const int n = 54, V = 6;
  double N[3] = {0, 0, 0}, b[2] = {0, 0};
  std::vector<double> Hs(9 * V), cs(3 * V), Es(9 * V), poses(6 * V), uvs(2 * n * V);
  for (int v = 0; v < V; ++v) {
    // camera pose relative to the board frame, then composed with the board's frame
    double rl[3] = {uni(-0.5, 0.5), uni(-0.5, 0.5), uni(-0.5, 0.5)}, tl[3] = {uni(-150, -90), uni(-100, -50), uni(500, 900)};
    double Rl[9], R[9], t[3];
    ba_rodrigues(rl, Rl);
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) R[i * 3 + j] = Rl[i * 3] * Rb[j * 3] + Rl[i * 3 + 1] * Rb[j * 3 + 1] + Rl[i * 3 + 2] * Rb[j * 3 + 2];
      t[i] = tl[i] - (R[i * 3] * boff[0] + R[i * 3 + 1] * boff[1] + R[i * 3 + 2] * boff[2]);
    }
    cal_rvec_from_R(R, &poses[6 * v]);
    for (int i = 0; i < 3; ++i) poses[6 * v + 3 + i] = t[i];
    for (int i = 0; i < n; ++i) cal_project<CAL_PINHOLE>(k, R, t, &obj[3 * i], uvs[2 * (n * v + i)], uvs[2 * (n * v + i) + 1]);
    double ev[3];
    cal_object_frame(obj.data(), n, &cs[3 * v], &Es[9 * v], ev);
    if (!cal_is_planar(ev)) return false;
    cal_homography(obj.data(), &uvs[2 * n * v], n, &cs[3 * v], &Es[9 * v], &Hs[9 * v]);
    cal_zhang_accumulate(&Hs[9 * v], cx, cy, N, b);
  }
  double gfx = 0, gfy = 0;
  if (!cal_zhang_solve(N, b, gfx, gfy)) return false;
  double worst = std::fmax(std::fabs(gfx - fx) / fx, std::fabs(gfy - fy) / fy);
  for (int v = 0; v < V; ++v) {
    double pose[6];
    cal_pose_from_homography(&Hs[9 * v], gfx, gfy, cx, cy, &cs[3 * v], &Es[9 * v], pose);
    worst = std::fmax(worst, rot_dist(pose, &poses[6 * v]));
    for (int i = 0; i < 3; ++i) worst = std::fmax(worst, std::fabs(pose[3 + i] - poses[6 * v + 3 + i]) / 900.0);
  }
  std::printf("planar start (noise-free): largest relative error %.3e\n", worst);
  // every view fronto-parallel: the focal-length system must be reported singular
  double N2[3] = {0, 0, 0}, b2[2] = {0, 0};
  for (int v = 0; v < 4; ++v) {
    const double a = 0.3 * v, s = 2.0 + 0.1 * v;
    const double H[9] = {s * std::cos(a), -s * std::sin(a), cx + 3 * v, s * std::sin(a), s * std::cos(a), cy - 2 * v, 0, 0, 1};
    cal_zhang_accumulate(H, cx, cy, N2, b2);
  }
  if (cal_zhang_solve(N2, b2, gfx, gfy)) {
    std::printf("fronto-parallel views were not reported singular\n");
    return false;
  }
  if (!(worst < 1e-8)) return false;
  std::printf("planar start ok\n");
  return true;
}

// 3 x 4 DLT pose on noise-free normalised points of a non-planar target
static bool check_dlt_start() {
  double worst = 0.0;
  for (int trial = 0; trial < 5; ++trial) {
    const int n = trial == 0 ? 6 : 10;
    std::vector<double> obj(3 * n), xn(2 * n);
    for (int i = 0; i < 3 * n; ++i) obj[i] = uni(-400, 400);
    const double rv[3] = {uni(-1.5, 1.5), uni(-1.5, 1.5), uni(-1.5, 1.5)}, t[3] = {uni(-100, 100), uni(-100, 100), uni(1500, 2500)};
    double R[9];
    ba_rodrigues(rv, R);
    for (int i = 0; i < n; ++i) {
      double x0, x1, x2;
      cal_camera_point(R, t, &obj[3 * i], x0, x1, x2);
      xn[2 * i] = x0 / x2, xn[2 * i + 1] = x1 / x2;
    }
    double c[3], E[9], ev[3], pose[6];
    cal_object_frame(obj.data(), n, c, E, ev);
    if (cal_is_planar(ev)) return false;
    cal_pose_dlt(obj.data(), xn.data(), n, c, pose);
    worst = std::fmax(worst, rot_dist(pose, rv));
    for (int i = 0; i < 3; ++i) worst = std::fmax(worst, std::fabs(pose[3 + i] - t[i]) / 2500.0);
  }
  std::printf("DLT start (noise-free): largest relative error %.3e\n", worst);
  if (!(worst < 1e-8)) return false;
  std::printf("DLT start ok\n");
  return true;
}

int main() {
  double worst = 0.0;
  bool ok = check_model<CAL_PINHOLE>("pinhole", worst);
  ok = check_model<CAL_OMNIDIR>("omnidir", worst) && ok;
  std::printf("largest relative jacobian error %.3e\n", worst);
  ok = check_rvec() && ok;
  ok = check_planar_start() && ok;
  ok = check_dlt_start() && ok;
  return ok ? 0 : 1;
}
