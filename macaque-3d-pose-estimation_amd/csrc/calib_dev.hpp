// Per-point residual and Jacobian rows of the view calibration (calib.hip), and the closed-form starts of its
// Levenberg-Marquardt: plane homography, Zhang's focal length, pose from a homography or a 3 x 4 DLT.  Every
// function compiles for the host too (tests/calib_jac_check.cpp checks them against differences and identities).
//
// It replaces what the reference takes from OpenCV in calibrate_intrinsic (multicam_toolbox.py:74-116,
// cv2.calibrateCamera and cv2.omnidir.calibrate) and get_extrinsic_from_cagekeypoints (:213-242, cv2.solvePnP).
// OpenCV is not part of this project: where a rule below says "as cv2", it is cv2's rule as recalled, not pinned.
//
// A problem has 10 intrinsic slots and 6 pose slots per view; a Jacobian row has CAL_NC = 16 columns, intrinsics
// first.  Model ids are camera.hpp's:
//   CAL_OMNIDIR (0)  fx, fy, s, cx, cy, xi, k1, k2, p1, p2          camera.hpp omni_project
//   CAL_PINHOLE (1)  fx, fy, cx, cy, k1, k2, p1, p2, k3, (unused)   camera.hpp pinhole_project
// Derivatives are bundle_dev.hpp's staged dual numbers, no stage with more than six slots:
//   rvec (3)                    -> R                  once per view (ba_rotation_jac)
//   Xc (3) [, xi]               -> (x, y)             Xc[:2] / Xc[2], or the unit sphere shifted by xi (4 slots)
//   x, y, k1, k2, p1, p2 (6)    -> (xd, yd)           radial + tangential; the pinhole's k3 column by hand
//   fx, fy, s, cx, cy           -> (u, v)             affine: written out
#pragma once
#include "bundle_dev.hpp"

namespace mq {

constexpr int CAL_NI = 10;           // intrinsic slots
constexpr int CAL_NC = CAL_NI + 6;   // Jacobian columns: intrinsics, rvec, tvec
constexpr int CAL_OMNIDIR = 0, CAL_PINHOLE = 1;

// pinhole_project's distortion with its operation order; k3 is carried as a plain number
template <class T>
BA_HD void cal_pinhole_distort(const T& x, const T& y, const T& k1, const T& k2, const T& p1, const T& p2, double k3,
                               T& xd, T& yd) {
  const T r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
  const T a1 = 2.0 * x * y, a2 = r2 + 2.0 * x * x, a3 = r2 + 2.0 * y * y;
  const T cdist = 1.0 + k1 * r2 + k2 * r4 + r6 * k3;
  xd = x * cdist + p1 * a1 + p2 * a2;
  yd = y * cdist + p1 * a3 + p2 * a1;
}

BA_HD void cal_camera_point(const double* R, const double* t, const double* X, double& x0, double& x1, double& x2) {
  x0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
  x1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
  x2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
}

// projection of one point; k: the 10 slots, R, t: the view's pose
template <int MODEL>
BA_HD void cal_project(const double* k, const double* R, const double* t, const double* X, double& u, double& v) {
  double x0, x1, x2;
  cal_camera_point(R, t, X, x0, x1, x2);
  if (MODEL == CAL_PINHOLE) {
    const double iz = x2 != 0 ? 1. / x2 : 1;
    double xd, yd;
    cal_pinhole_distort(x0 * iz, x1 * iz, k[4], k[5], k[6], k[7], k[8], xd, yd);
    u = xd * k[0] + k[2];
    v = yd * k[1] + k[3];
  } else {
    double xu, yu, xd, yd;
    ba_omni_unit(x0, x1, x2, k[5], xu, yu);
    ba_omni_distort(xu, yu, k[6], k[7], k[8], k[9], xd, yd);
    u = k[0] * xd + k[2] * yd + k[3];
    v = k[1] * yd + k[4];
  }
}

// Residual r (2) = projection - pixel and its Jacobian A (2 x CAL_NC, row-major).  dR: ba_rotation_jac's 3 x 9.
template <int MODEL>
BA_HD void cal_obs_jac(const double* k, const double* R, const double* dR, const double* t, const double* X,
                       const double* ob, double* r, double* A) {
  constexpr int P = CAL_NC;
  double x0, x1, x2;
  cal_camera_point(R, t, X, x0, x1, x2);
  double Jq[2][3];  // d (u, v) / d Xc
  if (MODEL == CAL_PINHOLE) {
    const double z = x2 != 0 ? x2 : 1;
    const Dual<3> iz = 1.0 / dual_var<3>(z, 2);
    const Dual<3> x3 = dual_var<3>(x0, 0) * iz, y3 = dual_var<3>(x1, 1) * iz;
    Dual<6> xd6, yd6;
    cal_pinhole_distort(dual_var<6>(x3.v, 0), dual_var<6>(y3.v, 1), dual_var<6>(k[4], 2), dual_var<6>(k[5], 3),
                        dual_var<6>(k[6], 4), dual_var<6>(k[7], 5), k[8], xd6, yd6);
    const double fx = k[0], fy = k[1];
    r[0] = xd6.v * fx + k[2] - ob[0];
    r[1] = yd6.v * fy + k[3] - ob[1];
    for (int j = 0; j < 3; ++j) {
      Jq[0][j] = fx * (xd6.d[0] * x3.d[j] + xd6.d[1] * y3.d[j]);
      Jq[1][j] = fy * (yd6.d[0] * x3.d[j] + yd6.d[1] * y3.d[j]);
    }
    const double r2 = x3.v * x3.v + y3.v * y3.v, r6 = r2 * r2 * r2;
    A[0 * P + 0] = xd6.v, A[1 * P + 0] = 0.0;  // fx
    A[0 * P + 1] = 0.0, A[1 * P + 1] = yd6.v;  // fy
    A[0 * P + 2] = 1.0, A[1 * P + 2] = 0.0;    // cx
    A[0 * P + 3] = 0.0, A[1 * P + 3] = 1.0;    // cy
    for (int j = 0; j < 4; ++j) {              // k1, k2, p1, p2
      A[0 * P + 4 + j] = fx * xd6.d[2 + j];
      A[1 * P + 4 + j] = fy * yd6.d[2 + j];
    }
    A[0 * P + 8] = fx * (x3.v * r6), A[1 * P + 8] = fy * (y3.v * r6);  // k3
    A[0 * P + 9] = 0.0, A[1 * P + 9] = 0.0;
  } else {
    Dual<4> xu4, yu4;
    ba_omni_unit(dual_var<4>(x0, 0), dual_var<4>(x1, 1), dual_var<4>(x2, 2), dual_var<4>(k[5], 3), xu4, yu4);
    Dual<6> xd6, yd6;
    ba_omni_distort(dual_var<6>(xu4.v, 0), dual_var<6>(yu4.v, 1), dual_var<6>(k[6], 2), dual_var<6>(k[7], 3),
                    dual_var<6>(k[8], 4), dual_var<6>(k[9], 5), xd6, yd6);
    const double fx = k[0], fy = k[1], sk = k[2];
    const double xd = xd6.v, yd = yd6.v;
    r[0] = fx * xd + sk * yd + k[3] - ob[0];
    r[1] = fy * yd + k[4] - ob[1];
    double G[2][2];  // d (u, v) / d (xu, yu)
    for (int j = 0; j < 2; ++j) {
      G[0][j] = fx * xd6.d[j] + sk * yd6.d[j];
      G[1][j] = fy * yd6.d[j];
    }
    for (int j = 0; j < 3; ++j) {
      Jq[0][j] = G[0][0] * xu4.d[j] + G[0][1] * yu4.d[j];
      Jq[1][j] = G[1][0] * xu4.d[j] + G[1][1] * yu4.d[j];
    }
    A[0 * P + 0] = xd, A[1 * P + 0] = 0.0;   // fx
    A[0 * P + 1] = 0.0, A[1 * P + 1] = yd;   // fy
    A[0 * P + 2] = yd, A[1 * P + 2] = 0.0;   // s
    A[0 * P + 3] = 1.0, A[1 * P + 3] = 0.0;  // cx
    A[0 * P + 4] = 0.0, A[1 * P + 4] = 1.0;  // cy
    A[0 * P + 5] = G[0][0] * xu4.d[3] + G[0][1] * yu4.d[3];  // xi
    A[1 * P + 5] = G[1][0] * xu4.d[3] + G[1][1] * yu4.d[3];
    for (int j = 0; j < 4; ++j) {  // k1, k2, p1, p2
      A[0 * P + 6 + j] = fx * xd6.d[2 + j] + sk * yd6.d[2 + j];
      A[1 * P + 6 + j] = fy * yd6.d[2 + j];
    }
  }
  for (int c = 0; c < 3; ++c) {
    const double* D = dR + 9 * c;  // d Xc / d rvec_c = dR_c X
    const double d0 = D[0] * X[0] + D[1] * X[1] + D[2] * X[2];
    const double d1 = D[3] * X[0] + D[4] * X[1] + D[5] * X[2];
    const double d2 = D[6] * X[0] + D[7] * X[1] + D[8] * X[2];
    for (int row = 0; row < 2; ++row) {
      A[row * P + CAL_NI + c] = Jq[row][0] * d0 + Jq[row][1] * d1 + Jq[row][2] * d2;
      A[row * P + CAL_NI + 3 + c] = Jq[row][c];
    }
  }
}

// ----------------------------------------------------------------------------- closed-form starts
// Cyclic Jacobi on a symmetric N x N matrix (row-major, destroyed: its diagonal ends as the eigenvalues).
// V (row-major): column j is the eigenvector of A[j][j].  At most 30 sweeps.
template <int N>
BA_HD void cal_jacobi_eig(double* A, double* V) {
  double nrm = 0.0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      V[i * N + j] = i == j ? 1.0 : 0.0;
      nrm += A[i * N + j] * A[i * N + j];
    }
  const double tiny = 1e-18 * sqrt(nrm);
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p * N + q];
        if (!(fabs(apq) > tiny)) continue;
        rotated = true;
        const double theta = (A[q * N + q] - A[p * N + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < N; ++i) {  // columns p, q
          const double aip = A[i * N + p], aiq = A[i * N + q];
          A[i * N + p] = c * aip - s * aiq;
          A[i * N + q] = s * aip + c * aiq;
        }
        for (int i = 0; i < N; ++i) {  // rows p, q
          const double api = A[p * N + i], aqi = A[q * N + i];
          A[p * N + i] = c * api - s * aqi;
          A[q * N + i] = s * api + c * aqi;
        }
        for (int i = 0; i < N; ++i) {
          const double vip = V[i * N + p], viq = V[i * N + q];
          V[i * N + p] = c * vip - s * viq;
          V[i * N + q] = s * vip + c * viq;
        }
      }
    if (!rotated) break;
  }
}

template <int N>
BA_HD int cal_smallest(const double* A) {
  int m = 0;
  for (int j = 1; j < N; ++j)
    if (A[j * N + j] < A[m * N + m]) m = j;
  return m;
}

BA_HD double cal_det3(const double* M) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// The rotation nearest to M (3 x 3 row-major, det M > 0) in the Frobenius norm: R = M (M^T M)^-1/2.  Returns the
// mean singular value of M (NaN entries in R where M is singular).
BA_HD double cal_polar3(const double* M, double* R) {
  double S[9], V[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) S[i * 3 + j] = M[i] * M[j] + M[3 + i] * M[3 + j] + M[6 + i] * M[6 + j];
  cal_jacobi_eig<3>(S, V);
  double sg[3], Q[9];
  for (int j = 0; j < 3; ++j) sg[j] = sqrt(S[j * 3 + j]);
  for (int i = 0; i < 3; ++i)  // Q = V diag(1 / sigma) V^T
    for (int j = 0; j < 3; ++j)
      Q[i * 3 + j] = V[i * 3] * V[j * 3] / sg[0] + V[i * 3 + 1] * V[j * 3 + 1] / sg[1] + V[i * 3 + 2] * V[j * 3 + 2] / sg[2];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = M[i * 3] * Q[j] + M[i * 3 + 1] * Q[3 + j] + M[i * 3 + 2] * Q[6 + j];
  return (sg[0] + sg[1] + sg[2]) / 3.0;
}

// R -> rvec (the inverse of ba_rodrigues), with the branch near a half turn taken from R + R^T.
BA_HD void cal_rvec_from_R(const double* R, double* rv) {
  const double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
  const double s = 0.5 * sqrt(rx * rx + ry * ry + rz * rz);
  double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  c = c > 1.0 ? 1.0 : c < -1.0 ? -1.0 : c;
  const double theta = atan2(s, c);
  if (s < 1e-5) {
    if (c > 0.0) {  // R = I + [r]x to first order
      rv[0] = 0.5 * rx, rv[1] = 0.5 * ry, rv[2] = 0.5 * rz;
      return;
    }
    // (R + I) / 2 = a a^T at a half turn: the axis from the row of its largest diagonal entry
    const int i = R[0] >= R[4] && R[0] >= R[8] ? 0 : R[4] >= R[8] ? 1 : 2;
    const double ai = sqrt(fmax((R[4 * i] + 1.0) * 0.5, 0.0));
    double a[3];
    for (int j = 0; j < 3; ++j) a[j] = j == i ? ai : 0.25 * (R[3 * i + j] + R[3 * j + i]) / ai;
    const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const double sgn = a[0] * rx + a[1] * ry + a[2] * rz < 0.0 ? -1.0 : 1.0;
    for (int j = 0; j < 3; ++j) rv[j] = sgn * theta * a[j] / n;
    return;
  }
  const double f = theta / (2.0 * s);
  rv[0] = f * rx, rv[1] = f * ry, rv[2] = f * rz;
}

// Centroid c, eigenframe E (3 x 3 row-major, columns by falling eigenvalue, det +1) and eigenvalues ev (falling)
// of the scatter matrix of n object points.
BA_HD void cal_object_frame(const double* obj, int n, double* c, double* E, double* ev) {
  c[0] = c[1] = c[2] = 0.0;
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) c[k] += obj[3 * i + k];
  for (int k = 0; k < 3; ++k) c[k] /= n;
  double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, V[9];
  for (int i = 0; i < n; ++i) {
    const double d[3] = {obj[3 * i] - c[0], obj[3 * i + 1] - c[1], obj[3 * i + 2] - c[2]};
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) S[a * 3 + b] += d[a] * d[b];
  }
  cal_jacobi_eig<3>(S, V);
  int o[3] = {0, 1, 2};
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2 - a; ++b)
      if (S[o[b] * 4] < S[o[b + 1] * 4]) {
        const int tmp = o[b];
        o[b] = o[b + 1], o[b + 1] = tmp;
      }
  for (int j = 0; j < 3; ++j) {
    ev[j] = S[o[j] * 4];
    for (int i = 0; i < 3; ++i) E[i * 3 + j] = V[i * 3 + o[j]];
  }
  if (cal_det3(E) < 0.0)
    for (int i = 0; i < 3; ++i) E[i * 3 + 2] = -E[i * 3 + 2];
}

// The planarity rule (cv2.solvePnP's, as recalled): the smallest eigenvalue below 1e-3 of the middle one.
BA_HD bool cal_is_planar(const double* ev) { return ev[2] < 1e-3 * ev[1]; }

// Hartley-normalised DLT homography H (3 x 3 row-major) from the plane coordinates q = E^T (X - c) [:2] of n object
// points to their image points uv: the eigenvector of the smallest eigenvalue of the 9 x 9 A^T A.
BA_HD void cal_homography(const double* obj, const double* uv, int n, const double* c, const double* E, double* H) {
  double mq[2] = {0, 0}, mu[2] = {0, 0}, dq = 0.0, du = 0.0;
  for (int i = 0; i < n; ++i) {
    mu[0] += uv[2 * i], mu[1] += uv[2 * i + 1];
  }
  mu[0] /= n, mu[1] /= n;  // the plane coordinates are centred by construction
  for (int i = 0; i < n; ++i) {
    const double d[3] = {obj[3 * i] - c[0], obj[3 * i + 1] - c[1], obj[3 * i + 2] - c[2]};
    const double qx = E[0] * d[0] + E[3] * d[1] + E[6] * d[2], qy = E[1] * d[0] + E[4] * d[1] + E[7] * d[2];
    dq += sqrt(qx * qx + qy * qy);
    const double ux = uv[2 * i] - mu[0], uy = uv[2 * i + 1] - mu[1];
    du += sqrt(ux * ux + uy * uy);
  }
  const double sq = 1.4142135623730951 * n / dq, su = 1.4142135623730951 * n / du;
  double A[81], V[81];
  for (int e = 0; e < 81; ++e) A[e] = 0.0;
  for (int i = 0; i < n; ++i) {
    const double d[3] = {obj[3 * i] - c[0], obj[3 * i + 1] - c[1], obj[3 * i + 2] - c[2]};
    const double X = sq * (E[0] * d[0] + E[3] * d[1] + E[6] * d[2] - mq[0]);
    const double Y = sq * (E[1] * d[0] + E[4] * d[1] + E[7] * d[2] - mq[1]);
    const double u = su * (uv[2 * i] - mu[0]), v = su * (uv[2 * i + 1] - mu[1]);
    const double a1[9] = {-X, -Y, -1.0, 0, 0, 0, u * X, u * Y, u};
    const double a2[9] = {0, 0, 0, -X, -Y, -1.0, v * X, v * Y, v};
    for (int a = 0; a < 9; ++a)
      for (int b = 0; b < 9; ++b) A[a * 9 + b] += a1[a] * a1[b] + a2[a] * a2[b];
  }
  cal_jacobi_eig<9>(A, V);
  const int m = cal_smallest<9>(A);
  double h[9];
  for (int e = 0; e < 9; ++e) h[e] = V[e * 9 + m];
  // H = Tu^-1 Hn Tq, Tq = [[sq, 0, 0], [0, sq, 0], [0, 0, 1]] (centred), Tu^-1 = [[1/su, 0, mu0], [0, 1/su, mu1], [0, 0, 1]]
  for (int j = 0; j < 3; ++j) {
    const double f = j < 2 ? sq : 1.0;
    H[j] = (h[j] / su + mu[0] * h[6 + j]) * f;
    H[3 + j] = (h[3 + j] / su + mu[1] * h[6 + j]) * f;
    H[6 + j] = h[6 + j] * f;
  }
}

// Zhang's two constraints of one view on (1 / fx^2, 1 / fy^2) with the centre fixed at (cx, cy), in the scaled
// form of cv2's cvInitIntrinsicParams2D (as recalled): added to the 2 x 2 normal equations N (n00, n01, n11), b.
BA_HD void cal_zhang_accumulate(const double* H, double cx, double cy, double* N, double* b) {
  double h[3], v[3], d1[3], d2[3];
  h[0] = H[0] - cx * H[6], h[1] = H[3] - cy * H[6], h[2] = H[6];
  v[0] = H[1] - cx * H[7], v[1] = H[4] - cy * H[7], v[2] = H[7];
  double nh = 0, nv = 0, n1 = 0, n2 = 0;
  for (int j = 0; j < 3; ++j) {
    d1[j] = (h[j] + v[j]) * 0.5;
    d2[j] = (h[j] - v[j]) * 0.5;
    nh += h[j] * h[j], nv += v[j] * v[j], n1 += d1[j] * d1[j], n2 += d2[j] * d2[j];
  }
  nh = 1.0 / sqrt(nh), nv = 1.0 / sqrt(nv), n1 = 1.0 / sqrt(n1), n2 = 1.0 / sqrt(n2);
  for (int j = 0; j < 3; ++j) h[j] *= nh, v[j] *= nv, d1[j] *= n1, d2[j] *= n2;
  const double a[2][2] = {{h[0] * v[0], h[1] * v[1]}, {d1[0] * d2[0], d1[1] * d2[1]}};
  const double rhs[2] = {-h[2] * v[2], -d1[2] * d2[2]};
  for (int e = 0; e < 2; ++e) {
    N[0] += a[e][0] * a[e][0], N[1] += a[e][0] * a[e][1], N[2] += a[e][1] * a[e][1];
    b[0] += a[e][0] * rhs[e], b[1] += a[e][1] * rhs[e];
  }
}

// fx, fy from the summed normal equations; false when the system is singular (reciprocal condition below 1e-9,
// every view fronto-parallel for instance) or the result is not a finite positive length.
BA_HD bool cal_zhang_solve(const double* N, const double* b, double& fx, double& fy) {
  const double det = N[0] * N[2] - N[1] * N[1];
  const double tr = N[0] + N[2];
  if (!(det > 1e-9 * tr * tr)) return false;
  const double X = (N[2] * b[0] - N[1] * b[1]) / det, Y = (N[0] * b[1] - N[1] * b[0]) / det;
  fx = sqrt(fabs(1.0 / X));
  fy = sqrt(fabs(1.0 / Y));
  return isfinite(fx) && isfinite(fy) && fx > 0.0 && fy > 0.0;
}

// Pose of the plane (c, E) from its homography and fx, fy, cx, cy: K^-1 H scaled by 1 / |column 0|, signed so that
// t_z > 0, [r1 r2 r1 x r2] projected onto a rotation.  pose: rvec, tvec of the object frame.
BA_HD void cal_pose_from_homography(const double* H, double fx, double fy, double cx, double cy, const double* c,
                                    const double* E, double* pose) {
  double M[9];
  for (int j = 0; j < 3; ++j) {
    M[j] = (H[j] - cx * H[6 + j]) / fx;
    M[3 + j] = (H[3 + j] - cy * H[6 + j]) / fy;
    M[6 + j] = H[6 + j];
  }
  double sc = 1.0 / sqrt(M[0] * M[0] + M[3] * M[3] + M[6] * M[6]);
  if (M[8] * sc < 0.0) sc = -sc;
  const double r1[3] = {M[0] * sc, M[3] * sc, M[6] * sc}, r2[3] = {M[1] * sc, M[4] * sc, M[7] * sc};
  const double tp[3] = {M[2] * sc, M[5] * sc, M[8] * sc};
  const double r3[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
  const double Q[9] = {r1[0], r2[0], r3[0], r1[1], r2[1], r3[1], r1[2], r2[2], r3[2]};
  double Rp[9], R[9];
  cal_polar3(Q, Rp);
  for (int i = 0; i < 3; ++i)  // R = R' E^T
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = Rp[i * 3] * E[j * 3] + Rp[i * 3 + 1] * E[j * 3 + 1] + Rp[i * 3 + 2] * E[j * 3 + 2];
  cal_rvec_from_R(R, pose);
  for (int i = 0; i < 3; ++i) pose[3 + i] = tp[i] - (R[i * 3] * c[0] + R[i * 3 + 1] * c[1] + R[i * 3 + 2] * c[2]);
}

// Pose of a non-planar target from n >= 6 normalised image points xn: Hartley-normalised 3 x 4 DLT (the eigenvector
// of the smallest eigenvalue of the 12 x 12 A^T A), its left 3 x 3 projected onto a rotation.
BA_HD void cal_pose_dlt(const double* obj, const double* xn, int n, const double* c, double* pose) {
  double mu[2] = {0, 0}, dX = 0.0, du = 0.0;
  for (int i = 0; i < n; ++i) mu[0] += xn[2 * i], mu[1] += xn[2 * i + 1];
  mu[0] /= n, mu[1] /= n;
  for (int i = 0; i < n; ++i) {
    const double d[3] = {obj[3 * i] - c[0], obj[3 * i + 1] - c[1], obj[3 * i + 2] - c[2]};
    dX += sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const double ux = xn[2 * i] - mu[0], uy = xn[2 * i + 1] - mu[1];
    du += sqrt(ux * ux + uy * uy);
  }
  const double sX = 1.7320508075688772 * n / dX, su = 1.4142135623730951 * n / du;
  double A[144], V[144];
  for (int e = 0; e < 144; ++e) A[e] = 0.0;
  for (int i = 0; i < n; ++i) {
    const double X[4] = {sX * (obj[3 * i] - c[0]), sX * (obj[3 * i + 1] - c[1]), sX * (obj[3 * i + 2] - c[2]), 1.0};
    const double u = su * (xn[2 * i] - mu[0]), v = su * (xn[2 * i + 1] - mu[1]);
    double a1[12], a2[12];
    for (int k = 0; k < 4; ++k) {
      a1[k] = -X[k], a1[4 + k] = 0.0, a1[8 + k] = u * X[k];
      a2[k] = 0.0, a2[4 + k] = -X[k], a2[8 + k] = v * X[k];
    }
    for (int a = 0; a < 12; ++a)
      for (int b = 0; b < 12; ++b) A[a * 12 + b] += a1[a] * a1[b] + a2[a] * a2[b];
  }
  cal_jacobi_eig<12>(A, V);
  const int m = cal_smallest<12>(A);
  double p[12], P[12];
  for (int e = 0; e < 12; ++e) p[e] = V[e * 12 + m];
  // P = Tu^-1 Pn TX, TX = [sX I | -sX c]
  for (int j = 0; j < 4; ++j) {
    P[j] = p[j] / su + mu[0] * p[8 + j];
    P[4 + j] = p[4 + j] / su + mu[1] * p[8 + j];
    P[8 + j] = p[8 + j];
  }
  double M[9], t4[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) M[i * 3 + j] = P[i * 4 + j] * sX;
    t4[i] = P[i * 4 + 3] - sX * (P[i * 4] * c[0] + P[i * 4 + 1] * c[1] + P[i * 4 + 2] * c[2]);
  }
  if (cal_det3(M) < 0.0) {
    for (int e = 0; e < 9; ++e) M[e] = -M[e];
    for (int i = 0; i < 3; ++i) t4[i] = -t4[i];
  }
  double R[9];
  const double s = cal_polar3(M, R);
  cal_rvec_from_R(R, pose);
  for (int i = 0; i < 3; ++i) pose[3 + i] = t4[i] / s;
}

}  // namespace mq
