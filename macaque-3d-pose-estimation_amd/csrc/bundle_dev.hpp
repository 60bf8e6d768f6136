// Per-observation residual and Jacobian blocks of the rig bundle adjustment (bundle.hip), as functions that
// compile for the host too (a CPU program can check the derivatives against differences).
//
// Derivatives are forward-mode dual numbers through projections templated on the scalar type, in stages so
// that no stage carries more than six derivative slots:
//   rvec (3)                 -> R                    once per camera and workgroup, not per observation
//   Xc = R X + t, xi (4)     -> (xu, yu)             unit sphere + xi shift (mode 1) or Xc[:2] / Xc[2] (mode 0)
//   xu, yu, k1, k2, p1, p2   -> (xd, yd)             radial + tangential distortion
//   K                        -> (u, v)               affine: written out
// and chained by hand.  The stage functions restate camera.hpp's omni_project with its operation order.
//
// Mode 2 (aniposelib's CameraGroup.bundle_adjust, cameras.py:894-980) has 9 slots per camera, rvec, tvec, f, k1,
// k2, and a model per camera (camera.hpp's ids) with the data the solve does not move next to them:
//   Xc (3)                   -> (x, y)               Xc[:2] / Xc[2], or the omnidir unit-sphere point (xi fixed)
//   x, y, f, k1, k2 (5)      -> (u, v)               pinhole: f x (1 + k1 r2 + k2 r2^2) + cx;  fisheye: f x
//                                                    theta_d / r + cx, theta_d = theta (1 + k1 theta^2 + k2
//                                                    theta^4);  omnidir: fixed K, D on (x, y) alone (2 slots)
#pragma once
#include <math.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif
#define BA_HD __host__ __device__ inline

namespace mq {

constexpr int BA_MAXC = 16;  // cameras (OPT_MAXC)
constexpr int BA_MAXP = 16;  // parameters per camera in mode 1: rvec, tvec, K00, K01, K02, K11, K12, xi, D[4]
constexpr int BA_GP = 9;     // parameter slots per camera in mode 2: rvec, tvec, f, k1, k2
constexpr int BA_GFIX = 11;  // mode 2, what the solve does not move: model, then cx, cy (pinhole, fisheye) or
                             // K00, K01, K02, K11, K12, xi, D[4] (omnidir)
constexpr int BA_GROW = BA_GP + BA_GFIX;  // a mode-2 camera row: the slots, then the fixed data
constexpr int BA_CAM_OMNIDIR = 0, BA_CAM_PINHOLE = 1, BA_CAM_FISHEYE = 2;  // camera.hpp's CamModel

constexpr int ba_nparams(int mode) { return mode == 2 ? BA_GP : mode ? 16 : 6; }

template <int N>
struct Dual {
  double v;
  double d[N];
};

template <int N>
BA_HD Dual<N> dual_const(double v) {
  Dual<N> r;
  r.v = v;
  for (int i = 0; i < N; ++i) r.d[i] = 0.0;
  return r;
}
template <int N>
BA_HD Dual<N> dual_var(double v, int slot) {
  Dual<N> r = dual_const<N>(v);
  r.d[slot] = 1.0;
  return r;
}
template <int N>
BA_HD Dual<N> operator+(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v + b.v;
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] + b.d[i];
  return r;
}
template <int N>
BA_HD Dual<N> operator-(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v - b.v;
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] - b.d[i];
  return r;
}
template <int N>
BA_HD Dual<N> operator*(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v * b.v;
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
  return r;
}
template <int N>
BA_HD Dual<N> operator/(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  const double ib = 1.0 / b.v;
  r.v = a.v / b.v;
  for (int i = 0; i < N; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * ib;
  return r;
}
template <int N>
BA_HD Dual<N> operator+(const Dual<N>& a, double b) {
  Dual<N> r = a;
  r.v = a.v + b;
  return r;
}
template <int N>
BA_HD Dual<N> operator+(double a, const Dual<N>& b) {
  return b + a;
}
template <int N>
BA_HD Dual<N> operator-(double a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a - b.v;
  for (int i = 0; i < N; ++i) r.d[i] = -b.d[i];
  return r;
}
template <int N>
BA_HD Dual<N> operator/(double a, const Dual<N>& b) {
  Dual<N> r;
  const double ib = 1.0 / b.v;
  r.v = a / b.v;
  for (int i = 0; i < N; ++i) r.d[i] = -(r.v * b.d[i]) * ib;
  return r;
}
template <int N>
BA_HD Dual<N> operator*(const Dual<N>& a, double b) {
  Dual<N> r;
  r.v = a.v * b;
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * b;
  return r;
}
template <int N>
BA_HD Dual<N> operator*(double a, const Dual<N>& b) {
  return b * a;
}
template <int N>
BA_HD Dual<N> ba_sqrt(const Dual<N>& a) {
  Dual<N> r;
  r.v = sqrt(a.v);
  const double h = 0.5 / r.v;
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * h;
  return r;
}
template <int N>
BA_HD Dual<N> ba_sin(const Dual<N>& a) {
  Dual<N> r;
  r.v = sin(a.v);
  const double c = cos(a.v);
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * c;
  return r;
}
template <int N>
BA_HD Dual<N> ba_cos(const Dual<N>& a) {
  Dual<N> r;
  r.v = cos(a.v);
  const double s = -sin(a.v);
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * s;
  return r;
}
template <int N>
BA_HD Dual<N> ba_atan(const Dual<N>& a) {
  Dual<N> r;
  r.v = atan(a.v);
  const double h = 1.0 / (1.0 + a.v * a.v);
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * h;
  return r;
}
BA_HD double ba_atan(double a) { return atan(a); }
BA_HD double ba_sqrt(double a) { return sqrt(a); }
BA_HD double ba_sin(double a) { return sin(a); }
BA_HD double ba_cos(double a) { return cos(a); }
BA_HD double ba_value(double a) { return a; }
template <int N>
BA_HD double ba_value(const Dual<N>& a) {
  return a.v;
}

// Rodrigues: R = c I + (1 - c) u u^T + s [u]x, u = r / |r| (cv2.Rodrigues; the reference's `rotate` :551-564 is
// the same map applied to a point).  Below |r|^2 = 1e-24 the first-order R = I + [r]x keeps the derivative
// finite where the reference divides 0 by 0 and zeroes it.
template <class T>
BA_HD void ba_rodrigues(const T r[3], T R[9]) {
  const T t2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  if (ba_value(t2) < 1e-24) {
    const T one = r[0] * 0.0 + 1.0;
    R[0] = one, R[1] = 0.0 - r[2], R[2] = r[1];
    R[3] = r[2], R[4] = one, R[5] = 0.0 - r[0];
    R[6] = 0.0 - r[1], R[7] = r[0], R[8] = one;
    return;
  }
  const T th = ba_sqrt(t2);
  const T c = ba_cos(th), s = ba_sin(th);
  const T c1 = 1.0 - c;
  const T ux = r[0] / th, uy = r[1] / th, uz = r[2] / th;
  R[0] = c + c1 * ux * ux, R[1] = c1 * ux * uy - s * uz, R[2] = c1 * ux * uz + s * uy;
  R[3] = c1 * uy * ux + s * uz, R[4] = c + c1 * uy * uy, R[5] = c1 * uy * uz - s * ux;
  R[6] = c1 * uz * ux - s * uy, R[7] = c1 * uz * uy + s * ux, R[8] = c + c1 * uz * uz;
}

// R (9) and dR / d rvec_k (3 x 9) of one camera
BA_HD void ba_rotation_jac(const double* rvec, double* R, double* dR) {
  Dual<3> r[3], Rd[9];
  for (int k = 0; k < 3; ++k) r[k] = dual_var<3>(rvec[k], k);
  ba_rodrigues(r, Rd);
  for (int e = 0; e < 9; ++e) {
    R[e] = Rd[e].v;
    for (int k = 0; k < 3; ++k) dR[9 * k + e] = Rd[e].d[k];
  }
}

// omni_project up to the distortion: point on the unit sphere, shifted by xi
template <class T>
BA_HD void ba_omni_unit(const T& x0, const T& x1, const T& x2, const T& xi, T& xu, T& yu) {
  const T nrm = ba_sqrt(x0 * x0 + x1 * x1 + x2 * x2);
  const T xs = x0 / nrm, ys = x1 / nrm, zs = x2 / nrm;
  xu = xs / (zs + xi);
  yu = ys / (zs + xi);
}

template <class T>
BA_HD void ba_omni_distort(const T& xu, const T& yu, const T& k1, const T& k2, const T& p1, const T& p2, T& xd,
                           T& yd) {
  const T r2 = xu * xu + yu * yu;
  const T r4 = r2 * r2;
  xd = xu * (1.0 + k1 * r2 + k2 * r4) + 2.0 * p1 * xu * yu + p2 * (r2 + 2.0 * xu * xu);
  yd = yu * (1.0 + k1 * r2 + k2 * r4) + p1 * (r2 + 2.0 * yu * yu) + 2.0 * p2 * xu * yu;
}

// Mode 2, pinhole on the reduced model set_params leaves (cameras.py:290-299: fx = fy = f, distortions k1, k2
// only): pinhole_project's operation order with the terms that are zero left out.
template <class T>
BA_HD void ba_group_pinhole(const T& x, const T& y, const T& f, const T& k1, const T& k2, double cx, double cy, T& u,
                            T& v) {
  const T r2 = x * x + y * y;
  const T r4 = r2 * r2;
  const T cdist = 1.0 + k1 * r2 + k2 * r4;
  u = (x * cdist) * f + cx;
  v = (y * cdist) * f + cy;
}

// Mode 2, fisheye on the reduced model (cameras.py:392-403): fisheye_project's operation order and its rule
// cdist = 1 at r <= 1e-8, where theta_d / r -> 1 and the derivative with respect to k1, k2 is O(r^2).
template <class T>
BA_HD void ba_group_fisheye(const T& x, const T& y, const T& f, const T& k1, const T& k2, double cx, double cy, T& u,
                            T& v) {
  const T r2 = x * x + y * y;
  T cdist = r2 * 0.0 + 1.0;
  if (sqrt(ba_value(r2)) > 1e-8) {
    const T r = ba_sqrt(r2);
    const T th = ba_atan(r);
    const T th2 = th * th, th3 = th2 * th, th4 = th2 * th2, th5 = th4 * th;
    const T theta_d = th + k1 * th3 + k2 * th5;
    cdist = theta_d * (1.0 / r);
  }
  u = (x * cdist) * f + cx;
  v = (y * cdist) * f + cy;
}

// Mode 2, one camera row's projection of the camera-frame point; g: the row's fixed data (after the model)
template <class T>
BA_HD void ba_group_unit(int model, const double* g, const T& x0, const T& x1, const T& x2, T& x, T& y) {
  if (model == BA_CAM_OMNIDIR) {
    ba_omni_unit(x0, x1, x2, x0 * 0.0 + g[5], x, y);
  } else {
    x = x0 / x2;
    y = x1 / x2;
  }
}

// Residual of one observation.  cp: the camera's P parameters (mode 2: its BA_GROW row); R: its rotation matrix.
template <int MODE>
BA_HD void ba_obs_res(const double* cp, const double* R, const double* X, const double* ob, double* r) {
  const double x0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + cp[3];
  const double x1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + cp[4];
  const double x2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + cp[5];
  if (MODE == 2) {
    const int model = (int)cp[BA_GP];
    const double* g = cp + BA_GP + 1;
    double x, y, u, v;
    ba_group_unit(model, g, x0, x1, x2, x, y);
    if (model == BA_CAM_OMNIDIR) {
      double xd, yd;
      ba_omni_distort(x, y, g[6], g[7], g[8], g[9], xd, yd);
      u = g[0] * xd + g[1] * yd + g[2];
      v = g[3] * yd + g[4];
    } else if (model == BA_CAM_PINHOLE) {
      ba_group_pinhole(x, y, cp[6], cp[7], cp[8], g[0], g[1], u, v);
    } else {
      ba_group_fisheye(x, y, cp[6], cp[7], cp[8], g[0], g[1], u, v);
    }
    r[0] = u - ob[0];
    r[1] = v - ob[1];
  } else if (MODE == 0) {
    r[0] = x0 / x2 - ob[0];
    r[1] = x1 / x2 - ob[1];
  } else {
    double xu, yu, xd, yd;
    ba_omni_unit(x0, x1, x2, cp[11], xu, yu);
    ba_omni_distort(xu, yu, cp[12], cp[13], cp[14], cp[15], xd, yd);
    r[0] = cp[6] * xd + cp[7] * yd + cp[8] - ob[0];
    r[1] = cp[9] * yd + cp[10] - ob[1];
  }
}

// Residual r (2) and the Jacobian blocks of one observation: A (2 x P, row-major) with respect to the camera's
// parameters, B (2 x 3) with respect to the point.  dR: ba_rotation_jac's 3 x 9.
template <int MODE>
BA_HD void ba_obs_jac(const double* cp, const double* R, const double* dR, const double* X, const double* ob,
                      double* r, double* A, double* B) {
  constexpr int P = ba_nparams(MODE);
  const double x0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + cp[3];
  const double x1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + cp[4];
  const double x2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + cp[5];
  double Jq[2][3];  // d (u, v) / d Xc
  if (MODE == 2) {
    const int model = (int)cp[BA_GP];
    const double* g = cp + BA_GP + 1;
    Dual<3> x3, y3;
    ba_group_unit(model, g, dual_var<3>(x0, 0), dual_var<3>(x1, 1), dual_var<3>(x2, 2), x3, y3);
    double G[2][2];  // d (u, v) / d (x, y)
    if (model == BA_CAM_OMNIDIR) {  // K, xi, D are not among the slots: columns 6.. are zero and stay frozen
      Dual<2> xd2, yd2;
      ba_omni_distort(dual_var<2>(x3.v, 0), dual_var<2>(y3.v, 1), dual_const<2>(g[6]), dual_const<2>(g[7]),
                      dual_const<2>(g[8]), dual_const<2>(g[9]), xd2, yd2);
      r[0] = g[0] * xd2.v + g[1] * yd2.v + g[2] - ob[0];
      r[1] = g[3] * yd2.v + g[4] - ob[1];
      for (int j = 0; j < 2; ++j) {
        G[0][j] = g[0] * xd2.d[j] + g[1] * yd2.d[j];
        G[1][j] = g[3] * yd2.d[j];
      }
      for (int j = 6; j < P; ++j) A[0 * P + j] = 0.0, A[1 * P + j] = 0.0;
    } else {
      Dual<5> u5, v5;
      if (model == BA_CAM_PINHOLE)
        ba_group_pinhole(dual_var<5>(x3.v, 0), dual_var<5>(y3.v, 1), dual_var<5>(cp[6], 2), dual_var<5>(cp[7], 3),
                         dual_var<5>(cp[8], 4), g[0], g[1], u5, v5);
      else
        ba_group_fisheye(dual_var<5>(x3.v, 0), dual_var<5>(y3.v, 1), dual_var<5>(cp[6], 2), dual_var<5>(cp[7], 3),
                         dual_var<5>(cp[8], 4), g[0], g[1], u5, v5);
      r[0] = u5.v - ob[0];
      r[1] = v5.v - ob[1];
      for (int j = 0; j < 2; ++j) G[0][j] = u5.d[j], G[1][j] = v5.d[j];
      for (int j = 0; j < 3; ++j) A[0 * P + 6 + j] = u5.d[2 + j], A[1 * P + 6 + j] = v5.d[2 + j];  // f, k1, k2
    }
    for (int j = 0; j < 3; ++j) {
      Jq[0][j] = G[0][0] * x3.d[j] + G[0][1] * y3.d[j];
      Jq[1][j] = G[1][0] * x3.d[j] + G[1][1] * y3.d[j];
    }
  } else if (MODE == 0) {
    const double iz = 1.0 / x2;
    const double x = x0 / x2, y = x1 / x2;
    r[0] = x - ob[0];
    r[1] = y - ob[1];
    Jq[0][0] = iz, Jq[0][1] = 0.0, Jq[0][2] = -x * iz;
    Jq[1][0] = 0.0, Jq[1][1] = iz, Jq[1][2] = -y * iz;
  } else {
    Dual<4> xu4, yu4;
    ba_omni_unit(dual_var<4>(x0, 0), dual_var<4>(x1, 1), dual_var<4>(x2, 2), dual_var<4>(cp[11], 3), xu4, yu4);
    Dual<6> xd6, yd6;
    ba_omni_distort(dual_var<6>(xu4.v, 0), dual_var<6>(yu4.v, 1), dual_var<6>(cp[12], 2), dual_var<6>(cp[13], 3),
                    dual_var<6>(cp[14], 4), dual_var<6>(cp[15], 5), xd6, yd6);
    const double fx = cp[6], sk = cp[7], cx = cp[8], fy = cp[9], cy = cp[10];
    const double xd = xd6.v, yd = yd6.v;
    r[0] = fx * xd + sk * yd + cx - ob[0];
    r[1] = fy * yd + cy - ob[1];
    // d (u, v) / d (xd, yd) = [[fx, sk], [0, fy]]; through the distortion's 2 x 2 to (xu, yu)
    double G[2][2];  // d (u, v) / d (xu, yu)
    for (int j = 0; j < 2; ++j) {
      G[0][j] = fx * xd6.d[j] + sk * yd6.d[j];
      G[1][j] = fy * yd6.d[j];
    }
    for (int j = 0; j < 3; ++j) {
      Jq[0][j] = G[0][0] * xu4.d[j] + G[0][1] * yu4.d[j];
      Jq[1][j] = G[1][0] * xu4.d[j] + G[1][1] * yu4.d[j];
    }
    A[0 * P + 6] = xd, A[1 * P + 6] = 0.0;   // K00
    A[0 * P + 7] = yd, A[1 * P + 7] = 0.0;   // K01
    A[0 * P + 8] = 1.0, A[1 * P + 8] = 0.0;  // K02
    A[0 * P + 9] = 0.0, A[1 * P + 9] = yd;   // K11
    A[0 * P + 10] = 0.0, A[1 * P + 10] = 1.0;  // K12
    A[0 * P + 11] = G[0][0] * xu4.d[3] + G[0][1] * yu4.d[3];  // xi
    A[1 * P + 11] = G[1][0] * xu4.d[3] + G[1][1] * yu4.d[3];
    for (int j = 0; j < 4; ++j) {  // D
      A[0 * P + 12 + j] = fx * xd6.d[2 + j] + sk * yd6.d[2 + j];
      A[1 * P + 12 + j] = fy * yd6.d[2 + j];
    }
  }
  for (int k = 0; k < 3; ++k) {
    const double* D = dR + 9 * k;  // d Xc / d rvec_k = dR_k X
    const double d0 = D[0] * X[0] + D[1] * X[1] + D[2] * X[2];
    const double d1 = D[3] * X[0] + D[4] * X[1] + D[5] * X[2];
    const double d2 = D[6] * X[0] + D[7] * X[1] + D[8] * X[2];
    for (int row = 0; row < 2; ++row) {
      A[row * P + k] = Jq[row][0] * d0 + Jq[row][1] * d1 + Jq[row][2] * d2;
      A[row * P + 3 + k] = Jq[row][k];
      B[row * 3 + k] = Jq[row][0] * R[k] + Jq[row][1] * R[3 + k] + Jq[row][2] * R[6 + k];
    }
  }
}

}  // namespace mq
