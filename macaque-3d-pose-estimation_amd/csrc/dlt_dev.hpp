// Device helpers shared by the float64 geometry kernels (geometry.hip), the tracklet lift (tracklet.hip)
// and the candidate kernels (candidates.hip): the camera row accessor, the one-sided Jacobi SVD, the
// mvpose pinv DLT solve and the homogeneous DLT.
// Translation units including this are built with -ffp-contract=off (the numpy oracle's rounding order).
#pragma once
#include "common.hpp"

namespace mq {

__device__ __forceinline__ const CamParams& cam_at(const double* cams, int c) {
  return *reinterpret_cast<const CamParams*>(cams + 24 * c);
}

// One-sided (Hestenes) Jacobi SVD of an m x N matrix held as N columns of length M
// (unused rows zero).  Returns the right singular vectors in V and the column
// norms (singular values) in sig.
template <int M, int N>
__device__ __forceinline__ void jacobi_svd(double (&a)[N][M], double (&V)[N][N], double (&sig)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < N - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
        for (int i = 0; i < M; ++i) {
          alpha += a[p][i] * a[p][i];
          beta += a[q][i] * a[q][i];
          gamma += a[p][i] * a[q][i];
        }
        if (fabs(gamma) > 1e-15 * sqrt(alpha * beta) && gamma != 0.0) {
          rotated = true;
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + t * t);
          const double s = c * t;
#pragma unroll
          for (int i = 0; i < M; ++i) {
            const double ap = a[p][i], aq = a[q][i];
            a[p][i] = c * ap - s * aq;
            a[q][i] = s * ap + c * aq;
          }
#pragma unroll
          for (int i = 0; i < N; ++i) {
            const double vp = V[p][i], vq = V[q][i];
            V[p][i] = c * vp - s * vq;
            V[q][i] = s * vp + c * vq;
          }
        }
      }
    }
    if (!rotated) break;
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double s = 0;
#pragma unroll
    for (int i = 0; i < M; ++i) s += a[j][i] * a[j][i];
    sig[j] = sqrt(s);
  }
}

// mvpose inhomogeneous DLT of one point (multicam_toolbox.py:433-486): X = pinv(A[:, :3]) A[:, 3],
// P = -X, over the cameras flagged in `use` with undistorted coordinates (x[c], y[c]); NaN with fewer
// than two cameras.
template <int MAXC>
__device__ __forceinline__ void pinv_dlt_solve(const double* cams, int C, const double* x, const double* y,
                                               unsigned use, double out[3]) {
  double a[3][2 * MAXC], b[2 * MAXC];
  int cnt = 0;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const bool on = (c < C) && ((use >> c) & 1u);
    if (on) {
      ++cnt;
      const CamParams& cp = cam_at(cams, c);
      const double P0[4] = {cp.R[0], cp.R[1], cp.R[2], cp.t[0]};
      const double P1[4] = {cp.R[3], cp.R[4], cp.R[5], cp.t[1]};
      const double P2[4] = {cp.R[6], cp.R[7], cp.R[8], cp.t[2]};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a[k][2 * c] = x[c] * P2[k] - P0[k];
        a[k][2 * c + 1] = y[c] * P2[k] - P1[k];
      }
      b[2 * c] = x[c] * P2[3] - P0[3];
      b[2 * c + 1] = y[c] * P2[3] - P1[3];
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) a[k][2 * c] = a[k][2 * c + 1] = 0.0;
      b[2 * c] = b[2 * c + 1] = 0.0;
    }
  }
  if (cnt < 2) {
    out[0] = out[1] = out[2] = NAN;
    return;
  }
  double V[3][3], sig[3];
  jacobi_svd<2 * MAXC, 3>(a, V, sig);
  const double smax = fmax(fmax(sig[0], sig[1]), sig[2]);
  double X[3] = {0, 0, 0};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (sig[j] > 1e-15 * smax) {
      double ub = 0;
#pragma unroll
      for (int i = 0; i < 2 * MAXC; ++i) ub += a[j][i] * b[i];
      const double w = ub / (sig[j] * sig[j]);
#pragma unroll
      for (int k = 0; k < 3; ++k) X[k] += V[j][k] * w;
    }
  }
  out[0] = -X[0];
  out[1] = -X[1];
  out[2] = -X[2];
}

// Homogeneous DLT (cameras.py:20-32) over the cameras flagged in `use`.
template <int MAXC>
__device__ __forceinline__ void dlt_point(const double* cams, int C, const double* ux, const double* uy,
                                          unsigned use, double out[3]) {
  double a[4][2 * MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const bool on = (c < C) && ((use >> c) & 1u);
    if (on) {
      const CamParams& cp = cam_at(cams, c);
      const double P0[4] = {cp.R[0], cp.R[1], cp.R[2], cp.t[0]};
      const double P1[4] = {cp.R[3], cp.R[4], cp.R[5], cp.t[1]};
      const double P2[4] = {cp.R[6], cp.R[7], cp.R[8], cp.t[2]};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a[k][2 * c] = ux[c] * P2[k] - P0[k];
        a[k][2 * c + 1] = uy[c] * P2[k] - P1[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a[k][2 * c] = 0.0;
        a[k][2 * c + 1] = 0.0;
      }
    }
  }
  double V[4][4], sig[4];
  jacobi_svd<2 * MAXC, 4>(a, V, sig);
  int jmin = 0;
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (sig[j] < sig[jmin]) jmin = j;
  double v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = V[jmin][k];
  out[0] = v[0] / v[3];
  out[1] = v[1] / v[3];
  out[2] = v[2] / v[3];
}

}  // namespace mq
