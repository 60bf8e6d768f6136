// Camera calibration from detected points: the fits behind the reference's calibrate_intrinsic
// (multicam_toolbox.py:74-116, cv2.calibrateCamera and cv2.omnidir.calibrate) and the pose-only fit of
// get_extrinsic_from_cagekeypoints (:213-242, cv2.solvePnP).  float64 throughout.
//
// One problem = one camera: <= 10 shared intrinsic slots and a 6-parameter pose per view.  It is bundle.hip's
// block structure with the roles swapped: the shared block is the intrinsics, the eliminated blocks are the
// 6 x 6 view poses.  With r = projection - pixel, J = [A | B_v] (intrinsic | pose columns), U = sum A^T A,
// V_v = B_v^T B_v, W_v = A^T B_v and Marquardt damping, one trial step of calib_lm is
//
//   linearise   the workgroup's waves take views w, w + CAL_W, ... ; lanes are the view's points (a view with more
//               than 64 points takes several passes) and leave their two Jacobian rows in shared memory; then one
//               lane per entry sums U_v, W_v, V_v, g over the points in index order.  Lanes 0..10 factor
//               V_v* = V_v + lambda diag V_v (6 x 6 Cholesky) and solve for the rows of Y_v = W_v V_v*^-1 and for
//               V_v*^-1 g_v, which go to the global workspace; one lane per entry adds U_v - Y_v W_v^T and
//               -g_p + Y_v g_v to the wave's share of the reduced system, views in index order.
//   solve       the waves' shares are added in wave order; thread 0 factors the <= 10 free columns.
//   backsub     one thread per view: delta pose_v = -V_v*^-1 g_v - Y_v^T delta p, the trial poses, the predicted
//               decrease and the step norm (fixed-pairing tree sums).
//   accelerate  a second pass over the points forms J^T f_vv, f_vv the second directional derivative of the residuals
//               along the step (one more projection per point); the stored factors turn it into the geodesic
//               acceleration a, and the trial step is delta + a / 2 when 2 |a| <= 0.75 |delta|.
//   cost        1/2 sum r^2 at the trial parameters; gain ratio, accept / reject and the lambda update are
//               bundle.hip's rules (Nielsen's factor floored at 1/10, lambda *= nu on a rejected step).
//
// The whole LM runs in one launch, one workgroup per problem: every loop is bounded by max_iter, the view count
// or the point count, there is no synchronisation between workgroups and no floating-point atomic, so a
// problem's result is the same bits on every run and does not depend on the problems it shares a launch with.
//
// Expected bound: latency.  One workgroup per problem leaves most of the device idle; the per-view work is a few
// thousand float64 operations between workgroup barriers.
#include <algorithm>
#include <cmath>
#include <vector>

#include "bundle.hpp"
#include "calib.hpp"
#include "calib_dev.hpp"
#include "camera.hpp"

namespace mq {
namespace {

static_assert(CAL_NI == CAL_NI_API, "the entry point's slot count is the kernels'");
static_assert(CAL_OMNIDIR == CAM_OMNIDIR && CAL_PINHOLE == CAM_PINHOLE, "calibration uses camera.hpp's model ids");

constexpr int CAL_W = 2;            // waves per workgroup
constexpr int CAL_T = 64 * CAL_W;   // threads per workgroup
constexpr int CAL_JS = 2 * (CAL_NC + 1);  // a point's record: two rows of 16 columns and the residual
// per-view sums, one lane per entry: U (10 x 10) | W (10 x 6) | V (6 x 6) | g (16) | cost
constexpr int CAL_OU = 0, CAL_OW = 100, CAL_OV = 160, CAL_OG = 196, CAL_OC = 212, CAL_NE = 213;
// reduced system: S (10 x 10) | rhs (10) | g_p (10) | diag U (10) | cost
constexpr int CAL_RS = 0, CAL_RR = 100, CAL_RG = 110, CAL_RD = 120, CAL_RC = 130, CAL_NR = 131;
// per-view record in the workspace: Y (10 x 6) | V*^-1 g_v (6) | diag V (6) | g_v (6) | Cholesky factor of V* (21,
// packed lower) | delta pose_v (6) | acceleration a_v (6)
constexpr int CAL_VB = 112, CAL_VL = 78, CAL_VD = 99, CAL_VA = 105;
constexpr double CAL_GH = 0.1;     // step of the second directional derivative, in units of the LM step
constexpr double CAL_GALPHA = 0.75;  // the acceleration is used when 2 |a| <= alpha |delta|
constexpr int CAL_EPL = (CAL_NE + 63) / 64, CAL_RPL = (CAL_NR + 63) / 64;  // entries per lane

__device__ __forceinline__ double block_sum(double* sm, int tid, double v) {
  sm[tid] = v;
  for (int s = CAL_T / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (tid < s) sm[tid] += sm[tid + s];
  }
  __syncthreads();
  const double r = sm[0];
  __syncthreads();
  return r;
}

struct CalView {
  const int* pt_prefix;
  const double* obj;
  const double* img;
  int v0, V, rounds;
};

// 1/2 sum r^2 of the problem at intrinsics k (shared) and poses `pose`; resid: (n_pts, 2) or null
template <int MODEL>
__device__ double cal_cost(const CalView& cv, const double* k, const double* pose, double* resid,
                           double (*sRot)[36], double* sm) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  double c = 0.0;
  for (int r = 0; r < cv.rounds; ++r) {
    const int v = r * CAL_W + w;
    const bool active = v < cv.V;
    if (active && lane == 0) ba_rodrigues(pose + 6 * (size_t)(cv.v0 + v), sRot[w]);
    __syncthreads();
    if (active) {
      const int p0 = cv.pt_prefix[cv.v0 + v], cnt = cv.pt_prefix[cv.v0 + v + 1] - p0;
      const double* t = pose + 6 * (size_t)(cv.v0 + v) + 3;
      for (int j = lane; j < cnt; j += 64) {
        double u, vv;
        cal_project<MODEL>(k, sRot[w], t, cv.obj + 3 * (size_t)(p0 + j), u, vv);
        const double r0 = u - cv.img[2 * (size_t)(p0 + j)], r1 = vv - cv.img[2 * (size_t)(p0 + j) + 1];
        c += 0.5 * (r0 * r0 + r1 * r1);
        if (resid) resid[2 * (size_t)(p0 + j)] = r0, resid[2 * (size_t)(p0 + j) + 1] = r1;
      }
    }
    __syncthreads();
  }
  return block_sum(sm, tid, c);
}

__device__ __forceinline__ void entry_cols(int e, int& ca, int& cb, double& sc) {
  sc = 1.0;
  if (e < CAL_OW) {
    ca = e / 10, cb = e - 10 * ca;
  } else if (e < CAL_OV) {
    const int f = e - CAL_OW;
    ca = f / 6, cb = CAL_NI + (f - 6 * ca);
  } else if (e < CAL_OG) {
    const int f = e - CAL_OV;
    ca = CAL_NI + f / 6, cb = CAL_NI + f % 6;
  } else if (e < CAL_OC) {
    ca = e - CAL_OG, cb = CAL_NC;
  } else {
    ca = cb = CAL_NC, sc = 0.5;
  }
}

// Cholesky of V* = V + lambda diag V (V: 36 doubles) in registers; false when it is not positive definite
__device__ __forceinline__ bool chol6(const double* Vs, double damp, double (&L)[6][6]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = Vs[j * 6 + j] * damp;
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0) || !isfinite(d)) ok = false, d = 1.0;
    d = sqrt(d);
    L[j][j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = Vs[i * 6 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / d;
    }
  }
  return ok;
}

__device__ __forceinline__ void chol6_solve(const double (&L)[6][6], double (&b)[6]) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i][k] * b[k];
    b[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = b[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * b[k];
    b[i] = s / L[i][i];
  }
}

enum { CI_MAXN = 0, CI_FAIL, CI_DONE, CI_OK, CI_WHICH, CI_NF, CI_N };
enum { CS_LAMBDA = 0, CS_NU, CS_COST, CS_PRED, CS_STEP2, CS_X2, CS_N };

template <int MODEL>
__global__ __launch_bounds__(CAL_T) void calib_lm(const int* __restrict__ view_prefix,
                                                  const int* __restrict__ pt_prefix,
                                                  const double* __restrict__ obj, const double* __restrict__ img,
                                                  const int* __restrict__ free_mask, double* intr, double* pose_a,
                                                  double* pose_b, double* viewbuf, double ftol, double xtol,
                                                  int max_iter, double* resid, double* __restrict__ info) {
  __shared__ double sJ[CAL_W][64][CAL_JS];
  __shared__ double sS[CAL_W][CAL_NE + 3];
  __shared__ double sY[CAL_W][66];
  __shared__ double sRot[CAL_W][36];
  __shared__ double sRot2[CAL_W][9];
  __shared__ double sKh[CAL_NI], sAp[CAL_NI];
  __shared__ int sIdx[CAL_NI];
  __shared__ double sRedW[CAL_W][CAL_NR + 1];
  __shared__ double sSys[CAL_NR + 1];
  __shared__ double sM[CAL_NI * CAL_NI], sDp[CAL_NI], sK[CAL_NI], sKt[CAL_NI];
  __shared__ double sm[CAL_T];
  __shared__ double sSt[CS_N];
  __shared__ int sI[CI_N];
  const int prob = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  CalView cv;
  cv.pt_prefix = pt_prefix, cv.obj = obj, cv.img = img;
  cv.v0 = view_prefix[prob];
  cv.V = view_prefix[prob + 1] - cv.v0;
  cv.rounds = (cv.V + CAL_W - 1) / CAL_W;
  const int v0 = cv.v0, V = cv.V;
  const int* mask = free_mask + prob * CAL_NI;
  if (tid < CAL_NI) sK[tid] = intr[prob * CAL_NI + tid];
  if (tid < CI_N) sI[tid] = 0;
  __syncthreads();
  {
    int mx = 0;
    for (int v = tid; v < V; v += CAL_T) mx = max(mx, pt_prefix[v0 + v + 1] - pt_prefix[v0 + v]);
    atomicMax(&sI[CI_MAXN], mx);
  }
  __syncthreads();
  const int passes = (sI[CI_MAXN] + 63) / 64;
  double cost = cal_cost<MODEL>(cv, sK, pose_a, nullptr, sRot, sm);
  const double cost0 = cost;
  int iters = 0, accepted = 0, n_lin = 0, stop = BA_STOP_MAX_ITER, nf = 0;
  for (int p = 0; p < CAL_NI; ++p) nf += mask[p] != 0;
  if (tid == 0) {
    sSt[CS_LAMBDA] = 1e-3, sSt[CS_NU] = 2.0;
    if (V == 0) sI[CI_DONE] = BA_STOP_LAMBDA;  // nothing to solve
  }
  __syncthreads();

  for (int it = 0; it < max_iter; ++it) {
    if (sI[CI_DONE]) break;
    double* pc = sI[CI_WHICH] ? pose_b : pose_a;
    double* pt = sI[CI_WHICH] ? pose_a : pose_b;
    const double lambda = sSt[CS_LAMBDA], damp = 1.0 + lambda;
    __syncthreads();
    if (tid == 0) sI[CI_FAIL] = 0;
    // ---- linearise
    double red[CAL_RPL];
    for (int k = 0; k < CAL_RPL; ++k) red[k] = 0.0;
    for (int r = 0; r < cv.rounds; ++r) {
      const int v = r * CAL_W + w;
      const bool active = v < V;
      const double* pose = pc + 6 * (size_t)(v0 + v);
      if (active && lane == 0) ba_rotation_jac(pose, sRot[w], sRot[w] + 9);
      double acc[CAL_EPL];
      for (int k = 0; k < CAL_EPL; ++k) acc[k] = 0.0;
      const int p0 = active ? pt_prefix[v0 + v] : 0;
      const int cnt = active ? pt_prefix[v0 + v + 1] - p0 : 0;
      __syncthreads();
      for (int pass = 0; pass < passes; ++pass) {
        const int j = pass * 64 + lane;
        if (j < cnt) {
          double rr[2], A[2 * CAL_NC];
          cal_obs_jac<MODEL>(sK, sRot[w], sRot[w] + 9, pose + 3, obj + 3 * (size_t)(p0 + j),
                             img + 2 * (size_t)(p0 + j), rr, A);
          double* o = sJ[w][lane];
          for (int c = 0; c < CAL_NC; ++c) o[c] = A[c], o[CAL_NC + 1 + c] = A[CAL_NC + c];
          o[CAL_NC] = rr[0], o[2 * CAL_NC + 1] = rr[1];
        }
        __syncthreads();
        const int m = min(64, cnt - pass * 64);
        for (int k = 0; k < CAL_EPL; ++k) {
          const int e = lane + 64 * k;
          if (e < CAL_NE) {
            int ca, cb;
            double sc;
            entry_cols(e, ca, cb, sc);
            double s = acc[k];
            for (int jj = 0; jj < m; ++jj) {
              const double* o = sJ[w][jj];
              s += sc * (o[ca] * o[cb] + o[CAL_NC + 1 + ca] * o[CAL_NC + 1 + cb]);
            }
            acc[k] = s;
          }
        }
        __syncthreads();
      }
      for (int k = 0; k < CAL_EPL; ++k)
        if (lane + 64 * k < CAL_NE) sS[w][lane + 64 * k] = acc[k];
      __syncthreads();
      // ---- the view's 6 x 6 block: lanes 0..9 a row of Y = W V*^-1, lane 10 V*^-1 g_v
      if (active && lane <= CAL_NI) {
        double L[6][6], b[6];
        const bool ok = chol6(sS[w] + CAL_OV, damp, L);
        const double* src = lane < CAL_NI ? sS[w] + CAL_OW + 6 * lane : sS[w] + CAL_OG + CAL_NI;
#pragma unroll
        for (int k = 0; k < 6; ++k) b[k] = src[k];
        chol6_solve(L, b);
        double* vb = viewbuf + (size_t)(v0 + v) * CAL_VB;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          sY[w][6 * lane + k] = b[k];
          vb[6 * lane + k] = b[k];
        }
        if (lane == CAL_NI) {
#pragma unroll
          for (int k = 0; k < 6; ++k) {
            vb[66 + k] = sS[w][CAL_OV + 7 * k];
            vb[72 + k] = sS[w][CAL_OG + CAL_NI + k];
#pragma unroll
            for (int q = 0; q <= k; ++q) vb[CAL_VL + k * (k + 1) / 2 + q] = L[k][q];
          }
          if (!ok) sI[CI_FAIL] = 1;
        }
      }
      __syncthreads();
      if (active) {
        const double* S = sS[w];
        const double* Y = sY[w];
        for (int k = 0; k < CAL_RPL; ++k) {
          const int f = lane + 64 * k;
          if (f < CAL_RR) {
            const int p = f / 10, q = f - 10 * p;
            double s = S[CAL_OU + f];
            for (int c = 0; c < 6; ++c) s -= Y[6 * p + c] * S[CAL_OW + 6 * q + c];
            red[k] += s;
          } else if (f < CAL_RG) {
            const int p = f - CAL_RR;
            double s = -S[CAL_OG + p];
            for (int c = 0; c < 6; ++c) s += Y[6 * p + c] * S[CAL_OG + CAL_NI + c];
            red[k] += s;
          } else if (f < CAL_RD) {
            red[k] += S[CAL_OG + (f - CAL_RG)];
          } else if (f < CAL_RC) {
            red[k] += S[CAL_OU + 11 * (f - CAL_RD)];
          } else if (f == CAL_RC) {
            red[k] += S[CAL_OC];
          }
        }
      }
      // sS and sY are next written after the barriers of the following round
    }
    for (int k = 0; k < CAL_RPL; ++k)
      if (lane + 64 * k < CAL_NR) sRedW[w][lane + 64 * k] = red[k];
    __syncthreads();
    for (int f = tid; f < CAL_NR; f += CAL_T) {
      double s = 0.0;
      for (int ww = 0; ww < CAL_W; ++ww) s += sRedW[ww][f];
      sSys[f] = s;
    }
    __syncthreads();
    ++n_lin;
    ++iters;
    // ---- reduced system on the free columns (in the mask, and seen: diag U > 0)
    if (tid == 0) {
      int* idx = sIdx;
      int n = 0;
      for (int p = 0; p < CAL_NI; ++p) {
        sDp[p] = 0.0;
        if (mask[p] && sSys[CAL_RD + p] > 0.0) idx[n++] = p;
      }
      sI[CI_NF] = n;
      bool ok = !sI[CI_FAIL];
      for (int a = 0; a < n; ++a)
        for (int b = 0; b <= a; ++b)
          sM[a * CAL_NI + b] = sSys[CAL_RS + idx[a] * 10 + idx[b]] + (a == b ? lambda * sSys[CAL_RD + idx[a]] : 0.0);
      double rhs[CAL_NI];
      for (int a = 0; a < n; ++a) rhs[a] = sSys[CAL_RR + idx[a]];
      for (int j = 0; j < n && ok; ++j) {
        double d = sM[j * CAL_NI + j];
        for (int k = 0; k < j; ++k) d -= sM[j * CAL_NI + k] * sM[j * CAL_NI + k];
        if (!(d > 0.0) || !isfinite(d)) {
          ok = false;
          break;
        }
        d = sqrt(d);
        sM[j * CAL_NI + j] = d;
        for (int i = j + 1; i < n; ++i) {
          double s = sM[i * CAL_NI + j];
          for (int k = 0; k < j; ++k) s -= sM[i * CAL_NI + k] * sM[j * CAL_NI + k];
          sM[i * CAL_NI + j] = s / d;
        }
      }
      if (ok) {
        for (int i = 0; i < n; ++i) {
          double s = rhs[i];
          for (int k = 0; k < i; ++k) s -= sM[i * CAL_NI + k] * rhs[k];
          rhs[i] = s / sM[i * CAL_NI + i];
        }
        for (int i = n - 1; i >= 0; --i) {
          double s = rhs[i];
          for (int k = i + 1; k < n; ++k) s -= sM[k * CAL_NI + i] * rhs[k];
          rhs[i] = s / sM[i * CAL_NI + i];
        }
        for (int a = 0; a < n; ++a) sDp[idx[a]] = rhs[a];
      }
      double pred = 0.0, step2 = 0.0, x2 = 0.0;
      for (int p = 0; p < CAL_NI; ++p) {
        const double d = sDp[p];
        pred += 0.5 * (lambda * sSys[CAL_RD + p] * d * d - sSys[CAL_RG + p] * d);
        step2 += d * d;
        x2 += sK[p] * sK[p];
      }
      sSt[CS_PRED] = pred, sSt[CS_STEP2] = step2, sSt[CS_X2] = x2;
      sI[CI_OK] = ok;
      nf = n;
    }
    __syncthreads();
    bool ok = sI[CI_OK] != 0;  // uniform
    double cost_try = 0.0, pred = 0.0, step2 = 0.0, x2 = 0.0;
    if (ok) {
      // ---- back-substitution, one thread per view: delta pose_v into the view's record
      double pv = 0.0, dn = 0.0;
      for (int v = tid; v < V; v += CAL_T) {
        double* vb = viewbuf + (size_t)(v0 + v) * CAL_VB;
        for (int c = 0; c < 6; ++c) {
          double d = -vb[60 + c];
          for (int p = 0; p < CAL_NI; ++p) d -= vb[6 * p + c] * sDp[p];
          vb[CAL_VD + c] = d;
          pv += 0.5 * (lambda * vb[66 + c] * d * d - vb[72 + c] * d);
          dn += d * d;
        }
      }
      if (tid < CAL_NI) sKh[tid] = sK[tid] + CAL_GH * sDp[tid];
      pred = sSt[CS_PRED] + block_sum(sm, tid, pv);
      const double nd2 = sSt[CS_STEP2] + block_sum(sm, tid, dn);
      // ---- geodesic acceleration (Transtrum and Sethna): with f_vv = 2 / h ((r(x + h delta) - r(x)) / h - J delta),
      // the second directional derivative of the residuals along the step, a = -(H + lambda D)^-1 J^T f_vv comes
      // out of the factorisations this trial step already has.  Without it the omnidir fit creeps along the
      // curved valley its barely identifiable xi leaves.
      double red2 = 0.0;  // lane p < 10: the wave's share of -g2_p + Y_v g2_v, g2 = J^T f_vv
      for (int r = 0; r < cv.rounds; ++r) {
        const int v = r * CAL_W + w;
        const bool active = v < V;
        const double* pose = pc + 6 * (size_t)(v0 + v);
        double* vb = viewbuf + (size_t)(v0 + v) * CAL_VB;
        if (active && lane == 0) {
          ba_rotation_jac(pose, sRot[w], sRot[w] + 9);
          const double ph[3] = {pose[0] + CAL_GH * vb[CAL_VD], pose[1] + CAL_GH * vb[CAL_VD + 1],
                                pose[2] + CAL_GH * vb[CAL_VD + 2]};
          ba_rodrigues(ph, sRot2[w]);
        }
        const int p0 = active ? pt_prefix[v0 + v] : 0;
        const int cnt = active ? pt_prefix[v0 + v + 1] - p0 : 0;
        double acc2 = 0.0;  // lane e < 16: (J^T f_vv)[e] of the view
        __syncthreads();
        for (int pass = 0; pass < passes; ++pass) {
          const int j = pass * 64 + lane;
          if (j < cnt) {
            double rr[2], A[2 * CAL_NC];
            const double* X = obj + 3 * (size_t)(p0 + j);
            const double* ob = img + 2 * (size_t)(p0 + j);
            cal_obs_jac<MODEL>(sK, sRot[w], sRot[w] + 9, pose + 3, X, ob, rr, A);
            double jd0 = 0.0, jd1 = 0.0;
            for (int c = 0; c < CAL_NI; ++c) jd0 += A[c] * sDp[c], jd1 += A[CAL_NC + c] * sDp[c];
            for (int c = 0; c < 6; ++c) {
              jd0 += A[CAL_NI + c] * vb[CAL_VD + c];
              jd1 += A[CAL_NC + CAL_NI + c] * vb[CAL_VD + c];
            }
            const double th[3] = {pose[3] + CAL_GH * vb[CAL_VD + 3], pose[4] + CAL_GH * vb[CAL_VD + 4],
                                  pose[5] + CAL_GH * vb[CAL_VD + 5]};
            double uh, vh;
            cal_project<MODEL>(sKh, sRot2[w], th, X, uh, vh);
            double* o = sJ[w][lane];
            for (int c = 0; c < CAL_NC; ++c) o[c] = A[c], o[CAL_NC + 1 + c] = A[CAL_NC + c];
            o[CAL_NC] = 2.0 / CAL_GH * (((uh - ob[0]) - rr[0]) / CAL_GH - jd0);
            o[2 * CAL_NC + 1] = 2.0 / CAL_GH * (((vh - ob[1]) - rr[1]) / CAL_GH - jd1);
          }
          __syncthreads();
          const int m = min(64, cnt - pass * 64);
          if (lane < CAL_NC)
            for (int jj = 0; jj < m; ++jj) {
              const double* o = sJ[w][jj];
              acc2 += o[lane] * o[CAL_NC] + o[CAL_NC + 1 + lane] * o[2 * CAL_NC + 1];
            }
          __syncthreads();
        }
        if (lane < CAL_NC) sS[w][CAL_OG + lane] = acc2;
        __syncthreads();
        if (active && lane == 0) {  // V*^-1 g2_v through the stored factor
          double L[6][6], b[6];
#pragma unroll
          for (int k = 0; k < 6; ++k) {
            b[k] = sS[w][CAL_OG + CAL_NI + k];
#pragma unroll
            for (int q = 0; q < 6; ++q) L[k][q] = q <= k ? vb[CAL_VL + k * (k + 1) / 2 + q] : 0.0;
          }
          chol6_solve(L, b);
#pragma unroll
          for (int k = 0; k < 6; ++k) vb[CAL_VA + k] = b[k];
        }
        if (active && lane < CAL_NI) {
          double t = -sS[w][CAL_OG + lane];
          for (int c = 0; c < 6; ++c) t += vb[6 * lane + c] * sS[w][CAL_OG + CAL_NI + c];
          red2 += t;
        }
        // sS is next written after the barriers of the following round
      }
      if (lane < CAL_NI) sRedW[w][lane] = red2;
      __syncthreads();
      if (tid == 0) {
        const int n = sI[CI_NF];
        double rhs[CAL_NI];
        for (int p = 0; p < CAL_NI; ++p) sAp[p] = 0.0;
        for (int a = 0; a < n; ++a) {
          double t = 0.0;
          for (int ww = 0; ww < CAL_W; ++ww) t += sRedW[ww][sIdx[a]];
          rhs[a] = t;
        }
        for (int i = 0; i < n; ++i) {
          double t = rhs[i];
          for (int k = 0; k < i; ++k) t -= sM[i * CAL_NI + k] * rhs[k];
          rhs[i] = t / sM[i * CAL_NI + i];
        }
        for (int i = n - 1; i >= 0; --i) {
          double t = rhs[i];
          for (int k = i + 1; k < n; ++k) t -= sM[k * CAL_NI + i] * rhs[k];
          rhs[i] = t / sM[i * CAL_NI + i];
        }
        for (int a = 0; a < n; ++a) sAp[sIdx[a]] = rhs[a];
      }
      __syncthreads();
      double an = 0.0;
      for (int v = tid; v < V; v += CAL_T) {
        double* vb = viewbuf + (size_t)(v0 + v) * CAL_VB;
        for (int c = 0; c < 6; ++c) {
          double a = -vb[CAL_VA + c];
          for (int p = 0; p < CAL_NI; ++p) a -= vb[6 * p + c] * sAp[p];
          vb[CAL_VA + c] = a;
          an += a * a;
        }
      }
      double na2 = block_sum(sm, tid, an);
      for (int p = 0; p < CAL_NI; ++p) na2 += sAp[p] * sAp[p];
      const bool use_acc = 2.0 * sqrt(na2) <= CAL_GALPHA * sqrt(nd2);  // false on a non-finite acceleration
      // ---- the trial parameters
      double sv = 0.0, xv = 0.0;
      for (int v = tid; v < V; v += CAL_T) {
        const double* vb = viewbuf + (size_t)(v0 + v) * CAL_VB;
        for (int c = 0; c < 6; ++c) {
          const double d = use_acc ? vb[CAL_VD + c] + 0.5 * vb[CAL_VA + c] : vb[CAL_VD + c];
          const double x = pc[6 * (size_t)(v0 + v) + c];
          pt[6 * (size_t)(v0 + v) + c] = x + d;
          sv += d * d;
          xv += x * x;
        }
      }
      double sp = 0.0;
      for (int p = 0; p < CAL_NI; ++p) {
        const double d = use_acc ? sDp[p] + 0.5 * sAp[p] : sDp[p];
        sp += d * d;
        if (tid == p) sKt[p] = sK[p] + d;
      }
      step2 = sp + block_sum(sm, tid, sv);
      x2 = sSt[CS_X2] + block_sum(sm, tid, xv);
      cost_try = cal_cost<MODEL>(cv, sKt, pt, nullptr, sRot, sm);
      ok = isfinite(cost_try) && isfinite(pred) && pred > 0.0;
    }
    // ---- accept / reject: every thread takes the same branch on the same numbers
    const double actual = cost - cost_try;
    const bool tiny = ok && sqrt(step2) < xtol * (xtol + sqrt(x2));
    int done = 0;
    if (ok && actual > 0.0) {
      const double rho = actual / pred;
      ++accepted;
      const double t = 2.0 * rho - 1.0;
      const double before = cost;
      cost = cost_try;
      if (rho > 0.25 && actual < ftol * before)
        done = BA_STOP_FTOL;
      else if (tiny)
        done = BA_STOP_XTOL;
      __syncthreads();
      if (tid < CAL_NI) sK[tid] = sKt[tid];
      if (tid == 0) {
        sSt[CS_LAMBDA] = fmax(lambda * fmax(0.1, 1.0 - t * t * t), 1e-12);
        sSt[CS_NU] = 2.0;
        sI[CI_WHICH] ^= 1;
        sI[CI_DONE] = done;
      }
    } else {
      const double nu = sSt[CS_NU];
      if (tiny || cost == 0.0)
        done = BA_STOP_XTOL;
      else if (!(lambda * nu < 1e16))
        done = BA_STOP_LAMBDA;
      __syncthreads();
      if (tid == 0) {
        sSt[CS_LAMBDA] = lambda * nu;
        sSt[CS_NU] = nu * 2.0;
        sI[CI_DONE] = done;
      }
    }
    __syncthreads();
  }
  __syncthreads();
  if (sI[CI_DONE]) stop = sI[CI_DONE];
  const double* pc = sI[CI_WHICH] ? pose_b : pose_a;
  if (resid) cal_cost<MODEL>(cv, sK, pc, resid, sRot, sm);
  if (pc != pose_a)
    for (int e = tid; e < 6 * V; e += CAL_T) pose_a[6 * (size_t)v0 + e] = pc[6 * (size_t)v0 + e];
  if (tid < CAL_NI) intr[prob * CAL_NI + tid] = sK[tid];
  if (tid == 0) {
    double* o = info + 8 * (size_t)prob;
    o[0] = cost0, o[1] = cost, o[2] = iters, o[3] = stop;
    o[4] = accepted, o[5] = sSt[CS_LAMBDA], o[6] = n_lin, o[7] = nf + 6 * V;
  }
}

// ----------------------------------------------------------------------------- starts
// per-view record of the init: c (3) | E (9) | H (9)
constexpr int CAL_IB = 21;

__device__ __forceinline__ CamParams cam_from_slots(int model, const double* k) {
  CamParams cp;
  if (model == CAL_PINHOLE) {
    cp.fx = k[0], cp.fy = k[1], cp.skew = 0.0, cp.cx = k[2], cp.cy = k[3], cp.xi = 0.0;
    cp.k1 = k[4], cp.k2 = k[5], cp.p1 = k[6], cp.p2 = k[7], cp.k3 = k[8];
  } else {
    cp.fx = k[0], cp.fy = k[1], cp.skew = k[2], cp.cx = k[3], cp.cy = k[4], cp.xi = k[5];
    cp.k1 = k[6], cp.k2 = k[7], cp.p1 = k[8], cp.p2 = k[9], cp.k3 = 0.0;
  }
  for (int e = 0; e < 9; ++e) cp.R[e] = e % 4 == 0 ? 1.0 : 0.0;
  cp.t[0] = cp.t[1] = cp.t[2] = 0.0;
  cp.model = model;
  return cp;
}

// One thread per view: the image points the start works on (normalised through the given intrinsics, or the
// pixels), the object frame, and either the plane's homography or, for a non-planar view, the DLT pose.
__global__ __launch_bounds__(64) void calib_init_views(int model, int n_views, const int* __restrict__ prob_of_view,
                                                       const int* __restrict__ pt_prefix,
                                                       const double* __restrict__ obj,
                                                       const double* __restrict__ img,
                                                       const double* __restrict__ intr, int use_intrinsics,
                                                       double* uvn, double* initbuf, double* pose,
                                                       int* __restrict__ status) {
  const int v = blockIdx.x * 64 + threadIdx.x;
  if (v >= n_views) return;
  const int p0 = pt_prefix[v], n = pt_prefix[v + 1] - p0;
  if (use_intrinsics) {
    const CamParams cp = cam_from_slots(model, intr + prob_of_view[v] * CAL_NI);
    for (int i = 0; i < n; ++i)
      cam_undistort(cp, img[2 * (size_t)(p0 + i)], img[2 * (size_t)(p0 + i) + 1], uvn[2 * (size_t)(p0 + i)],
                    uvn[2 * (size_t)(p0 + i) + 1]);
  } else {
    for (int i = 0; i < 2 * n; ++i) uvn[2 * (size_t)p0 + i] = img[2 * (size_t)p0 + i];
  }
  double* ib = initbuf + (size_t)v * CAL_IB;
  double ev[3];
  cal_object_frame(obj + 3 * (size_t)p0, n, ib, ib + 3, ev);
  if (cal_is_planar(ev)) {
    cal_homography(obj + 3 * (size_t)p0, uvn + 2 * (size_t)p0, n, ib, ib + 3, ib + 12);
    status[v] = 0;
  } else if (!use_intrinsics) {
    status[v] = CAL_INIT_NONPLANAR;
  } else if (n < 6) {
    status[v] = CAL_INIT_FEW;
  } else {
    cal_pose_dlt(obj + 3 * (size_t)p0, uvn + 2 * (size_t)p0, n, ib, pose + 6 * (size_t)v);
    status[v] = -1;  // pose done
  }
}

// One thread per problem: Zhang's focal length from the problem's homographies, summed in view order; the
// centre at ((w - 1) / 2, (h - 1) / 2), no distortion; the omnidir start doubles fx, fy and sets xi = 1.
__global__ __launch_bounds__(64) void calib_init_focal(int model, int n_prob, const int* __restrict__ view_prefix,
                                                       const double* __restrict__ initbuf, int width, int height,
                                                       double* intr, int* __restrict__ pstatus) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= n_prob) return;
  const double cx = 0.5 * (width - 1), cy = 0.5 * (height - 1);
  double N[3] = {0, 0, 0}, b[2] = {0, 0}, fx = 0.0, fy = 0.0;
  for (int v = view_prefix[p]; v < view_prefix[p + 1]; ++v)
    cal_zhang_accumulate(initbuf + (size_t)v * CAL_IB + 12, cx, cy, N, b);
  if (view_prefix[p + 1] == view_prefix[p]) {  // no views: nothing to start from, the slots stay
    pstatus[p] = 0;
    return;
  }
  if (!cal_zhang_solve(N, b, fx, fy)) {
    pstatus[p] = CAL_INIT_SINGULAR;
    return;
  }
  pstatus[p] = 0;
  double* k = intr + p * CAL_NI;
  for (int e = 0; e < CAL_NI; ++e) k[e] = 0.0;
  if (model == CAL_PINHOLE) {
    k[0] = fx, k[1] = fy, k[2] = cx, k[3] = cy;
  } else {
    k[0] = 2.0 * fx, k[1] = 2.0 * fy, k[3] = cx, k[4] = cy, k[5] = 1.0;
  }
}

// One thread per planar view: the pose from its homography.  K is the pinhole start (the halved omnidir fx, fy),
// or the identity when the points were normalised through given intrinsics.
__global__ __launch_bounds__(64) void calib_init_pose(int model, int n_views, const int* __restrict__ prob_of_view,
                                                      const double* __restrict__ initbuf,
                                                      const double* __restrict__ intr, int use_intrinsics,
                                                      double* pose, int* __restrict__ status) {
  const int v = blockIdx.x * 64 + threadIdx.x;
  if (v >= n_views) return;
  double* ps = pose + 6 * (size_t)v;
  if (status[v] == 0) {
    double fx = 1.0, fy = 1.0, cx = 0.0, cy = 0.0;
    if (!use_intrinsics) {
      const double* k = intr + prob_of_view[v] * CAL_NI;
      if (model == CAL_PINHOLE)
        fx = k[0], fy = k[1], cx = k[2], cy = k[3];
      else
        fx = 0.5 * k[0], fy = 0.5 * k[1], cx = k[3], cy = k[4];
    }
    const double* ib = initbuf + (size_t)v * CAL_IB;
    cal_pose_from_homography(ib + 12, fx, fy, cx, cy, ib, ib + 3, ps);
  }
  if (status[v] <= 0) {
    bool fin = true;
    for (int e = 0; e < 6; ++e) fin = fin && isfinite(ps[e]);
    status[v] = fin ? 0 : CAL_INIT_POSE;
  }
}

struct Layout {
  size_t intr, pose_a, pose_b, viewbuf, info, uvn, initbuf, ints, total;  // in doubles
  size_t i_view_prefix, i_pt_prefix, i_prob_of_view, i_status, i_pstatus, i_mask;  // in ints, from `ints`
};

Layout cal_layout(int n_prob, int n_views, int n_pts) {
  Layout l;
  size_t at = 0;
  auto take = [&](size_t doubles) {
    const size_t here = at;
    at += (doubles + 1) & ~(size_t)1;
    return here;
  };
  l.intr = take((size_t)n_prob * CAL_NI);
  l.pose_a = take((size_t)n_views * 6);
  l.pose_b = take((size_t)n_views * 6);
  l.viewbuf = take((size_t)n_views * CAL_VB);
  l.info = take((size_t)n_prob * 8);
  l.uvn = take((size_t)n_pts * 2);
  l.initbuf = take((size_t)n_views * CAL_IB);
  size_t ia = 0;
  auto itake = [&](size_t ints) {
    const size_t here = ia;
    ia += ints;
    return here;
  };
  l.i_view_prefix = itake((size_t)n_prob + 1);
  l.i_pt_prefix = itake((size_t)n_views + 1);
  l.i_prob_of_view = itake((size_t)n_views);
  l.i_status = itake((size_t)n_views);
  l.i_pstatus = itake((size_t)n_prob);
  l.i_mask = itake((size_t)n_prob * CAL_NI);
  l.ints = take((ia + 1) / 2);
  l.total = at;
  return l;
}

#define CAL_HIP(expr)                    \
  do {                                   \
    if ((expr) != hipSuccess) return -5; \
  } while (0)

}  // namespace

size_t calib_workspace_bytes(int n_prob, int n_views, int n_pts) {
  return cal_layout(n_prob, n_views, n_pts).total * sizeof(double);
}

int calib_init(int model, int n_prob, int n_views, int n_pts, const int* view_prefix, const int* pt_prefix,
               const double* obj, const double* img, int width, int height, int use_intrinsics, double* intr,
               double* poses, int* where, void* ws_, hipStream_t s) {
  const Layout l = cal_layout(n_prob, n_views, n_pts);
  double* ws = reinterpret_cast<double*>(ws_);
  int* wi = reinterpret_cast<int*>(ws + l.ints);
  std::vector<int> pov(std::max(n_views, 1));
  for (int p = 0; p < n_prob; ++p)
    for (int v = view_prefix[p]; v < view_prefix[p + 1]; ++v) pov[v] = p;
  if (n_views == 0) return 0;
  CAL_HIP(hipMemcpyAsync(wi + l.i_view_prefix, view_prefix, sizeof(int) * (n_prob + 1), hipMemcpyHostToDevice, s));
  CAL_HIP(hipMemcpyAsync(wi + l.i_pt_prefix, pt_prefix, sizeof(int) * (n_views + 1), hipMemcpyHostToDevice, s));
  CAL_HIP(hipMemcpyAsync(wi + l.i_prob_of_view, pov.data(), sizeof(int) * n_views, hipMemcpyHostToDevice, s));
  CAL_HIP(hipMemcpyAsync(ws + l.intr, intr, sizeof(double) * n_prob * CAL_NI, hipMemcpyHostToDevice, s));
  const int gv = (n_views + 63) / 64, gp = (n_prob + 63) / 64;
  hipLaunchKernelGGL(calib_init_views, dim3(gv), dim3(64), 0, s, model, n_views, wi + l.i_prob_of_view,
                     wi + l.i_pt_prefix, obj, img, ws + l.intr, use_intrinsics, ws + l.uvn, ws + l.initbuf,
                     ws + l.pose_a, wi + l.i_status);
  CAL_HIP(hipGetLastError());
  std::vector<int> st(n_views), pst(n_prob, 0);
  CAL_HIP(hipMemcpyAsync(st.data(), wi + l.i_status, sizeof(int) * n_views, hipMemcpyDeviceToHost, s));
  CAL_HIP(hipStreamSynchronize(s));
  for (int v = 0; v < n_views; ++v)
    if (st[v] > 0) {
      *where = v;
      return st[v];
    }
  if (!use_intrinsics) {
    hipLaunchKernelGGL(calib_init_focal, dim3(gp), dim3(64), 0, s, model, n_prob, wi + l.i_view_prefix,
                       ws + l.initbuf, width, height, ws + l.intr, wi + l.i_pstatus);
    CAL_HIP(hipGetLastError());
    CAL_HIP(hipMemcpyAsync(pst.data(), wi + l.i_pstatus, sizeof(int) * n_prob, hipMemcpyDeviceToHost, s));
    CAL_HIP(hipStreamSynchronize(s));
    for (int p = 0; p < n_prob; ++p)
      if (pst[p] > 0) {
        *where = p;
        return pst[p];
      }
  }
  hipLaunchKernelGGL(calib_init_pose, dim3(gv), dim3(64), 0, s, model, n_views, wi + l.i_prob_of_view,
                     ws + l.initbuf, ws + l.intr, use_intrinsics, ws + l.pose_a, wi + l.i_status);
  CAL_HIP(hipGetLastError());
  CAL_HIP(hipMemcpyAsync(st.data(), wi + l.i_status, sizeof(int) * n_views, hipMemcpyDeviceToHost, s));
  CAL_HIP(hipStreamSynchronize(s));
  for (int v = 0; v < n_views; ++v)
    if (st[v] > 0) {
      *where = v;
      return st[v];
    }
  std::vector<double> hi((size_t)n_prob * CAL_NI), hp((size_t)n_views * 6);
  CAL_HIP(hipMemcpyAsync(hi.data(), ws + l.intr, sizeof(double) * hi.size(), hipMemcpyDeviceToHost, s));
  CAL_HIP(hipMemcpyAsync(hp.data(), ws + l.pose_a, sizeof(double) * hp.size(), hipMemcpyDeviceToHost, s));
  CAL_HIP(hipStreamSynchronize(s));
  std::copy(hi.begin(), hi.end(), intr);
  std::copy(hp.begin(), hp.end(), poses);
  return 0;
}

int calibrate_views(int model, int n_prob, int n_views, int n_pts, const int* view_prefix, const int* pt_prefix,
                    const double* obj, const double* img, const uint8_t* free_mask, double ftol, double xtol,
                    int max_iter, double* intr, double* poses, double* resid, double* info, void* ws_,
                    hipStream_t s) {
  const Layout l = cal_layout(n_prob, n_views, n_pts);
  double* ws = reinterpret_cast<double*>(ws_);
  int* wi = reinterpret_cast<int*>(ws + l.ints);
  std::vector<int> hm((size_t)n_prob * CAL_NI);
  for (size_t e = 0; e < hm.size(); ++e) hm[e] = free_mask[e] != 0;
  CAL_HIP(hipMemcpyAsync(wi + l.i_view_prefix, view_prefix, sizeof(int) * (n_prob + 1), hipMemcpyHostToDevice, s));
  CAL_HIP(hipMemcpyAsync(wi + l.i_pt_prefix, pt_prefix, sizeof(int) * (n_views + 1), hipMemcpyHostToDevice, s));
  CAL_HIP(hipMemcpyAsync(wi + l.i_mask, hm.data(), sizeof(int) * hm.size(), hipMemcpyHostToDevice, s));
  CAL_HIP(hipMemcpyAsync(ws + l.intr, intr, sizeof(double) * n_prob * CAL_NI, hipMemcpyHostToDevice, s));
  if (n_views > 0)
    CAL_HIP(hipMemcpyAsync(ws + l.pose_a, poses, sizeof(double) * n_views * 6, hipMemcpyHostToDevice, s));
  if (model == CAL_PINHOLE)
    hipLaunchKernelGGL(calib_lm<CAL_PINHOLE>, dim3(n_prob), dim3(CAL_T), 0, s, wi + l.i_view_prefix,
                       wi + l.i_pt_prefix, obj, img, wi + l.i_mask, ws + l.intr, ws + l.pose_a, ws + l.pose_b,
                       ws + l.viewbuf, ftol, xtol, max_iter, resid, ws + l.info);
  else
    hipLaunchKernelGGL(calib_lm<CAL_OMNIDIR>, dim3(n_prob), dim3(CAL_T), 0, s, wi + l.i_view_prefix,
                       wi + l.i_pt_prefix, obj, img, wi + l.i_mask, ws + l.intr, ws + l.pose_a, ws + l.pose_b,
                       ws + l.viewbuf, ftol, xtol, max_iter, resid, ws + l.info);
  CAL_HIP(hipGetLastError());
  std::vector<double> hi((size_t)n_prob * CAL_NI), hp((size_t)n_views * 6), hinfo((size_t)n_prob * 8);
  CAL_HIP(hipMemcpyAsync(hi.data(), ws + l.intr, sizeof(double) * hi.size(), hipMemcpyDeviceToHost, s));
  if (n_views > 0)
    CAL_HIP(hipMemcpyAsync(hp.data(), ws + l.pose_a, sizeof(double) * hp.size(), hipMemcpyDeviceToHost, s));
  CAL_HIP(hipMemcpyAsync(hinfo.data(), ws + l.info, sizeof(double) * hinfo.size(), hipMemcpyDeviceToHost, s));
  CAL_HIP(hipStreamSynchronize(s));
  std::copy(hi.begin(), hi.end(), intr);
  std::copy(hp.begin(), hp.end(), poses);
  std::copy(hinfo.begin(), hinfo.end(), info);
  return 0;
}

}  // namespace mq
