// Bundle adjustment of the camera rig on marker traces: multicam_toolbox.optimize_extrinsic (:488-636, mode 0:
// 6 extrinsic parameters per camera, residual on undistorted points) and optimize_all_camera_params (:638-824,
// mode 1: 16 parameters per camera, residual = omnidir projection - pixel), and aniposelib's
// CameraGroup.bundle_adjust (cameras.py:894-980, mode 2: rvec, tvec, f, k1, k2 per camera, a camera model per
// camera, residual = projection of the reduced model - pixel).  float64 throughout.
//
// Solver: Levenberg-Marquardt on the Schur complement of the point blocks, Marquardt (diagonal) scaling.  It
// stands in for scipy's least_squares(method='trf', x_scale='jac'); it is not a restatement of it.  With
// r = projection - observation, J = [A | B] (camera | point columns), U_c = sum A^T A, V_i = sum B^T B,
// W_ci = A^T B, g = J^T r and the damped U* = U + lambda diag U, V* likewise, one trial step is
//
//   ba_linearise   chunks of 64 points per workgroup.  Phase A, one thread per point: walk the point's <= C
//                  observations, form A (2 x P) and B (2 x 3) by dual numbers (bundle_dev.hpp), keep V_i and g_i
//                  in registers, invert V_i*, and leave W_ci, Y_ci = W_ci V_i*^-1, A and A^T r of every
//                  observation in the workspace.  Phase B, one thread per entry of the reduced system: sum the
//                  chunk's contributions U*_cc' - Y_ci W_c'i^T and -g_c + W_ci V_i*^-1 g_i over its points in
//                  index order into this workgroup's partial.  A workgroup takes chunks g, g + G, ... in order.
//   ba_reduce      sums the G partials in index order: no floating-point atomics anywhere, so the reduced system
//                  -- and with it every output -- is the same bits on every run.
//   host           Cholesky of the <= 256 free camera unknowns (columns outside the free mask and unobserved
//                  columns removed), the gain ratio, accept / reject and the lambda update (Nielsen's rule,
//                  floor 1/10).
//   ba_backsub     delta X_i = -V_i*^-1 g_i - Y_ci^T delta c_c per point, the trial points, and per-workgroup
//                  tree sums of the points' share of the predicted decrease and of |delta X|^2, |X|^2.
//   ba_cost        cost 1/2 sum r^2 at the trial cameras and points, per-workgroup tree sums (fixed pairing).
//
// Expected bound: latency, not arithmetic.  One trial step is four short launches, two small host round trips and
// a <= 256^2 host Cholesky; the per-point work is a few hundred float64 operations and the chunk sums read the
// workspace back from L2.
#include <algorithm>
#include <cmath>
#include <vector>

#include "bundle.hpp"
#include "bundle_dev.hpp"
#include "camera.hpp"

namespace mq {
namespace {

static_assert(BA_MAXC == BA_MAXC_API, "the entry point's camera limit is the kernels' shared-array size");
static_assert(BA_GP == BA_GP_API && BA_GFIX == BA_GFIX_API, "the entry point's mode-2 row is the kernels'");
static_assert(BA_CAM_OMNIDIR == CAM_OMNIDIR && BA_CAM_PINHOLE == CAM_PINHOLE && BA_CAM_FISHEYE == CAM_FISHEYE,
              "mode 2 uses camera.hpp's model ids");
constexpr int BA_T = 256;      // threads per workgroup
constexpr int BA_CHUNK = 64;   // points per chunk (phase A threads)
constexpr int BA_MAXG = 128;   // workgroups (partials) of ba_linearise
constexpr int BA_PT = 10;      // per-point record: V*^-1 g (3), diag V (3), g (3), cost

// shared-memory stride of a camera: its parameters, and in mode 2 the fixed data next to them
__host__ __device__ constexpr int ba_stride(int mode) { return mode == 2 ? BA_GROW : BA_MAXP; }

// one camera's row into shared memory: P parameters from cam, in mode 2 followed by its BA_GFIX fixed doubles
template <int MODE>
__device__ __forceinline__ void load_camera(double* row, const double* __restrict__ cam,
                                            const double* __restrict__ fix, int c) {
  constexpr int P = ba_nparams(MODE);
  for (int p = 0; p < P; ++p) row[p] = cam[c * P + p];
  if (MODE == 2)
    for (int q = 0; q < BA_GFIX; ++q) row[P + q] = fix[c * BA_GFIX + q];
}

// fixed-pairing tree sum of sm[0 .. BA_T) into sm[0]
__device__ __forceinline__ void tree_sum(double* sm, int tid) {
  for (int s = BA_T / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (tid < s) sm[tid] += sm[tid + s];
  }
  __syncthreads();
}

template <int MODE>
__global__ __launch_bounds__(BA_T) void ba_linearise(const double* __restrict__ cam, const double* __restrict__ fix,
                                                     const double* __restrict__ X,
                                                     const double* __restrict__ obs,
                                                     const uint8_t* __restrict__ use, int C, int N, double lambda,
                                                     int n_chunks, double* obsbuf, double* ptbuf,
                                                     double* __restrict__ partial) {
  constexpr int P = ba_nparams(MODE);
  constexpr int CS = ba_stride(MODE);
  constexpr int OS = 9 * P;  // per observation: W (3P) | Y (3P) | A row 0 (P) | A row 1 (P) | A^T r (P)
  __shared__ double sC[BA_MAXC * CS];
  __shared__ double sR[BA_MAXC * 9];
  __shared__ double sdR[BA_MAXC * 27];
  const int tid = threadIdx.x;
  const int n = C * P;
  const int L = n * n + 3 * n + 1;
  if (tid < C) {
    load_camera<MODE>(sC + tid * CS, cam, fix, tid);
    ba_rotation_jac(cam + tid * P, sR + tid * 9, sdR + tid * 27);
  }
  __syncthreads();
  const double damp = 1.0 + lambda;
  bool first = true;
  for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x, first = false) {
    const int base = chunk * BA_CHUNK;
    const int cnt = min(BA_CHUNK, N - base);
    // ---- phase A: one thread per point
    if (tid < cnt) {
      const int i = base + tid;
      const double Xi[3] = {X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2]};
      double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, cost = 0.0;
      bool seen = false;
      for (int c = 0; c < C; ++c) {
        double* o = obsbuf + ((size_t)i * C + c) * OS;
        if (use[(size_t)i * C + c]) {
          seen = true;
          double r[2], A[2 * P], B[6];
          ba_obs_jac<MODE>(sC + c * CS, sR + c * 9, sdR + c * 27, Xi, obs + ((size_t)c * N + i) * 2, r, A, B);
          V[0] += B[0] * B[0] + B[3] * B[3];
          V[1] += B[0] * B[1] + B[3] * B[4];
          V[2] += B[0] * B[2] + B[3] * B[5];
          V[3] += B[1] * B[1] + B[4] * B[4];
          V[4] += B[1] * B[2] + B[4] * B[5];
          V[5] += B[2] * B[2] + B[5] * B[5];
          for (int k = 0; k < 3; ++k) g[k] += B[k] * r[0] + B[3 + k] * r[1];
          cost += 0.5 * (r[0] * r[0] + r[1] * r[1]);
          for (int p = 0; p < P; ++p) {
            for (int k = 0; k < 3; ++k) o[3 * p + k] = A[p] * B[k] + A[P + p] * B[3 + k];
            o[6 * P + p] = A[p];
            o[7 * P + p] = A[P + p];
            o[8 * P + p] = A[p] * r[0] + A[P + p] * r[1];
          }
        } else {
          for (int e = 0; e < OS; ++e) o[e] = 0.0;
        }
      }
      // V* = V + lambda diag V; its inverse by cofactors (symmetric)
      const double a = V[0] * damp, b = V[1], c2 = V[2], d = V[3] * damp, e = V[4], f = V[5] * damp;
      double iv[6];
      iv[0] = d * f - e * e;
      iv[1] = c2 * e - b * f;
      iv[2] = b * e - c2 * d;
      iv[3] = a * f - c2 * c2;
      iv[4] = b * c2 - a * e;
      iv[5] = a * d - b * b;
      const double det = a * iv[0] + b * iv[1] + c2 * iv[2];
      const double idet = det > 0.0 ? 1.0 / det : 0.0;  // a point nobody sees: no step, no contribution
      // Mode 2 keeps points one camera sees: V is rank 2 and only the damping makes V* invertible.  Where the
      // inverse fails for a point that is seen, the cost slot carries NaN and the host rejects the step.
      if (MODE == 2 && seen && !(det > 0.0 && isfinite(idet))) cost = __builtin_nan("");
      for (int k = 0; k < 6; ++k) iv[k] *= idet;
      double* pt = ptbuf + (size_t)i * BA_PT;
      pt[0] = iv[0] * g[0] + iv[1] * g[1] + iv[2] * g[2];
      pt[1] = iv[1] * g[0] + iv[3] * g[1] + iv[4] * g[2];
      pt[2] = iv[2] * g[0] + iv[4] * g[1] + iv[5] * g[2];
      pt[3] = V[0], pt[4] = V[3], pt[5] = V[5];
      pt[6] = g[0], pt[7] = g[1], pt[8] = g[2];
      pt[9] = cost;
      for (int c = 0; c < C; ++c) {
        if (!use[(size_t)i * C + c]) continue;
        double* o = obsbuf + ((size_t)i * C + c) * OS;
        for (int p = 0; p < P; ++p) {
          const double w0 = o[3 * p], w1 = o[3 * p + 1], w2 = o[3 * p + 2];
          o[3 * P + 3 * p + 0] = w0 * iv[0] + w1 * iv[1] + w2 * iv[2];
          o[3 * P + 3 * p + 1] = w0 * iv[1] + w1 * iv[3] + w2 * iv[4];
          o[3 * P + 3 * p + 2] = w0 * iv[2] + w1 * iv[4] + w2 * iv[5];
        }
      }
    }
    __threadfence_block();
    __syncthreads();
    // ---- phase B: one thread per entry, the chunk's points in index order
    double* mine = partial + (size_t)blockIdx.x * L;
    for (int e = tid; e < L; e += BA_T) {
      double s = 0.0;
      if (e < n * n) {
        const int row = e / n, col = e - row * n;
        const int c = row / P, p = row - c * P, cc = col / P, q = col - cc * P;
        for (int j = 0; j < cnt; ++j) {
          const double* o1 = obsbuf + ((size_t)(base + j) * C + c) * OS;
          const double* o2 = obsbuf + ((size_t)(base + j) * C + cc) * OS;
          s -= o1[3 * P + 3 * p] * o2[3 * q] + o1[3 * P + 3 * p + 1] * o2[3 * q + 1] +
               o1[3 * P + 3 * p + 2] * o2[3 * q + 2];
          if (c == cc) {
            const double u = o1[6 * P + p] * o1[6 * P + q] + o1[7 * P + p] * o1[7 * P + q];
            s += row == col ? u * damp : u;
          }
        }
      } else if (e < n * n + 3 * n) {
        const int which = (e - n * n) / n, k = (e - n * n) - which * n;
        const int c = k / P, p = k - c * P;
        for (int j = 0; j < cnt; ++j) {
          const double* o1 = obsbuf + ((size_t)(base + j) * C + c) * OS;
          if (which == 0) {  // right-hand side: -g_c + W_ci V_i*^-1 g_i
            const double* pt = ptbuf + (size_t)(base + j) * BA_PT;
            s += o1[3 * p] * pt[0] + o1[3 * p + 1] * pt[1] + o1[3 * p + 2] * pt[2] - o1[8 * P + p];
          } else if (which == 1) {  // g_c
            s += o1[8 * P + p];
          } else {  // diag U
            s += o1[6 * P + p] * o1[6 * P + p] + o1[7 * P + p] * o1[7 * P + p];
          }
        }
      } else {
        for (int j = 0; j < cnt; ++j) s += ptbuf[(size_t)(base + j) * BA_PT + 9];
      }
      mine[e] = first ? s : mine[e] + s;
    }
  }
}

__global__ __launch_bounds__(BA_T) void ba_reduce(const double* __restrict__ partial, int G, int L,
                                                  double* __restrict__ out) {
  const int e = blockIdx.x * BA_T + threadIdx.x;
  if (e >= L) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += partial[(size_t)g * L + e];
  out[e] = s;
}

__global__ __launch_bounds__(BA_T) void ba_backsub(const double* __restrict__ obsbuf,
                                                   const double* __restrict__ ptbuf, const double* __restrict__ dc,
                                                   const double* __restrict__ X, int C, int N, int P, double lambda,
                                                   double* __restrict__ Xt, double* __restrict__ pr) {
  __shared__ double sD[BA_MAXC * BA_MAXP];
  __shared__ double sm[3][BA_T];
  const int tid = threadIdx.x;
  const int n = C * P, OS = 9 * P;
  for (int k = tid; k < n; k += BA_T) sD[k] = dc[k];
  __syncthreads();
  const int i = blockIdx.x * BA_T + tid;
  double pred = 0.0, sd = 0.0, sx = 0.0;
  if (i < N) {
    const double* pt = ptbuf + (size_t)i * BA_PT;
    double dx[3] = {-pt[0], -pt[1], -pt[2]};
    for (int c = 0; c < C; ++c) {
      const double* y = obsbuf + ((size_t)i * C + c) * OS + 3 * P;
      for (int p = 0; p < P; ++p) {
        const double d = sD[c * P + p];
        dx[0] -= y[3 * p] * d;
        dx[1] -= y[3 * p + 1] * d;
        dx[2] -= y[3 * p + 2] * d;
      }
    }
    for (int k = 0; k < 3; ++k) {
      const double x = X[3 * (size_t)i + k];
      Xt[3 * (size_t)i + k] = x + dx[k];
      pred += 0.5 * (lambda * pt[3 + k] * dx[k] * dx[k] - pt[6 + k] * dx[k]);
      sd += dx[k] * dx[k];
      sx += x * x;
    }
  }
  sm[0][tid] = pred, sm[1][tid] = sd, sm[2][tid] = sx;
  for (int s = BA_T / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (tid < s) {
      sm[0][tid] += sm[0][tid + s];
      sm[1][tid] += sm[1][tid + s];
      sm[2][tid] += sm[2][tid + s];
    }
  }
  if (tid == 0) {
    pr[4 * blockIdx.x + 0] = sm[0][0];
    pr[4 * blockIdx.x + 1] = sm[1][0];
    pr[4 * blockIdx.x + 2] = sm[2][0];
    pr[4 * blockIdx.x + 3] = 0.0;
  }
}

template <int MODE>
__global__ __launch_bounds__(BA_T) void ba_cost(const double* __restrict__ cam, const double* __restrict__ fix,
                                                const double* __restrict__ X, const double* __restrict__ obs,
                                                const uint8_t* __restrict__ use, int C, int N,
                                                double* __restrict__ resid, double* __restrict__ pc) {
  constexpr int P = ba_nparams(MODE);
  constexpr int CS = ba_stride(MODE);
  __shared__ double sC[BA_MAXC * CS];
  __shared__ double sR[BA_MAXC * 9];
  __shared__ double sm[BA_T];
  const int tid = threadIdx.x;
  if (tid < C) {
    load_camera<MODE>(sC + tid * CS, cam, fix, tid);
    ba_rodrigues(cam + tid * P, sR + tid * 9);
  }
  __syncthreads();
  const int i = blockIdx.x * BA_T + tid;
  double cost = 0.0;
  if (i < N) {
    const double Xi[3] = {X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2]};
    for (int c = 0; c < C; ++c) {
      double r[2] = {0.0, 0.0};
      if (use[(size_t)i * C + c]) {
        ba_obs_res<MODE>(sC + c * CS, sR + c * 9, Xi, obs + ((size_t)c * N + i) * 2, r);
        cost += 0.5 * (r[0] * r[0] + r[1] * r[1]);
      }
      if (resid) {
        resid[((size_t)i * C + c) * 2] = r[0];
        resid[((size_t)i * C + c) * 2 + 1] = r[1];
      }
    }
  }
  sm[tid] = cost;
  tree_sum(sm, tid);
  if (tid == 0) pc[blockIdx.x] = sm[0];
}

// in-place Cholesky M = L L^T (lower, row-major nf x nf) and solve; false when M is not positive definite
bool chol_solve(std::vector<double>& M, std::vector<double>& b, int nf) {
  for (int j = 0; j < nf; ++j) {
    double d = M[(size_t)j * nf + j];
    for (int k = 0; k < j; ++k) d -= M[(size_t)j * nf + k] * M[(size_t)j * nf + k];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    d = std::sqrt(d);
    M[(size_t)j * nf + j] = d;
    for (int i = j + 1; i < nf; ++i) {
      double s = M[(size_t)i * nf + j];
      for (int k = 0; k < j; ++k) s -= M[(size_t)i * nf + k] * M[(size_t)j * nf + k];
      M[(size_t)i * nf + j] = s / d;
    }
  }
  for (int i = 0; i < nf; ++i) {
    double s = b[i];
    for (int k = 0; k < i; ++k) s -= M[(size_t)i * nf + k] * b[k];
    b[i] = s / M[(size_t)i * nf + i];
  }
  for (int i = nf - 1; i >= 0; --i) {
    double s = b[i];
    for (int k = i + 1; k < nf; ++k) s -= M[(size_t)k * nf + i] * b[k];
    b[i] = s / M[(size_t)i * nf + i];
  }
  return true;
}

struct Layout {
  size_t obsbuf, ptbuf, partial, red, cam_a, cam_b, dc, xt, pr, pc, fix, total;
};

Layout ba_layout(int mode, int C, int N) {
  const size_t P = ba_nparams(mode), n = (size_t)C * P, L = n * n + 3 * n + 1;
  const size_t chunks = ((size_t)N + BA_CHUNK - 1) / BA_CHUNK;
  const size_t G = std::max<size_t>(1, std::min<size_t>(chunks, BA_MAXG));
  const size_t G2 = std::max<size_t>(1, ((size_t)N + BA_T - 1) / BA_T);
  Layout l;
  size_t at = 0;
  auto take = [&](size_t doubles) {
    const size_t here = at;
    at += (doubles + 1) & ~(size_t)1;
    return here;
  };
  l.obsbuf = take((size_t)N * C * 9 * P);
  l.ptbuf = take((size_t)N * BA_PT);
  l.partial = take(G * L);
  l.red = take(L);
  l.cam_a = take(n);
  l.cam_b = take(n);
  l.dc = take(n);
  l.xt = take((size_t)N * 3);
  l.pr = take(G2 * 4);
  l.pc = take(G2);
  l.fix = take(mode == 2 ? (size_t)C * BA_GFIX : 0);
  l.total = at;
  return l;
}

#define BA_HIP(expr)                 \
  do {                               \
    if ((expr) != hipSuccess) return -5; \
  } while (0)

template <int MODE>
int bundle_adjust_impl(int C, int N, double* cam, const double* cam_fixed, const uint8_t* free_mask, double* X,
                       const double* obs, const uint8_t* use, double ftol, double xtol, int max_iter, double* resid,
                       double* info, void* ws_, hipStream_t s) {
  constexpr int P = ba_nparams(MODE);
  const int n = C * P, L = n * n + 3 * n + 1;
  const int n_chunks = (N + BA_CHUNK - 1) / BA_CHUNK;
  const int G = std::max(1, std::min(n_chunks, BA_MAXG));
  const int G2 = std::max(1, (N + BA_T - 1) / BA_T);
  const Layout l = ba_layout(MODE, C, N);
  double* ws = reinterpret_cast<double*>(ws_);
  double *obsbuf = ws + l.obsbuf, *ptbuf = ws + l.ptbuf, *partial = ws + l.partial, *red = ws + l.red;
  double *cam_cur = ws + l.cam_a, *cam_try = ws + l.cam_b, *dc = ws + l.dc;
  double *x_cur = X, *x_try = ws + l.xt, *pr = ws + l.pr, *pc = ws + l.pc;
  const double* fix = MODE == 2 ? ws + l.fix : nullptr;

  std::vector<double> hcam(cam, cam + n), htry(n), hred(L), hdc(n), hpr((size_t)G2 * 4), hpc(G2);
  std::vector<double> M, rhs;
  std::vector<int> freeidx;

  auto cost_at = [&](const double* cam_d, const double* x_d, double* resid_d, double& out) -> int {
    hipLaunchKernelGGL(ba_cost<MODE>, dim3(G2), dim3(BA_T), 0, s, cam_d, fix, x_d, obs, use, C, N, resid_d, pc);
    BA_HIP(hipGetLastError());
    BA_HIP(hipMemcpyAsync(hpc.data(), pc, sizeof(double) * G2, hipMemcpyDeviceToHost, s));
    BA_HIP(hipStreamSynchronize(s));
    out = 0.0;
    for (int g = 0; g < G2; ++g) out += hpc[g];
    return 0;
  };

  BA_HIP(hipMemcpyAsync(cam_cur, hcam.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
  if (MODE == 2)
    BA_HIP(hipMemcpyAsync(ws + l.fix, cam_fixed, sizeof(double) * C * BA_GFIX, hipMemcpyHostToDevice, s));
  double cost = 0.0;
  int rc = cost_at(cam_cur, x_cur, nullptr, cost);
  if (rc) return rc;
  const double cost0 = cost;
  double lambda = 1e-3, nu = 2.0;
  int iters = 0, accepted = 0, n_lin = 0, stop = BA_STOP_MAX_ITER, nf = 0;

  while (iters < max_iter && N > 0) {
    hipLaunchKernelGGL(ba_linearise<MODE>, dim3(G), dim3(BA_T), 0, s, cam_cur, fix, x_cur, obs, use, C, N,
                       lambda, n_chunks, obsbuf, ptbuf, partial);
    BA_HIP(hipGetLastError());
    hipLaunchKernelGGL(ba_reduce, dim3((L + BA_T - 1) / BA_T), dim3(BA_T), 0, s, partial, G, L, red);
    BA_HIP(hipGetLastError());
    BA_HIP(hipMemcpyAsync(hred.data(), red, sizeof(double) * L, hipMemcpyDeviceToHost, s));
    BA_HIP(hipStreamSynchronize(s));
    ++n_lin;
    const double* Sm = hred.data();
    const double* rh = Sm + (size_t)n * n;
    const double* gc = rh + n;
    const double* du = gc + n;
    // free unknowns: in the free mask, and the camera is observed (diag U > 0)
    freeidx.clear();
    for (int k = 0; k < n; ++k)
      if (free_mask[k] && du[k] > 0.0) freeidx.push_back(k);
    nf = (int)freeidx.size();
    if (nf == 0) {
      stop = BA_STOP_LAMBDA;
      break;
    }
    M.assign((size_t)nf * nf, 0.0);
    rhs.assign(nf, 0.0);
    for (int a = 0; a < nf; ++a) {
      rhs[a] = rh[freeidx[a]];
      for (int b = 0; b <= a; ++b) M[(size_t)a * nf + b] = Sm[(size_t)freeidx[a] * n + freeidx[b]];
    }
    ++iters;
    // mode 2: a seen point whose damped 3 x 3 block could not be inverted (NaN in the cost slot) rejects the step
    bool ok = (MODE != 2 || std::isfinite(hred[(size_t)L - 1])) && chol_solve(M, rhs, nf);
    double cost_try = 0.0, pred = 0.0, step2 = 0.0, x2 = 0.0;
    if (ok) {
      std::fill(hdc.begin(), hdc.end(), 0.0);
      for (int a = 0; a < nf; ++a) hdc[freeidx[a]] = rhs[a];
      for (int k = 0; k < n; ++k) {
        htry[k] = hcam[k] + hdc[k];
        pred += 0.5 * (lambda * du[k] * hdc[k] * hdc[k] - gc[k] * hdc[k]);
        step2 += hdc[k] * hdc[k];
        x2 += hcam[k] * hcam[k];
      }
      BA_HIP(hipMemcpyAsync(dc, hdc.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
      BA_HIP(hipMemcpyAsync(cam_try, htry.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(ba_backsub, dim3(G2), dim3(BA_T), 0, s, obsbuf, ptbuf, dc, x_cur, C, N, P, lambda, x_try,
                         pr);
      BA_HIP(hipGetLastError());
      BA_HIP(hipMemcpyAsync(hpr.data(), pr, sizeof(double) * 4 * G2, hipMemcpyDeviceToHost, s));
      rc = cost_at(cam_try, x_try, nullptr, cost_try);
      if (rc) return rc;
      for (int g = 0; g < G2; ++g) {
        pred += hpr[4 * (size_t)g];
        step2 += hpr[4 * (size_t)g + 1];
        x2 += hpr[4 * (size_t)g + 2];
      }
      ok = std::isfinite(cost_try) && std::isfinite(pred) && pred > 0.0;
    }
    const double actual = cost - cost_try;
    const bool tiny = ok && std::sqrt(step2) < xtol * (xtol + std::sqrt(x2));
    if (ok && actual > 0.0) {
      const double rho = actual / pred;
      std::swap(cam_cur, cam_try);
      std::swap(x_cur, x_try);
      hcam = htry;
      ++accepted;
      // Nielsen's factor 1 - (2 rho - 1)^3, floored at Marquardt's 1/10 instead of 1/3: a step the model
      // predicted well takes the damping down fast, so the last steps are Gauss-Newton steps (on noise-free
      // observations the cost then falls to rounding level in as many steps as scipy's trust region needs)
      const double t = 2.0 * rho - 1.0;
      lambda = std::max(lambda * std::max(0.1, 1.0 - t * t * t), 1e-12);
      nu = 2.0;
      const double before = cost;
      cost = cost_try;
      if (rho > 0.25 && actual < ftol * before) {
        stop = BA_STOP_FTOL;
        break;
      }
      if (tiny) {
        stop = BA_STOP_XTOL;
        break;
      }
    } else {
      if (tiny || cost == 0.0) {
        stop = BA_STOP_XTOL;
        break;
      }
      lambda *= nu;
      nu *= 2.0;
      if (!(lambda < 1e16)) {
        stop = BA_STOP_LAMBDA;
        break;
      }
    }
  }

  if (x_cur != X) BA_HIP(hipMemcpyAsync(X, x_cur, sizeof(double) * 3 * (size_t)N, hipMemcpyDeviceToDevice, s));
  if (resid) {
    double again = 0.0;
    rc = cost_at(cam_cur, x_cur, resid, again);
    if (rc) return rc;
  }
  BA_HIP(hipStreamSynchronize(s));
  for (int k = 0; k < n; ++k) cam[k] = hcam[k];
  info[0] = cost0, info[1] = cost, info[2] = iters, info[3] = stop;
  info[4] = accepted, info[5] = lambda, info[6] = n_lin, info[7] = nf;
  return 0;
}

}  // namespace

size_t bundle_workspace_bytes(int mode, int C, int N) { return ba_layout(mode, C, N).total * sizeof(double); }

int bundle_adjust(int mode, int C, int N, double* cam, double* X, const double* obs, const uint8_t* use,
                  int fix_cam0, double ftol, double xtol, int max_iter, double* resid, double* info, void* ws,
                  hipStream_t s) {
  // fix_cam0 as a column mask: camera 0's rvec and tvec frozen, every other column free
  std::vector<uint8_t> free_mask((size_t)C * ba_nparams(mode), 1);
  if (fix_cam0) std::fill(free_mask.begin(), free_mask.begin() + 6, 0);
  if (mode == 0)
    return bundle_adjust_impl<0>(C, N, cam, nullptr, free_mask.data(), X, obs, use, ftol, xtol, max_iter, resid,
                                 info, ws, s);
  return bundle_adjust_impl<1>(C, N, cam, nullptr, free_mask.data(), X, obs, use, ftol, xtol, max_iter, resid, info,
                               ws, s);
}

int bundle_adjust_group(int C, int N, double* cam, const double* cam_fixed, const uint8_t* free_mask, double* X,
                        const double* obs, const uint8_t* use, double ftol, double xtol, int max_iter,
                        double* resid, double* info, void* ws, hipStream_t s) {
  return bundle_adjust_impl<2>(C, N, cam, cam_fixed, free_mask, X, obs, use, ftol, xtol, max_iter, resid, info, ws,
                               s);
}

}  // namespace mq
