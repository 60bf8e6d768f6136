// The scalar core of lsmr (scipy 1.15.3 sparse/linalg/_isolve/lsmr.py:29-460) as optim_trf.hip's kernels run it
// (optim_points); oracle/trf.py's lsmr_phased states the same in numpy.  The scalar functions compile for the host
// too: tests/trf_core_check.cpp runs them on dense matrices without a GPU.  The solver objects are built without FMA
// contraction, so an expression gives the same bits wherever it is inlined.  (optim_possible.hip still carries its
// own copy of this core: moving its kernels here kept their bits but not their speed, profiles/trf_core_ab.txt.)
//
// The phase order is the kernels': iteration k's recurrences run once alpha_k and beta_k are reduced (lsmr_recurrence,
// with the x / h / hbar coefficients for the caller's vectors) and its stop test one phase later, once |x_k| is
// (lsmr_istop).  The state lives in LSMR_NS doubles, S_* below.
//
// Device only: the 256-thread reductions whose fixed order makes every workgroup hold the same scalars bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif
#define LSMR_HD __host__ __device__ inline __attribute__((always_inline))

namespace mq {

// lsmr state slot
enum {
  S_ALPHABAR, S_RHO, S_RHOBAR, S_CBAR, S_SBAR, S_ZETABAR, S_ZETA, S_BETADD, S_BETAD, S_RHODOLD, S_TAUTILDEOLD,
  S_THETATILDE, S_D, S_NORMA2, S_MAXRBAR, S_MINRBAR, S_ITN, S_NORMR, S_NORMAR, S_NORMA, S_CONDA,
  S_CHAT, S_SHAT, S_ALPHAHAT  // sym_ortho(alphabar, damp) of the next iteration (depends on neither norm)
};
constexpr int LSMR_NS = 24;  // lsmr state doubles per slot
static_assert(S_ALPHAHAT < LSMR_NS, "lsmr state slot");

// scipy.sparse.linalg._isolve.lsqr._sym_ortho (np.sign(0) = 0)
LSMR_HD double sgn0(double a) { return a > 0 ? 1.0 : (a < 0 ? -1.0 : 0.0); }
LSMR_HD void sym_ortho(double a, double b, double& c, double& s, double& r) {
  if (b == 0) {
    c = sgn0(a);
    s = 0;
    r = fabs(a);
  } else if (a == 0) {
    c = 0;
    s = sgn0(b);
    r = fabs(b);
  } else if (fabs(b) > fabs(a)) {
    const double tau = a / b;
    s = sgn0(b) / sqrt(1 + tau * tau);
    c = s * tau;
    r = b / s;
  } else {
    const double tau = b / a;
    c = sgn0(a) / sqrt(1 + tau * tau);
    s = c * tau;
    r = a / c;
  }
}

// The state before the first iteration (lsmr.py:205-239) from alpha = |A^T b| / |b| and beta = |b|.  True when
// normar == 0 (or normb == 0): the answer is x = 0 (lsmr.py:247-256, istop 8 here) and nothing more runs.
LSMR_HD bool lsmr_start(double* S, double alpha, double beta, double damp) {
  for (int i = 0; i < LSMR_NS; ++i) S[i] = 0.0;
  S[S_ZETABAR] = alpha * beta;
  S[S_ALPHABAR] = alpha;
  sym_ortho(alpha, damp, S[S_CHAT], S[S_SHAT], S[S_ALPHAHAT]);
  S[S_RHO] = 1;
  S[S_RHOBAR] = 1;
  S[S_CBAR] = 1;
  S[S_SBAR] = 0;
  S[S_BETADD] = beta;
  S[S_RHODOLD] = 1;
  S[S_NORMA2] = alpha * alpha;
  S[S_MINRBAR] = 1e+100;
  S[S_ITN] = 0;
  return !(alpha * beta != 0);
}

// One iteration's recurrences (lsmr.py:301-390) from its alpha and beta.  The caller's vectors follow with
// hbar = hbar * chb + h;  x = x + cx * hbar;  h = h * ch + v  (lsmr.py:342-348).
LSMR_HD void lsmr_recurrence(double* S, double alpha, double beta, double damp, double& chb, double& cx, double& ch) {
  // (lsmr.py:305's rotation of alphabar and damp was computed with the previous iteration's recurrences, off
  // the chain that waits on this iteration's norms)
  const double chat = S[S_CHAT], shat = S[S_SHAT], alphahat = S[S_ALPHAHAT];
  const double rhoold = S[S_RHO];
  double c, s, rho;
  sym_ortho(alphahat, beta, c, s, rho);
  const double thetanew = s * alpha;
  S[S_ALPHABAR] = c * alpha;
  sym_ortho(S[S_ALPHABAR], damp, S[S_CHAT], S[S_SHAT], S[S_ALPHAHAT]);
  const double rhobarold = S[S_RHOBAR];
  const double zetaold = S[S_ZETA];
  const double thetabar = S[S_SBAR] * rho;
  const double rhotemp = S[S_CBAR] * rho;
  double cbar, sbar, rhobar;
  sym_ortho(S[S_CBAR] * rho, thetanew, cbar, sbar, rhobar);
  const double zeta = cbar * S[S_ZETABAR];
  const double zetabar = -sbar * S[S_ZETABAR];
  chb = -(thetabar * rho / (rhoold * rhobarold));
  cx = zeta / (rho * rhobar);
  ch = -(thetanew / rho);
  const double betaacute = chat * S[S_BETADD];
  const double betacheck = -shat * S[S_BETADD];
  const double betahat = c * betaacute;
  const double betadd = -s * betaacute;
  const double thetatildeold = S[S_THETATILDE];
  double ctildeold, stildeold, rhotildeold;
  sym_ortho(S[S_RHODOLD], thetabar, ctildeold, stildeold, rhotildeold);
  const double thetatilde = stildeold * rhobar;
  const double rhodold = ctildeold * rhobar;
  const double betad = -stildeold * S[S_BETAD] + ctildeold * betahat;
  const double tautildeold = (zetaold - thetatildeold * S[S_TAUTILDEOLD]) / rhotildeold;
  const double taud = (zeta - thetatilde * tautildeold) / rhodold;
  const double d = S[S_D] + betacheck * betacheck;
  const double bt = betad - taud;
  const double normr = sqrt(d + bt * bt + betadd * betadd);
  double normA2 = S[S_NORMA2] + beta * beta;
  const double normA = sqrt(normA2);
  normA2 = normA2 + alpha * alpha;
  const double itn = S[S_ITN] + 1;
  const double maxrbar = fmax(S[S_MAXRBAR], rhobarold);
  const double minrbar = itn > 1 ? fmin(S[S_MINRBAR], rhobarold) : S[S_MINRBAR];
  const double condA = fmax(maxrbar, rhotemp) / fmin(minrbar, rhotemp);
  S[S_RHO] = rho;
  S[S_RHOBAR] = rhobar;
  S[S_CBAR] = cbar;
  S[S_SBAR] = sbar;
  S[S_ZETABAR] = zetabar;
  S[S_ZETA] = zeta;
  S[S_BETADD] = betadd;
  S[S_BETAD] = betad;
  S[S_RHODOLD] = rhodold;
  S[S_TAUTILDEOLD] = tautildeold;
  S[S_THETATILDE] = thetatilde;
  S[S_D] = d;
  S[S_NORMA2] = normA2;
  S[S_MAXRBAR] = maxrbar;
  S[S_MINRBAR] = minrbar;
  S[S_ITN] = itn;
  S[S_NORMR] = normr;
  S[S_NORMAR] = fabs(zetabar);
  S[S_NORMA] = normA;
  S[S_CONDA] = condA;
}

// the stop test of lsmr.py:413-441 from a state slot and ||x||; 0 = go on
LSMR_HD int lsmr_istop(const double* S, double normx, double normb, double maxiter, double atol, double btol,
                       double ctol) {
  const double normr = S[S_NORMR], normar = S[S_NORMAR], normA = S[S_NORMA], condA = S[S_CONDA];
  const double itn = S[S_ITN];
  const double test1 = normr / normb;
  const double test2 = (normA * normr) != 0 ? normar / (normA * normr) : INFINITY;
  const double test3 = 1 / condA;
  const double t1 = test1 / (1 + normA * normx / normb);
  const double rtol = btol + atol * normA * normx / normb;
  int istop = 0;
  if (itn >= maxiter) istop = 7;
  if (1 + test3 <= 1) istop = 6;
  if (1 + test2 <= 1) istop = 5;
  if (1 + t1 <= 1) istop = 4;
  if (test3 <= ctol) istop = 3;
  if (test2 <= atol) istop = 2;
  if (test1 <= rtol) istop = 1;
  return istop;
}

#ifdef __HIPCC__
constexpr int LSMR_THREADS = 256;  // the workgroup of every kernel that reduces with the functions below
static_assert(LSMR_THREADS == 4 * 64, "block_sum_all adds four wave sums");

// Sum over the workgroup; every thread returns the same bits (xor butterflies add the same two values,
// commuted, and the wave sums combine in one fixed order).  Ends on a barrier.
__device__ __forceinline__ double block_sum_all(double v, double* red) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return s;
}

__device__ __forceinline__ double block_max_all(double v, double* red) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  return s;
}

// sum_i p[i * stride] over i < count, the same value in every thread of every workgroup that asks
__device__ __forceinline__ double reduce_parts(const double* __restrict__ p, int count, int stride, double* red) {
  double v = 0.0;
  for (int i = threadIdx.x; i < count; i += LSMR_THREADS) v += p[(size_t)i * stride];
  return block_sum_all(v, red);
}
#endif  // __HIPCC__

}  // namespace mq

#undef LSMR_HD
