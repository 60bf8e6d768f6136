// optim_points_possible: refine 3D points over candidate 2D peaks (aniposelib cameras.py:1417-1513 with
// _error_fun_triangulation_possible :1622-1667, _initialize_params_triangulation_possible :1699-1712 and
// _jac_sparsity_triangulation_possible :1795-1847).
//
// The reference hands scipy.optimize.least_squares(method='trf', jac_sparsity=..., loss='linear', ftol=1e-3) the
// optim_points residuals on a SOFT 2D point per (camera, frame, joint) cell -- the softmax (beta = 5) of one
// variable ("alpha") per candidate weighs the cell's candidates -- plus one row 10 (1 - std(softmax)) per cell that
// keeps the weights decided.  The algorithm is the one csrc/optim_trf.hip restates for optim_points (scipy 1.15.3
// trf_no_bounds + lsmr; oracle/trf.py is the numpy restatement): damped lsmr Gauss-Newton step, 2-D subspace trust
// region, update_tr_radius, check_termination.  The Jacobian is analytic (tests/possible_ref.py states it in numpy).
//
// Work decomposition (optim_trf.hip's; one animal = one independent problem, B animals in every launch):
//   * a workgroup owns a block of POSS_FB consecutive frames of one animal (grid NB x B): its reprojection, std,
//     smoothness and limb-length rows and its parameters -- 3 J per frame and every alpha of its cells (an alpha
//     and a std row belong to one frame).  The length variables belong to block 0;
//   * lsmr is two launches per iteration.  poss_lsmr_u_kernel: the previous iteration's recurrences and x / h /
//     hbar updates for the block's parameters, then u = J v - alpha u for its rows; poss_lsmr_v_kernel: the previous
//     iteration's stop test, then v = J^T u - beta v for its parameters.  Every workgroup reduces the norms it
//     needs from the previous launch's per-block partials itself, in one fixed order, so all hold the same scalars
//     bit for bit; no floating-point atomic.  Vectors are kept raw and scaled by 1 / norm where they are read
//     (scipy's in-place scaling: the same products), so no launch waits on another workgroup;
//   * the vectors a launch reads more than once are staged in LDS: the n-space entries of the block's frames, the
//     next n_deriv frames, the lengths and the block's alphas for J v; the m rows of the block's frames and the
//     n_deriv frames before for J^T u.  Jacobian entries are read once per launch, straight from global memory;
//   * the host launches lsmr iterations in chunks and reads the per-animal done flags between chunks; the
//     trust-region logic (2x2 subproblem, radius, termination) runs on the host from the per-block partials, which
//     it adds in block order.
// The block shape depends on F, J, C, P and the constraint count only, so a result depends, bit for bit, only on
// the problem: not on the animals sharing the call, not on the device.
//
// Layouts inside the workspace, frame-major so that a block's share of every vector is contiguous:
//   cell = (f C + c) J + j;  parameters [p3d (F J 3), lengths (NL), alphas (cell, slot)];  a NaN candidate's alpha
//   has an all-zero Jacobian column, stays 0 and takes part in no norm (the reference leaves it out: the same problem);
//   rows [2 cell + comp] reprojection, [MS0 + cell] std, [MSM0 + f 3J + q] smoothness, [ML0 + f NL + l] lengths;
//   rows the reference leaves out (cells without a finite candidate) are 0.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "camera.hpp"
#include "common.hpp"
#include "optim_dev.hpp"
#include "trf_host.hpp"
#include "workspace.hpp"

extern "C" int mq_trust_region_2d(const double* B, const double* g, double Delta, double* p);

namespace mq {
namespace {

#define POSS_THREADS 256
constexpr int PT = POSS_THREADS;
static_assert(PT == 256, "poss_sum adds four wave sums");
constexpr int POSS_FB = 4;  // frames per workgroup (fewer when the staged vectors would not fit in LDS)
constexpr int POSS_MAXP = 4, POSS_MAXL = 64;
constexpr int POSS_NPF = 16;  // doubles per block of partials
constexpr int POSS_NS = 20;   // lsmr state doubles
constexpr double POSS_BETA = 5.0;  // cameras.py:1470
constexpr size_t POSS_LDS_MAX = 64 * 1024;

// per-block partials
enum { PF_COST, PF_ROWS, PF_NGOOD, PF_GG, PF_GMAX, PF_PP, PF_B00, PF_B01, PF_B11, PF_GD, PF_WW, PF_GS0, PF_GS1, PF_STEP };
// lsmr state
enum { S_ALPHABAR, S_RHO, S_RHOBAR, S_CBAR, S_SBAR, S_ZETABAR, S_ZETA, S_BETADD, S_BETAD, S_RHODOLD, S_TAUTILDEOLD,
       S_THETATILDE, S_D, S_NORMA2, S_MAXRBAR, S_MINRBAR, S_NORMR, S_NORMAR, S_NORMA, S_CONDA };
static_assert(S_CONDA < POSS_NS, "lsmr state slot");

struct PossDims {
  int B, C, F, J, P, NL, nS, n, loss;
  int CJ, NC, NX, NA, NV, M, MS0, MSM0, ML0, FB, NB;
  double rp, s_len, s_len_weak;
  double c0, c1, c2, c3;  // np.diff coefficients (named: a runtime index into by-value arguments goes to scratch)
  double atol, btol, ctol;
};

struct PossBufs {
  const double* cams;
  const double* p2d;
  const int* cons;
  const double* ssf;
  const int* act;     // [B] the animal takes part in this launch
  const double* ctl;  // [B][4]: damp, lsmr maxiter, p0, p1
  int* done;          // [B] lsmr finished (its istop)
  double* itn;        // [B] lsmr's iteration count
  double *x, *xt, *g, *vraw, *vn, *h, *hbar, *xl, *s1, *s2;  // [B][NV]
  double *f, *u, *js1, *js2;                                 // [B][M]
  double *Jx, *Ja, *lenJ;                                    // [B][NC][6], [B][NC][3 P], [B][F][NL][4]
  double* part;                                              // [B][NB][POSS_NPF]
  double *upart, *vpart, *xpart;                             // [2][B][NB]
  double* Lpart;                                             // [B][NB][NL]
  double* st;                                                // [2][B][POSS_NS]
};

// Sum / max over the workgroup, the same bits in every thread (xor butterflies add the same two values, commuted;
// the wave sums combine in one fixed order).  Both end on a barrier.
__device__ __forceinline__ double poss_wave_sum(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double poss_sum(double v, double* red) {
  v = poss_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return v;
}
__device__ __forceinline__ double poss_max(double v, double* red) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  return v;
}
// sum over the animal's blocks of p[i * stride], the same value in every thread of every workgroup that asks
__device__ __forceinline__ double poss_reduce_parts(const double* __restrict__ p, int count, int stride, double* red) {
  double v = 0.0;
  for (int i = threadIdx.x; i < count; i += PT) v += p[(size_t)i * stride];
  return poss_sum(v, red);
}

__device__ __forceinline__ double poss_dcoef(const PossDims& D, int m) {
  return m == 0 ? D.c0 : (m == 1 ? D.c1 : (m == 2 ? D.c2 : D.c3));
}

// numpy's population std of the P values a[0..P) (np.std: mean = sum / P, then sqrt(sum((a - mean)^2) / P))
__device__ __forceinline__ double poss_std(const double* a, int P) {
  double s = 0.0;
#pragma unroll
  for (int p = 0; p < POSS_MAXP; ++p)
    if (p < P) s += a[p];
  const double mean = s / P;
  double q = 0.0;
#pragma unroll
  for (int p = 0; p < POSS_MAXP; ++p)
    if (p < P) q += (a[p] - mean) * (a[p] - mean);
  return sqrt(q / P);
}

// The cell's softmax weights (0 at NaN candidates) and its count of finite candidates.  A candidate is bad when
// either coordinate is NaN (the reference looks at the first; its inputs carry NaN in both).
__device__ __forceinline__ int poss_softmax(const double* __restrict__ pp, const double* __restrict__ al, int P,
                                            double* a, double* cu, double* cv) {
  double e[POSS_MAXP], sum = 0.0;
  int ng = 0;
#pragma unroll
  for (int p = 0; p < POSS_MAXP; ++p) {
    e[p] = 0.0;
    cu[p] = cv[p] = 0.0;
    if (p < P) {
      const double u = pp[2 * p], v = pp[2 * p + 1];
      if (!(isnan(u) || isnan(v))) {
        e[p] = exp(POSS_BETA * al[p]);
        cu[p] = u;
        cv[p] = v;
        ++ng;
      }
      sum += e[p];
    }
  }
  if (ng == 0) sum = 1.0;
#pragma unroll
  for (int p = 0; p < POSS_MAXP; ++p) a[p] = e[p] / sum;
  return ng;
}

// the caller's candidates of a frame-major cell: p2d is (B, C, F, J, P, 2)
__device__ __forceinline__ const double* poss_cand(const PossDims& D, const PossBufs& Bf, int b, int cell, int& c,
                                                   int& fj) {
  const int f = cell / D.CJ, r = cell - f * D.CJ;
  c = r / D.J;
  const int j = r - c * D.J;
  fj = f * D.J + j;
  return Bf.p2d + ((((size_t)b * D.C + c) * D.F + f) * D.J + j) * D.P * 2;
}

// A vector's entries as a block sees them: either the global vector (offsets 0) or its LDS copy, which holds the
// p3d entries from xo on, the lengths, and the alphas from ao on.
struct PossVec {
  const double *X, *L, *A;
  int xo, ao;
};
// The m rows as a block sees them: global (offsets 0) or the LDS copy of the rows from cell co / smoothness row so /
// length row lo on.
struct PossRows {
  const double *rep, *sd, *sm, *len;
  int co, so, lo;
};

// out = (uold * us) * ua + J w for the rows of frames [f0, f1) (uold null: J w alone; out may be uold).  Returns the
// thread's share of sum out^2; with out2 / w2 also J w2 -> out2 and the shares of out . out2 and out2 . out2.
__device__ double poss_jv(const PossDims& D, const PossBufs& Bf, int b, int f0, int f1, const PossVec& w, double ws,
                          double* out, const double* uold, double us, double ua, const PossVec* w2, double* out2,
                          double* dot12, double* dot22) {
  const int t = threadIdx.x, J = D.J, F = D.F, P = D.P, J3 = 3 * J, NL = D.NL, n = D.n;
  const double* Jx = Bf.Jx + (size_t)b * D.NC * 6;
  const double* Ja = Bf.Ja + (size_t)b * D.NC * 3 * P;
  const double* lenJ = Bf.lenJ + (size_t)b * F * NL * 4;
  const double ssf = Bf.ssf[b];
  double sq = 0.0, d12 = 0.0, d22 = 0.0;
  for (int pass = 0; pass < (w2 ? 2 : 1); ++pass) {
    const PossVec& v = pass ? *w2 : w;
    double* o = pass ? out2 : out;
    for (int cell = f0 * D.CJ + t; cell < f1 * D.CJ; cell += PT) {
      const int f = cell / D.CJ, r = cell - f * D.CJ, c = r / J, j = r - c * J, fj = f * J + j;
      (void)c;
      const double* jx = Jx + (size_t)cell * 6;
      const double* ja = Ja + (size_t)cell * 3 * P;
      const double w0 = v.X[3 * fj - v.xo] * ws, w1 = v.X[3 * fj + 1 - v.xo] * ws, w2_ = v.X[3 * fj + 2 - v.xo] * ws;
      double r0 = jx[0] * w0 + jx[1] * w1 + jx[2] * w2_;
      double r1 = jx[3] * w0 + jx[4] * w1 + jx[5] * w2_;
      double r2 = 0.0;
      for (int k = 0; k < P; ++k) {
        const double wk = v.A[cell * P + k - v.ao] * ws;
        r0 += ja[k] * wk;
        r1 += ja[P + k] * wk;
        r2 += ja[2 * P + k] * wk;
      }
      if (uold) {
        r0 += (uold[2 * cell] * us) * ua;
        r1 += (uold[2 * cell + 1] * us) * ua;
        r2 += (uold[D.MS0 + cell] * us) * ua;
      }
      if (pass) d12 += out[2 * cell] * r0 + out[2 * cell + 1] * r1 + out[D.MS0 + cell] * r2;  // (this thread's rows)
      o[2 * cell] = r0;
      o[2 * cell + 1] = r1;
      o[D.MS0 + cell] = r2;
      (pass ? d22 : sq) += r0 * r0 + r1 * r1 + r2 * r2;
    }
    const int fs1 = min(f1, F - n);
    for (int i = f0 * J3 + t; i < fs1 * J3; i += PT) {
      double acc = 0.0;
      for (int m = 0; m <= n; ++m) acc += poss_dcoef(D, m) * (v.X[i + m * J3 - v.xo] * ws);
      double r = ssf * acc;
      if (uold) r += (uold[D.MSM0 + i] * us) * ua;
      if (pass) d12 += out[D.MSM0 + i] * r;
      o[D.MSM0 + i] = r;
      (pass ? d22 : sq) += r * r;
    }
    for (int i = f0 * NL + t; i < f1 * NL; i += PT) {
      const int f = i / NL, l = i - f * NL;
      const int ja_ = Bf.cons[2 * l], jb_ = Bf.cons[2 * l + 1];
      const double* lo = lenJ + (size_t)i * 4;
      const double* wa_ = v.X + (f * J3 + 3 * ja_ - v.xo);
      const double* wb_ = v.X + (f * J3 + 3 * jb_ - v.xo);
      double r = lo[0] * (wa_[0] * ws - wb_[0] * ws) + lo[1] * (wa_[1] * ws - wb_[1] * ws) +
                 lo[2] * (wa_[2] * ws - wb_[2] * ws) + lo[3] * (v.L[l] * ws);
      if (uold) r += (uold[D.ML0 + i] * us) * ua;
      if (pass) d12 += out[D.ML0 + i] * r;
      o[D.ML0 + i] = r;
      (pass ? d22 : sq) += r * r;
    }
  }
  if (dot12) *dot12 = d12;
  if (dot22) *dot22 = d22;
  return sq;
}

// out = vold * vb + J^T (u * us) for the parameters of frames [f0, f1) (vold null: J^T alone).  The length variables
// (block 0 only, lsum != null): the sum over the blocks, in block order, of lpart[blk][l] -- each the block's sum
// over its frames of dL * u_len -- times us.  Returns the thread's share of sum out^2; vmax: of max |out|.
__device__ double poss_jt(const PossDims& D, const PossBufs& Bf, int b, int f0, int f1, const PossRows& u, double us,
                          double* out, const double* vold, double vb, double& vmax, const double* lpart) {
  const int t = threadIdx.x, J = D.J, F = D.F, C = D.C, P = D.P, J3 = 3 * J, NL = D.NL, n = D.n;
  const double* Jx = Bf.Jx + (size_t)b * D.NC * 6;
  const double* Ja = Bf.Ja + (size_t)b * D.NC * 3 * P;
  const double* lenJ = Bf.lenJ + (size_t)b * F * NL * 4;
  const double ssf = Bf.ssf[b];
  double sq = 0.0;
  // the 3D points: the cameras in order, the smoothness rows holding the frame, the constraints in order
  for (int i = f0 * J3 + t; i < f1 * J3; i += PT) {
    const int fj = i / 3, k = i - 3 * fj, f = fj / J, j = fj - f * J, q = 3 * j + k;
    double acc = 0.0;
    for (int c = 0; c < C; ++c) {
      const int cell = (f * C + c) * J + j;
      const double* jx = Jx + (size_t)cell * 6;
      acc += jx[k] * (u.rep[2 * (cell - u.co)] * us) + jx[3 + k] * (u.rep[2 * (cell - u.co) + 1] * us);
    }
    for (int m = 0; m <= n; ++m) {
      const int r = f - m;
      if (r >= 0 && r < F - n) acc += ssf * poss_dcoef(D, m) * (u.sm[r * J3 + q - u.so] * us);
    }
    for (int l = 0; l < NL; ++l) {
      const int ja_ = Bf.cons[2 * l], jb_ = Bf.cons[2 * l + 1];
      if (ja_ != j && jb_ != j) continue;
      const double term = lenJ[((size_t)f * NL + l) * 4 + k] * (u.len[f * NL + l - u.lo] * us);
      if (ja_ == j) acc += term;
      else acc -= term;
    }
    const double v = vold ? vold[i] * vb + acc : acc;
    out[i] = v;
    sq += v * v;
    vmax = fmax(vmax, fabs(v));
  }
  // the alphas: the cell's two reprojection rows and its std row
  for (int i = f0 * D.CJ * P + t; i < f1 * D.CJ * P; i += PT) {
    const int cell = i / P, k = i - cell * P;
    const double* ja = Ja + (size_t)cell * 3 * P;
    const double acc = ja[k] * (u.rep[2 * (cell - u.co)] * us) + ja[P + k] * (u.rep[2 * (cell - u.co) + 1] * us) +
                       ja[2 * P + k] * (u.sd[cell - u.co] * us);
    const size_t o = (size_t)D.NX + NL + i;
    const double v = vold ? vold[o] * vb + acc : acc;
    out[o] = v;
    sq += v * v;
    vmax = fmax(vmax, fabs(v));
  }
  if (lpart) {
    for (int l = t; l < NL; l += PT) {
      double acc = 0.0;
      for (int bb = 0; bb < D.NB; ++bb) acc += lpart[(size_t)bb * NL + l];
      acc *= us;
      const size_t o = (size_t)D.NX + l;
      const double v = vold ? vold[o] * vb + acc : acc;
      out[o] = v;
      sq += v * v;
      vmax = fmax(vmax, fabs(v));
    }
  }
  return sq;
}

// the block's sums over its frames of dL * u_len (raw u) -> lp[l]
__device__ __forceinline__ void poss_len_partials(const PossDims& D, const PossBufs& Bf, int b, int f0, int f1,
                                                  const double* __restrict__ ulen, double* lp) {
  const double* lenJ = Bf.lenJ + (size_t)b * D.F * D.NL * 4;
  for (int l = threadIdx.x; l < D.NL; l += PT) {
    double acc = 0.0;
    for (int f = f0; f < f1; ++f) acc += lenJ[((size_t)f * D.NL + l) * 4 + 3] * ulen[f * D.NL + l];
    lp[l] = acc;
  }
}

// scipy.sparse.linalg._isolve.lsqr._sym_ortho (np.sign(0) = 0)
__device__ __forceinline__ double poss_sgn0(double a) { return a > 0 ? 1.0 : (a < 0 ? -1.0 : 0.0); }
__device__ __forceinline__ void poss_sym_ortho(double a, double b, double& c, double& s, double& r) {
  if (b == 0) {
    c = poss_sgn0(a);
    s = 0;
    r = fabs(a);
  } else if (a == 0) {
    c = 0;
    s = poss_sgn0(b);
    r = fabs(b);
  } else if (fabs(b) > fabs(a)) {
    const double tau = a / b;
    s = poss_sgn0(b) / sqrt(1 + tau * tau);
    c = s * tau;
    r = b / s;
  } else {
    const double tau = b / a;
    c = poss_sgn0(a) / sqrt(1 + tau * tau);
    s = c * tau;
    r = a / c;
  }
}

#define POSS_BLOCK()                                                   \
  const int blk = blockIdx.x, b = blockIdx.y, t = threadIdx.x;         \
  const int f0 = blk * D.FB, f1 = min(D.F, f0 + D.FB);                 \
  (void)t;                                                             \
  (void)f1

__device__ __forceinline__ PossVec poss_global_vec(const PossDims& D, const double* p) {
  return PossVec{p, p + D.NX, p + D.NX + D.NL, 0, 0};
}
__device__ __forceinline__ PossRows poss_global_rows(const PossDims& D, const double* u) {
  return PossRows{u, u + D.MS0, u + D.MSM0, u + D.ML0, 0, 0, 0};
}

// ---------------------------------------------------------------------------------------------------------
// The caller's [p3d, lengths] into the workspace layout, alphas = 0 (:1699-1712).
__global__ void __launch_bounds__(POSS_THREADS) poss_init_kernel(PossDims D, PossBufs Bf, const double* __restrict__ xin) {
  POSS_BLOCK();
  double* x = Bf.x + (size_t)b * D.NV;
  const int n0 = D.NX + D.NL, J3 = 3 * D.J;
  for (int i = f0 * J3 + t; i < f1 * J3; i += PT) x[i] = xin[(size_t)b * n0 + i];
  for (int i = f0 * D.CJ * D.P + t; i < f1 * D.CJ * D.P; i += PT) x[n0 + i] = 0.0;
  if (blk == 0)
    for (int l = t; l < D.NL; l += PT) x[D.NX + l] = xin[(size_t)b * n0 + D.NX + l];
}

// The trial point xt = x + p0 s1 + p1 s2 for the block's parameters; partial |step|^2.
__global__ void __launch_bounds__(POSS_THREADS) poss_step_kernel(PossDims D, PossBufs Bf) {
  POSS_BLOCK();
  if (!Bf.act[b]) return;
  __shared__ double red[4];
  const size_t nb = (size_t)b * D.NV;
  const double p0 = Bf.ctl[4 * b + 2], p1 = Bf.ctl[4 * b + 3];
  const int J3 = 3 * D.J, n0 = D.NX + D.NL;
  double st = 0.0;
  auto one = [&](size_t i) {
    const double step = Bf.s1[nb + i] * p0 + Bf.s2[nb + i] * p1;
    Bf.xt[nb + i] = Bf.x[nb + i] + step;
    st += step * step;
  };
  for (int i = f0 * J3 + t; i < f1 * J3; i += PT) one(i);
  for (int i = f0 * D.CJ * D.P + t; i < f1 * D.CJ * D.P; i += PT) one((size_t)n0 + i);
  if (blk == 0)
    for (int l = t; l < D.NL; l += PT) one((size_t)D.NX + l);
  st = poss_sum(st, red);
  if (t == 0) Bf.part[((size_t)b * D.NB + blk) * POSS_NPF + PF_STEP] = st;
}

// Residuals and Jacobian entries of the block's rows at x (src 0) or xt (src 1); partial cost, rows, finite
// candidates and |point|^2, and the block's sums of dL * r_len (for g's length entries).
__global__ void __launch_bounds__(POSS_THREADS) poss_eval_kernel(PossDims D, PossBufs Bf, int src) {
  POSS_BLOCK();
  if (!Bf.act[b]) return;
  __shared__ double red[4];
  const int J = D.J, F = D.F, P = D.P, J3 = 3 * J, NL = D.NL, n = D.n;
  const double* p = (src ? Bf.xt : Bf.x) + (size_t)b * D.NV;
  const double* L = p + D.NX;
  const double* al = p + D.NX + NL;
  double* fo = Bf.f + (size_t)b * D.M;
  double* Jx = Bf.Jx + (size_t)b * D.NC * 6;
  double* Ja = Bf.Ja + (size_t)b * D.NC * 3 * P;
  double* lenJ = Bf.lenJ + (size_t)b * F * NL * 4;
  const double ssf = Bf.ssf[b];
  double cost = 0.0, rows = 0.0, ngood = 0.0, pp = 0.0;
  for (int cell = f0 * D.CJ + t; cell < f1 * D.CJ; cell += PT) {
    int c, fj;
    const double* cand = poss_cand(D, Bf, b, cell, c, fj);
    double a[POSS_MAXP], cu[POSS_MAXP], cv[POSS_MAXP];
    const int ng = poss_softmax(cand, al + (size_t)cell * P, P, a, cu, cv);
    double res[3] = {0.0, 0.0, 0.0}, jx[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ja[3 * POSS_MAXP];
#pragma unroll
    for (int k = 0; k < 3 * POSS_MAXP; ++k) ja[k] = 0.0;
    if (ng > 0) {
      double su = 0.0, sv = 0.0;  // the soft 2D point (:1658)
#pragma unroll
      for (int q = 0; q < POSS_MAXP; ++q) {
        su += a[q] * cu[q];
        sv += a[q] * cv[q];
      }
      const double X[3] = {p[3 * fj], p[3 * fj + 1], p[3 * fj + 2]};
      double pu, pv, Ju[3], Jv[3];
      project_jac(cam_at(Bf.cams, c), X, pu, pv, Ju, Jv);
      double ru, dru, rv, drv;
      reproj_loss(su - pu, D.rp, D.loss, ru, dru);
      reproj_loss(sv - pv, D.rp, D.loss, rv, drv);
      res[0] = ru;
      res[1] = rv;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        jx[k] = -dru * Ju[k];
        jx[3 + k] = -drv * Jv[k];
      }
      // d soft / d alpha_k = beta a_k (cand_k - soft)
#pragma unroll
      for (int k = 0; k < POSS_MAXP; ++k) {
        ja[k] = dru * (POSS_BETA * a[k] * (cu[k] - su));
        ja[POSS_MAXP + k] = drv * (POSS_BETA * a[k] * (cv[k] - sv));
      }
      // the std row (:1664-1665) over all P slots, NaN candidates counting as 0
      const double sd = poss_std(a, P);
      res[2] = (1 - sd) * 10;
      double amin = a[0], amax = a[0];
#pragma unroll
      for (int q = 1; q < POSS_MAXP; ++q)
        if (q < P) {
          amin = fmin(amin, a[q]);
          amax = fmax(amax, a[q]);
        }
      if (amin == amax) {
        // every weight equal (x0 with all slots finite): std is not differentiable; the right-hand derivative
        // along alpha_k is std_P(d a / d alpha_k), what forward differences see
#pragma unroll
        for (int k = 0; k < POSS_MAXP; ++k) {
          double dv[POSS_MAXP];
#pragma unroll
          for (int i = 0; i < POSS_MAXP; ++i) dv[i] = POSS_BETA * a[k] * ((i == k ? 1.0 : 0.0) - a[i]);
          const double ds = poss_std(dv, P);
          if (k < P) ja[2 * POSS_MAXP + k] = -10 * ds;
        }
      } else {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < POSS_MAXP; ++q)
          if (q < P) s += a[q];
        const double mean = s / P;
        double T = 0.0;
#pragma unroll
        for (int q = 0; q < POSS_MAXP; ++q)
          if (q < P) T += (a[q] - mean) * a[q];
#pragma unroll
        for (int k = 0; k < POSS_MAXP; ++k)
          if (k < P) ja[2 * POSS_MAXP + k] = -10 * (POSS_BETA * a[k] * ((a[k] - mean) - T) / (P * sd));
      }
      cost += ru * ru + rv * rv + res[2] * res[2];
      rows += 3.0;
      ngood += ng;
    }
    fo[2 * cell] = res[0];
    fo[2 * cell + 1] = res[1];
    fo[D.MS0 + cell] = res[2];
#pragma unroll
    for (int k = 0; k < 6; ++k) Jx[(size_t)cell * 6 + k] = jx[k];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < POSS_MAXP; ++k)
        if (k < P) {
          Ja[((size_t)cell * 3 + r) * P + k] = ja[r * POSS_MAXP + k];
          if (r == 0) {
            const double av = al[(size_t)cell * P + k];
            pp += av * av;
          }
        }
  }
  // smoothness: np.diff(p3ds, n, axis=0) * scale_smooth (:1602), numpy's order of the differences
  for (int i = f0 * J3 + t; i < min(f1, F - n) * J3; i += PT) {
    const double x0 = p[i], x1 = p[i + J3];
    double dd = x1 - x0;
    if (n >= 2) {
      const double x2 = p[i + 2 * J3];
      const double e1 = x2 - x1;
      if (n == 2) {
        dd = e1 - dd;
      } else {
        const double x3 = p[i + 3 * J3];
        dd = ((x3 - x2) - e1) - (e1 - dd);
      }
    }
    const double val = dd * ssf;
    cost += val * val;
    rows += 1.0;
    fo[D.MSM0 + i] = val;
  }
  for (int i = f0 * J3 + t; i < f1 * J3; i += PT) pp += p[i] * p[i];
  if (blk == 0)
    for (int l = t; l < NL; l += PT) pp += L[l] * L[l];
  // limb lengths (:1604-1617): 100 (|Xa - Xb| - L) / L * scale
  for (int i = f0 * NL + t; i < f1 * NL; i += PT) {
    const int f = i / NL, l = i - f * NL;
    const int ja_ = Bf.cons[2 * l], jb_ = Bf.cons[2 * l + 1];
    const double Lv = L[l], s = l < D.nS ? D.s_len : D.s_len_weak;
    const double* Xa = p + (size_t)f * J3 + 3 * ja_;
    const double* Xb = p + (size_t)f * J3 + 3 * jb_;
    const double dx = Xa[0] - Xb[0], dy = Xa[1] - Xb[1], dz = Xa[2] - Xb[2];
    const double nr = sqrt(dx * dx + dy * dy + dz * dz);
    const double val = 100 * (nr - Lv) / Lv * s;
    cost += val * val;
    rows += 1.0;
    fo[D.ML0 + i] = val;
    const double k = nr > 0 ? s * 100 / Lv / nr : 0.0;
    double* lo = lenJ + (size_t)i * 4;
    lo[0] = k * dx;
    lo[1] = k * dy;
    lo[2] = k * dz;
    lo[3] = -s * 100 * nr / (Lv * Lv);
  }
  cost = poss_sum(cost, red);  // (the barrier: the length rows and their Jacobian entries are read below)
  rows = poss_sum(rows, red);
  ngood = poss_sum(ngood, red);
  pp = poss_sum(pp, red);
  poss_len_partials(D, Bf, b, f0, f1, fo + D.ML0, Bf.Lpart + ((size_t)b * D.NB + blk) * NL);
  if (t == 0) {
    double* pf = Bf.part + ((size_t)b * D.NB + blk) * POSS_NPF;
    pf[PF_COST] = cost;
    pf[PF_ROWS] = rows;
    pf[PF_NGOOD] = ngood;
    pf[PF_PP] = pp;
  }
}

// Dynamic LDS of a launch that stages the m rows of frames [fa, f1) (poss_stage_rows) or the n-space entries of
// frames [f0, fe) with the lengths and the block's alphas (poss_stage_vec).
extern __shared__ double poss_lds[];

__device__ __forceinline__ PossRows poss_stage_rows(const PossDims& D, const double* __restrict__ u, int fa, int f1) {
  const int t = threadIdx.x, J3 = 3 * D.J, NL = D.NL;
  const int nc = (f1 - fa) * D.CJ, ns = (f1 - fa) * J3, nl = (f1 - fa) * NL;
  double* rep = poss_lds;
  double* sd = rep + 2 * nc;
  double* sm = sd + nc;
  double* len = sm + ns;
  for (int i = t; i < 2 * nc; i += PT) rep[i] = u[2 * fa * D.CJ + i];
  for (int i = t; i < nc; i += PT) sd[i] = u[D.MS0 + fa * D.CJ + i];
  const int smax = (D.F - D.n) * J3;  // (the last n frames have no smoothness rows)
  for (int i = t; i < ns; i += PT) sm[i] = fa * J3 + i < smax ? u[D.MSM0 + fa * J3 + i] : 0.0;
  for (int i = t; i < nl; i += PT) len[i] = u[D.ML0 + fa * NL + i];
  return PossRows{rep, sd, sm, len, fa * D.CJ, fa * J3, fa * NL};
}
__device__ __forceinline__ PossVec poss_stage_vec(const PossDims& D, const double* __restrict__ v, int f0, int f1, int fe) {
  const int t = threadIdx.x, J3 = 3 * D.J, NL = D.NL;
  const int nx = (fe - f0) * J3, na = (f1 - f0) * D.CJ * D.P;
  double* X = poss_lds;
  double* L = X + nx;
  double* A = L + NL;
  for (int i = t; i < nx; i += PT) X[i] = v[f0 * J3 + i];
  for (int i = t; i < NL; i += PT) L[i] = v[D.NX + i];
  for (int i = t; i < na; i += PT) A[i] = v[D.NX + NL + f0 * D.CJ * D.P + i];
  return PossVec{X, L, A, f0 * J3, f0 * D.CJ * D.P};
}
size_t poss_lds_bytes(int FB, int n, int J, int C, int P, int NL) {
  const size_t rows = (size_t)(FB + n) * ((size_t)3 * C * J + 3 * J + NL);
  const size_t vec = (size_t)(FB + n) * 3 * J + NL + (size_t)FB * C * J * P;
  return std::max(rows, vec) * sizeof(double);
}

// v = J^T (u * us) - beta vn for the block's parameters.
//   MODE 0: g = J^T f; partials |g|^2, max |g|
//   MODE 1: lsmr's start, vraw = J^T (f / normb); partial |vraw|^2 in vpart[0]
__global__ void __launch_bounds__(POSS_THREADS) poss_jt_kernel(PossDims D, PossBufs Bf, int mode) {
  POSS_BLOCK();
  if (!Bf.act[b]) return;
  __shared__ double red[4];
  const double* f = Bf.f + (size_t)b * D.M;
  const PossRows u = poss_stage_rows(D, f, max(0, f0 - D.n), f1);
  __syncthreads();
  double us = 1.0;
  if (mode == 1) {
    const double cost = poss_reduce_parts(Bf.part + (size_t)b * D.NB * POSS_NPF + PF_COST, D.NB, POSS_NPF, red);
    us = 1 / sqrt(cost);
  }
  double* out = (mode == 0 ? Bf.g : Bf.vraw) + (size_t)b * D.NV;
  double vmax = 0.0;
  double sq = poss_jt(D, Bf, b, f0, f1, u, us, out, nullptr, 0.0, vmax,
                      blk == 0 ? Bf.Lpart + (size_t)b * D.NB * D.NL : nullptr);
  sq = poss_sum(sq, red);
  vmax = poss_max(vmax, red);
  if (t == 0) {
    if (mode == 0) {
      double* pf = Bf.part + ((size_t)b * D.NB + blk) * POSS_NPF;
      pf[PF_GG] = sq;
      pf[PF_GMAX] = vmax;
    } else {
      Bf.vpart[(size_t)b * D.NB + blk] = sq;
    }
  }
}

// js1 = J w1 (and js2 = J w2) for the block's rows; partials |js1|^2, js1 . js2, |js2|^2.  which 0: w1 = g alone
// (the next iteration's `regularize`, trf.py:480-484); 1: w1 = s1, w2 = s2 (B_S, trf.py:491).
__global__ void __launch_bounds__(POSS_THREADS) poss_jv_kernel(PossDims D, PossBufs Bf, int which) {
  POSS_BLOCK();
  if (!Bf.act[b]) return;
  __shared__ double red[4];
  const size_t nb = (size_t)b * D.NV;
  const PossVec w1 = poss_global_vec(D, (which ? Bf.s1 : Bf.g) + nb);
  const PossVec w2 = poss_global_vec(D, Bf.s2 + nb);
  double d12 = 0.0, d22 = 0.0;
  double sq = poss_jv(D, Bf, b, f0, f1, w1, 1.0, Bf.js1 + (size_t)b * D.M, nullptr, 0.0, 0.0, which ? &w2 : nullptr,
                      Bf.js2 + (size_t)b * D.M, &d12, &d22);
  sq = poss_sum(sq, red);
  d12 = poss_sum(d12, red);
  d22 = poss_sum(d22, red);
  if (t == 0) {
    double* pf = Bf.part + ((size_t)b * D.NB + blk) * POSS_NPF;
    pf[PF_B00] = sq;
    pf[PF_B01] = d12;
    pf[PF_B11] = d22;
  }
}

// ---------------------------------------------------------------------------------------------------------
// lsmr (scipy sparse/linalg/_isolve/lsmr.py:29-460; atol = btol 1e-6, conlim 1e8), iteration k >= 1 in two launches
// (par = k & 1, pp = par ^ 1).
//
// Launch 1: alpha_{k-1} from vpart[pp] and beta_{k-1} from upart[pp] (k = 1: normb); k = 1 starts the recurrences
// (:205-239), k > 1 runs iteration k - 1's (:301-390) with the hbar / x / h updates of the block's parameters;
// then u_k = J v_{k-1} - alpha_{k-1} u_{k-1} for the block's rows (:284-286), partial |u_k|^2, |x_{k-1}|^2 and the
// block's sums of dL * u_len.
__global__ void __launch_bounds__(POSS_THREADS) poss_lsmr_u_kernel(PossDims D, PossBufs Bf, int k) {
  POSS_BLOCK();
  if (!Bf.act[b] || Bf.done[b]) return;
  __shared__ double red[4];
  const int par = k & 1, pp = par ^ 1, NB = D.NB, J3 = 3 * D.J, n0 = D.NX + D.NL;
  const size_t nb = (size_t)b * D.NV, sb = (size_t)b * NB;
  const double damp = Bf.ctl[4 * b];
  const int fe = min(D.F, f1 + D.n);
  const PossVec vs = poss_stage_vec(D, Bf.vraw + nb, f0, f1, fe);  // (the first reduction below is the barrier)
  const double alpha = sqrt(poss_reduce_parts(Bf.vpart + (size_t)pp * D.B * NB + sb, NB, 1, red));
  double beta;
  if (k == 1) beta = sqrt(poss_reduce_parts(Bf.part + sb * POSS_NPF + PF_COST, NB, POSS_NPF, red));
  else beta = sqrt(poss_reduce_parts(Bf.upart + (size_t)pp * D.B * NB + sb, NB, 1, red));
  double S[POSS_NS];
  double chb = 0.0, cx = 0.0, ch = 0.0;
  if (k == 1) {
#pragma unroll
    for (int i = 0; i < POSS_NS; ++i) S[i] = 0.0;
    S[S_ZETABAR] = alpha * beta;
    S[S_ALPHABAR] = alpha;
    S[S_RHO] = 1;
    S[S_RHOBAR] = 1;
    S[S_CBAR] = 1;
    S[S_BETADD] = beta;
    S[S_RHODOLD] = 1;
    S[S_NORMA2] = alpha * alpha;
    S[S_MINRBAR] = 1e+100;
    if (!(alpha * beta != 0)) {  // normar == 0 (or normb == 0): x = 0 (lsmr.py:247-256)
      for (int i = f0 * J3 + t; i < f1 * J3; i += PT) Bf.xl[nb + i] = 0.0;
      for (int i = f0 * D.CJ * D.P + t; i < f1 * D.CJ * D.P; i += PT) Bf.xl[nb + n0 + i] = 0.0;
      if (blk == 0) {
        for (int l = t; l < D.NL; l += PT) Bf.xl[nb + D.NX + l] = 0.0;
        if (t == 0) {
          Bf.done[b] = 8;
          Bf.itn[b] = 0;
        }
      }
      return;
    }
  } else {
    const double* Si = Bf.st + ((size_t)pp * D.B + b) * POSS_NS;
#pragma unroll
    for (int i = 0; i < POSS_NS; ++i) S[i] = Si[i];
    const double itn = k - 1;
    double chat, shat, alphahat;
    poss_sym_ortho(S[S_ALPHABAR], damp, chat, shat, alphahat);
    const double rhoold = S[S_RHO];
    double c, sn, rho;
    poss_sym_ortho(alphahat, beta, c, sn, rho);
    const double thetanew = sn * alpha;
    S[S_ALPHABAR] = c * alpha;
    const double rhobarold = S[S_RHOBAR], zetaold = S[S_ZETA];
    const double thetabar = S[S_SBAR] * rho, rhotemp = S[S_CBAR] * rho;
    double cbar, sbar, rhobar;
    poss_sym_ortho(S[S_CBAR] * rho, thetanew, cbar, sbar, rhobar);
    const double zeta = cbar * S[S_ZETABAR];
    const double zetabar = -sbar * S[S_ZETABAR];
    chb = -(thetabar * rho / (rhoold * rhobarold));
    cx = zeta / (rho * rhobar);
    ch = -(thetanew / rho);
    const double betaacute = chat * S[S_BETADD], betacheck = -shat * S[S_BETADD];
    const double betahat = c * betaacute;
    const double betadd = -sn * betaacute;
    const double thetatildeold = S[S_THETATILDE];
    double ctildeold, stildeold, rhotildeold;
    poss_sym_ortho(S[S_RHODOLD], thetabar, ctildeold, stildeold, rhotildeold);
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
    S[S_NORMR] = normr;
    S[S_NORMAR] = fabs(zetabar);
    S[S_NORMA] = normA;
    S[S_CONDA] = condA;
  }
  if (blk == 0 && t == 0) {
    double* So = Bf.st + ((size_t)par * D.B + b) * POSS_NS;
#pragma unroll
    for (int i = 0; i < POSS_NS; ++i) So[i] = S[i];
  }
  // the block's parameters: v_{k-1} = vraw / alpha (scipy's in-place v *= 1 / alpha), hbar, x, h (:342-348)
  const double ia = 1 / alpha;
  double sx = 0.0;
  auto upd = [&](size_t i) {
    const double vv = Bf.vraw[nb + i] * ia;
    Bf.vn[nb + i] = vv;
    if (k == 1) {
      Bf.h[nb + i] = vv;
      Bf.hbar[nb + i] = 0.0;
      Bf.xl[nb + i] = 0.0;
    } else {
      const double hb = Bf.hbar[nb + i] * chb + Bf.h[nb + i];
      const double xx = Bf.xl[nb + i] + cx * hb;
      const double hh = Bf.h[nb + i] * ch + vv;
      Bf.hbar[nb + i] = hb;
      Bf.xl[nb + i] = xx;
      Bf.h[nb + i] = hh;
      sx += xx * xx;
    }
  };
  for (int i = f0 * J3 + t; i < f1 * J3; i += PT) upd(i);
  for (int i = f0 * D.CJ * D.P + t; i < f1 * D.CJ * D.P; i += PT) upd((size_t)n0 + i);
  if (blk == 0)
    for (int l = t; l < D.NL; l += PT) upd((size_t)D.NX + l);
  // u_k = (u_{k-1} / beta) * -alpha + J v_{k-1}, from the staged raw v
  double* u = Bf.u + (size_t)b * D.M;
  const double* uold = k == 1 ? Bf.f + (size_t)b * D.M : u;
  double su = poss_jv(D, Bf, b, f0, f1, vs, ia, u, uold, 1 / beta, -alpha, nullptr, nullptr, nullptr, nullptr);
  su = poss_sum(su, red);  // (the barrier: the length rows are read below by other threads)
  sx = poss_sum(sx, red);
  poss_len_partials(D, Bf, b, f0, f1, u + D.ML0, Bf.Lpart + (sb + blk) * D.NL);
  if (t == 0) {
    Bf.upart[(size_t)par * D.B * NB + sb + blk] = su;
    Bf.xpart[(size_t)par * D.B * NB + sb + blk] = sx;
  }
}

// Launch 2: beta_k from upart[par]; the stop test of iteration k - 1 (:392-441) with |x_{k-1}| from xpart[par] -- when
// it passes x_{k-1} is the answer and no later launch does anything; then v_k = J^T (u_k / beta_k) - beta_k v_{k-1}
// for the block's parameters (:289-291) and partial |v_k|^2.
__global__ void __launch_bounds__(POSS_THREADS) poss_lsmr_v_kernel(PossDims D, PossBufs Bf, int k) {
  POSS_BLOCK();
  if (!Bf.act[b] || Bf.done[b]) return;
  __shared__ double red[4];
  const int par = k & 1, NB = D.NB;
  const size_t nb = (size_t)b * D.NV, sb = (size_t)b * NB;
  const double maxiter = Bf.ctl[4 * b + 1];
  const PossRows us_rows = poss_stage_rows(D, Bf.u + (size_t)b * D.M, max(0, f0 - D.n), f1);
  const double beta = sqrt(poss_reduce_parts(Bf.upart + (size_t)par * D.B * NB + sb, NB, 1, red));
  if (k > 1) {
    const double normx = sqrt(poss_reduce_parts(Bf.xpart + (size_t)par * D.B * NB + sb, NB, 1, red));
    const double normb = sqrt(poss_reduce_parts(Bf.part + sb * POSS_NPF + PF_COST, NB, POSS_NPF, red));
    const double* S = Bf.st + ((size_t)par * D.B + b) * POSS_NS;
    const double normr = S[S_NORMR], normar = S[S_NORMAR], normA = S[S_NORMA], condA = S[S_CONDA];
    const double itn = k - 1;
    const double test1 = normr / normb;
    const double test2 = (normA * normr) != 0 ? normar / (normA * normr) : INFINITY;
    const double test3 = 1 / condA;
    const double t1 = test1 / (1 + normA * normx / normb);
    const double rtol = D.btol + D.atol * normA * normx / normb;
    int istop = 0;
    if (itn >= maxiter) istop = 7;
    if (1 + test3 <= 1) istop = 6;
    if (1 + test2 <= 1) istop = 5;
    if (1 + t1 <= 1) istop = 4;
    if (test3 <= D.ctol) istop = 3;
    if (test2 <= D.atol) istop = 2;
    if (test1 <= rtol) istop = 1;
    if (istop) {  // (every workgroup of the animal finds the same; block 0 records it for the launches to come)
      if (blk == 0 && t == 0) {
        Bf.done[b] = istop;
        Bf.itn[b] = itn;
      }
      return;
    }
  }
  double dummy = 0.0;
  double sv = poss_jt(D, Bf, b, f0, f1, us_rows, 1 / beta, Bf.vraw + nb, Bf.vn + nb, -beta, dummy,
                      blk == 0 ? Bf.Lpart + sb * D.NL : nullptr);
  sv = poss_sum(sv, red);
  if (t == 0) Bf.vpart[(size_t)par * D.B * NB + sb + blk] = sv;
}

// ---------------------------------------------------------------------------------------------------------
// S = orth([g, gn]) by Gram-Schmidt in three launches (trf.py:489-490; gn = lsmr's x): stage 0 partial g . gn;
// stage 1 s1 = g / |g|, w = gn - (s1 . gn) s1, partial |w|^2 and s1 . g; stage 2 s2 = w / |w|, partial s2 . g.
__global__ void __launch_bounds__(POSS_THREADS) poss_subspace_kernel(PossDims D, PossBufs Bf, int stage) {
  POSS_BLOCK();
  if (!Bf.act[b]) return;
  __shared__ double red[4];
  const size_t nb = (size_t)b * D.NV;
  const int J3 = 3 * D.J, n0 = D.NX + D.NL, NB = D.NB;
  const double* P0 = Bf.part + (size_t)b * NB * POSS_NPF;
  double ng = 0.0, dproj = 0.0, nw = 0.0;
  if (stage >= 1) {
    ng = sqrt(poss_reduce_parts(P0 + PF_GG, NB, POSS_NPF, red));
    const double gd = poss_reduce_parts(P0 + PF_GD, NB, POSS_NPF, red);
    dproj = ng > 0 ? gd / ng : 0.0;
  }
  if (stage == 2) nw = sqrt(poss_reduce_parts(P0 + PF_WW, NB, POSS_NPF, red));
  double a0 = 0.0, a1 = 0.0;
  auto one = [&](size_t i) {
    const double g = Bf.g[nb + i];
    if (stage == 0) {
      a0 += g * Bf.xl[nb + i];
    } else if (stage == 1) {
      const double a = ng > 0 ? g / ng : 0.0;
      const double w = Bf.xl[nb + i] - dproj * a;
      Bf.s1[nb + i] = a;
      Bf.s2[nb + i] = w;
      a0 += w * w;
      a1 += a * g;
    } else {
      const double w = nw > 0 ? Bf.s2[nb + i] / nw : 0.0;
      Bf.s2[nb + i] = w;
      a0 += w * g;
    }
  };
  for (int i = f0 * J3 + t; i < f1 * J3; i += PT) one(i);
  for (int i = f0 * D.CJ * D.P + t; i < f1 * D.CJ * D.P; i += PT) one((size_t)n0 + i);
  if (blk == 0)
    for (int l = t; l < D.NL; l += PT) one((size_t)D.NX + l);
  a0 = poss_sum(a0, red);
  a1 = poss_sum(a1, red);
  if (t == 0) {
    double* pf = Bf.part + ((size_t)b * NB + blk) * POSS_NPF;
    if (stage == 0) pf[PF_GD] = a0;
    if (stage == 1) {
      pf[PF_WW] = a0;
      pf[PF_GS0] = a1;
    }
    if (stage == 2) pf[PF_GS1] = a0;
  }
}

// x = xt for the animals that accepted their step.
__global__ void __launch_bounds__(POSS_THREADS) poss_accept_kernel(PossDims D, PossBufs Bf) {
  POSS_BLOCK();
  if (!Bf.act[b]) return;
  const size_t nb = (size_t)b * D.NV;
  const int J3 = 3 * D.J, n0 = D.NX + D.NL;
  for (int i = f0 * J3 + t; i < f1 * J3; i += PT) Bf.x[nb + i] = Bf.xt[nb + i];
  for (int i = f0 * D.CJ * D.P + t; i < f1 * D.CJ * D.P; i += PT) Bf.x[nb + n0 + i] = Bf.xt[nb + n0 + i];
  if (blk == 0)
    for (int l = t; l < D.NL; l += PT) Bf.x[nb + D.NX + l] = Bf.xt[nb + D.NX + l];
}

// The outputs: [p3d, lengths] back to the caller, alphas_norm (C, F, J, P) with NaN at NaN candidates (:1493-1506).
__global__ void __launch_bounds__(POSS_THREADS) poss_finish_kernel(PossDims D, PossBufs Bf, double* __restrict__ xout,
                                                                   double* __restrict__ anorm) {
  POSS_BLOCK();
  const int P = D.P, J3 = 3 * D.J, n0 = D.NX + D.NL;
  const double* x = Bf.x + (size_t)b * D.NV;
  for (int i = f0 * J3 + t; i < f1 * J3; i += PT) xout[(size_t)b * n0 + i] = x[i];
  if (blk == 0)
    for (int l = t; l < D.NL; l += PT) xout[(size_t)b * n0 + D.NX + l] = x[D.NX + l];
  const double* al = x + n0;
  for (int cell = f0 * D.CJ + t; cell < f1 * D.CJ; cell += PT) {
    int c, fj;
    const double* cand = poss_cand(D, Bf, b, cell, c, fj);
    double a[POSS_MAXP], cu[POSS_MAXP], cv[POSS_MAXP];
    (void)poss_softmax(cand, al + (size_t)cell * P, P, a, cu, cv);
    double* o = anorm + (size_t)(cand - Bf.p2d) / 2;
#pragma unroll
    for (int k = 0; k < POSS_MAXP; ++k)
      if (k < P) o[k] = (isnan(cand[2 * k]) || isnan(cand[2 * k + 1])) ? __builtin_nan("") : a[k];
  }
}

// frames per workgroup: POSS_FB, fewer when the staged vectors of a block would not fit in LDS (F-independent)
int poss_frames_per_block(int J, int C, int P, int NL) {
  for (int fb = POSS_FB; fb > 1; --fb)
    if (poss_lds_bytes(fb, 3, J, C, P, NL) <= POSS_LDS_MAX) return fb;
  return 1;
}

}  // namespace

namespace {

// The driver's workspace, carved in doubles (align 8; the int arrays are rounded to doubles).  Bf's input pointers
// (cams, p2d) are the caller's; the host-written inputs also as the pointers the driver uploads through.
struct PossWork {
  PossBufs Bf;
  double *ctl, *ssf;
  int *act, *done, *cons;
};

PossWork poss_layout(Carver& c, int B, int F, int J, int C, int P, int NL, int n_deriv) {
  const size_t NC = (size_t)C * F * J, NV = (size_t)F * J * 3 + NL + NC * P;
  const size_t M = 3 * NC + (size_t)(F - n_deriv) * J * 3 + (size_t)NL * F;
  const size_t FB = poss_frames_per_block(J, C, P, NL), BNB = (size_t)B * (((size_t)F + FB - 1) / FB);
  const size_t NVB = (size_t)B * NV, MB = (size_t)B * M;
  auto take = [&](size_t cnt) { return c.take<double>(cnt, 8); };
  PossWork W{};
  PossBufs& Bf = W.Bf;
  Bf.x = take(NVB);
  Bf.xt = take(NVB);
  Bf.g = take(NVB);
  Bf.vraw = take(NVB);
  Bf.vn = take(NVB);
  Bf.h = take(NVB);
  Bf.hbar = take(NVB);
  Bf.xl = take(NVB);
  Bf.s1 = take(NVB);
  Bf.s2 = take(NVB);
  Bf.f = take(MB);
  Bf.u = take(MB);
  Bf.js1 = take(MB);
  Bf.js2 = take(MB);
  Bf.Jx = take((size_t)B * NC * 6);
  Bf.Ja = take((size_t)B * NC * 3 * P);
  Bf.lenJ = take((size_t)B * F * NL * 4);
  Bf.part = take(BNB * POSS_NPF);
  Bf.upart = take(2 * BNB);
  Bf.vpart = take(2 * BNB);
  Bf.xpart = take(2 * BNB);
  Bf.Lpart = take(BNB * NL);
  Bf.st = take(2 * (size_t)B * POSS_NS);
  Bf.itn = take(B);
  Bf.ctl = W.ctl = take(4 * (size_t)B);
  Bf.ssf = W.ssf = take(B);
  Bf.act = W.act = reinterpret_cast<int*>(take(((size_t)B + 1) / 2 + 1));
  Bf.done = W.done = reinterpret_cast<int*>(take(((size_t)B + 1) / 2 + 1));
  Bf.cons = W.cons = reinterpret_cast<int*>(take((size_t)NL + 1));
  return W;
}

}  // namespace

size_t optim_possible_workspace_bytes(int B, int F, int J, int C, int P, int NL, int n_deriv) {
  return measure(poss_layout, B, F, J, C, P, NL, n_deriv);
}

// Host driver: the trf_no_bounds loop (scipy 1.15.3 optimize/_lsq/trf.py:401-540; oracle/trf.py), every animal on
// its own.  x: device (B, F J 3 + NL) in/out; anorm: device (B, C, F, J, P) out.  stats[8 b + ...] as
// optim_points_trf: initial cost, final cost, iterations, scipy's status, nfev, njev, lsmr iterations, longest run.
int optim_points_possible(const double* cams, int C, const double* p2d, double* x, double* anorm, int B, int F, int J,
                          int P, const int* cons_host, int n_strong, int n_weak, const double* ssf_host,
                          double scale_length, double scale_length_weak, double rp, int loss, int n_deriv,
                          int max_nfev_arg, double ftol, void* ws, size_t ws_bytes, double* stats,
                          hipStream_t s) {
  const int NL = n_strong + n_weak;
  if (B <= 0 || F <= 0 || J <= 0) return 0;
  if (P < 1 || P > POSS_MAXP || n_deriv < 1 || n_deriv > 3 || F <= n_deriv || C < 1 || NL > POSS_MAXL) return -2;
  PossDims D{};
  D.B = B;
  D.C = C;
  D.F = F;
  D.J = J;
  D.P = P;
  D.NL = NL;
  D.nS = n_strong;
  D.n = n_deriv;
  D.loss = loss;
  D.CJ = C * J;
  D.NC = C * F * J;
  D.NX = F * J * 3;
  D.NA = D.NC * P;
  D.NV = D.NX + NL + D.NA;
  D.MS0 = 2 * D.NC;
  D.MSM0 = 3 * D.NC;
  D.ML0 = D.MSM0 + (F - n_deriv) * J * 3;
  D.M = D.ML0 + NL * F;
  D.FB = poss_frames_per_block(J, C, P, NL);
  D.NB = (F + D.FB - 1) / D.FB;
  D.rp = rp;
  D.s_len = scale_length;
  D.s_len_weak = scale_length_weak;
  D.atol = 1e-6;
  D.btol = 1e-6;
  D.ctol = 1.0 / 1e8;
  {
    double cf[4];
    trf_diff_coefficients(n_deriv, cf);
    D.c0 = cf[0];
    D.c1 = cf[1];
    D.c2 = cf[2];
    D.c3 = cf[3];
  }
  const size_t lds = poss_lds_bytes(D.FB, n_deriv, J, C, P, NL);
  if (lds > POSS_LDS_MAX) return -2;
  const int NB = D.NB;
  const size_t BNB = (size_t)B * NB;
  Carver carver(ws, ws_bytes);
  const PossWork W = poss_layout(carver, B, F, J, C, P, NL, n_deriv);
  if (!carver.fits()) return -5;
  PossBufs Bf = W.Bf;
  Bf.cams = cams;
  Bf.p2d = p2d;
  double *ctl_d = W.ctl, *ssf_d = W.ssf;
  int *act_d = W.act, *done_d = W.done, *cons_d = W.cons;

  std::vector<int> act(B, 1), doneh(B, 0);
  std::vector<double> ctl(4 * (size_t)B, 0.0), part(BNB * POSS_NPF, 0.0), itnh(B, 0.0);
  auto sync = [&]() { return hipStreamSynchronize(s) == hipSuccess; };
  // (the host arrays of an upload stay untouched until the synchronisation that follows it)
  auto up = [&](void* d, const void* h, size_t bytes) {
    return bytes == 0 || hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
  };
  auto down = [&](void* h, const void* d, size_t bytes) {
    return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
  };
  auto read_part = [&]() { return down(part.data(), Bf.part, sizeof(double) * part.size()) && sync(); };
  // per-animal sum (or max) of a partial over the blocks, in block order
  auto psum = [&](int b, int field) {
    double v = 0.0;
    for (int k = 0; k < NB; ++k) v += part[((size_t)b * NB + k) * POSS_NPF + field];
    return v;
  };
  auto pmax = [&](int b, int field) {
    double v = 0.0;
    for (int k = 0; k < NB; ++k) v = std::max(v, part[((size_t)b * NB + k) * POSS_NPF + field]);
    return v;
  };
  const dim3 grid(NB, B), blk(POSS_THREADS);
  // f, J, g = J^T f, |point| and J g at x (src 0) or the trial point (src 1)
  auto launch_jac = [&](int src) {
    hipLaunchKernelGGL(poss_eval_kernel, grid, blk, 0, s, D, Bf, src);
    hipLaunchKernelGGL(poss_jt_kernel, grid, blk, lds, s, D, Bf, 0);
    hipLaunchKernelGGL(poss_jv_kernel, grid, blk, 0, s, D, Bf, 0);
  };
  if (!up(cons_d, cons_host, sizeof(int) * 2 * NL) || !up(ssf_d, ssf_host, sizeof(double) * B) ||
      !up(act_d, act.data(), sizeof(int) * B))
    return -3;
  hipLaunchKernelGGL(poss_init_kernel, grid, blk, 0, s, D, Bf, (const double*)x);
  launch_jac(0);
  if (!read_part()) return -3;

  std::vector<double> cost(B), gnorm2(B), ginf(B), rows(B), xnorm(B), areg(B), nparam(B);
  auto read_jac = [&](int b) {
    cost[b] = 0.5 * psum(b, PF_COST);
    rows[b] = psum(b, PF_ROWS);
    nparam[b] = D.NX + NL + psum(b, PF_NGOOD);
    gnorm2[b] = psum(b, PF_GG);
    ginf[b] = pmax(b, PF_GMAX);
    xnorm[b] = std::sqrt(psum(b, PF_PP));
    areg[b] = 0.5 * psum(b, PF_B00);
  };
  const double xtol = 1e-8, gtol = 1e-8;
  const int chunk = 16;  // lsmr iterations launched between two reads of the done flags
  enum { RUN, STOP };
  std::vector<int> state(B, RUN), status(B, 0), lsmr_total(B, 0), lsmr_max(B, 0), trial(B, 0);
  std::vector<long long> nfev(B, 1), njev(B, 1), max_nfev(B);
  std::vector<double> Delta(B), BS(3 * (size_t)B), gS(2 * (size_t)B), cost_new(B), actual(B), pred(B);
  for (int b = 0; b < B; ++b) {
    read_jac(b);
    stats[8 * b + 0] = cost[b];
    Delta[b] = xnorm[b] == 0 ? 1.0 : xnorm[b];
    max_nfev[b] = max_nfev_arg > 0 ? max_nfev_arg : 100LL * (long long)nparam[b];
  }
  for (;;) {
    bool any = false;
    for (int b = 0; b < B; ++b) {
      act[b] = 0;
      if (state[b] != RUN) continue;
      if (ginf[b] < gtol) status[b] = 1;  // trf.py:463-465
      if (status[b] != 0 || nfev[b] == max_nfev[b]) {
        state[b] = STOP;
        continue;
      }
      act[b] = 1;
      any = true;
    }
    if (!any) break;
    double maxit = 0.0;
    for (int b = 0; b < B; ++b) {
      ctl[4 * b] = ctl[4 * b + 1] = ctl[4 * b + 2] = ctl[4 * b + 3] = 0.0;
      doneh[b] = act[b] ? 0 : 1;
      if (!act[b]) continue;
      ctl[4 * b] = trf_regularize_damp(areg[b], gnorm2[b], Delta[b]);  // trf.py:480-484
      ctl[4 * b + 1] = std::min(rows[b], nparam[b]);
      maxit = std::max(maxit, ctl[4 * b + 1]);
    }
    if (!up(ctl_d, ctl.data(), sizeof(double) * ctl.size()) || !up(act_d, act.data(), sizeof(int) * B) ||
        !up(done_d, doneh.data(), sizeof(int) * B))
      return -3;
    // lsmr(J, f, damp): chunks of iterations, the done flags read between them
    hipLaunchKernelGGL(poss_jt_kernel, grid, blk, lds, s, D, Bf, 1);
    for (int k = 1;;) {
      for (int i = 0; i < chunk; ++i, ++k) {
        hipLaunchKernelGGL(poss_lsmr_u_kernel, grid, blk, lds, s, D, Bf, k);
        hipLaunchKernelGGL(poss_lsmr_v_kernel, grid, blk, lds, s, D, Bf, k);
      }
      if (!down(doneh.data(), done_d, sizeof(int) * B) || !sync()) return -3;
      bool all = true;
      for (int b = 0; b < B; ++b) all &= doneh[b] != 0;
      if (all) break;
      if (k > maxit + 4 + 2 * chunk) return -7;  // the device test stops every run by maxiter
    }
    // S = orth([g, gn]), g_S and B_S (trf.py:489-493)
    hipLaunchKernelGGL(poss_subspace_kernel, grid, blk, 0, s, D, Bf, 0);
    hipLaunchKernelGGL(poss_subspace_kernel, grid, blk, 0, s, D, Bf, 1);
    hipLaunchKernelGGL(poss_subspace_kernel, grid, blk, 0, s, D, Bf, 2);
    hipLaunchKernelGGL(poss_jv_kernel, grid, blk, 0, s, D, Bf, 1);
    if (!down(itnh.data(), Bf.itn, sizeof(double) * B) || !read_part()) return -3;
    for (int b = 0; b < B; ++b) {
      trial[b] = act[b];
      actual[b] = -1;
      if (!act[b]) continue;
      const int it = (int)itnh[b];
      lsmr_total[b] += it;
      lsmr_max[b] = std::max(lsmr_max[b], it);
      gS[2 * b] = psum(b, PF_GS0);
      gS[2 * b + 1] = psum(b, PF_GS1);
      BS[3 * b] = psum(b, PF_B00);
      BS[3 * b + 1] = psum(b, PF_B01);
      BS[3 * b + 2] = psum(b, PF_B11);
    }
    // the trial steps (trf.py:496-540), every animal until it accepts, terminates or runs out of evaluations
    for (;;) {
      bool anyt = false;
      for (int b = 0; b < B; ++b) {
        act[b] = trial[b] && actual[b] <= 0 && nfev[b] < max_nfev[b];
        trial[b] = act[b];
        if (!act[b]) continue;
        anyt = true;
        double p[2];
        if (mq_trust_region_2d(&BS[3 * b], &gS[2 * b], Delta[b], p) != 0) return -5;
        ctl[4 * b + 2] = p[0];
        ctl[4 * b + 3] = p[1];
        const double q = p[0] * (BS[3 * b] * p[0] + BS[3 * b + 1] * p[1]) + p[1] * (BS[3 * b + 1] * p[0] + BS[3 * b + 2] * p[1]);
        pred[b] = -(0.5 * q + (p[0] * gS[2 * b] + p[1] * gS[2 * b + 1]));
      }
      if (!anyt) break;
      if (!up(ctl_d, ctl.data(), sizeof(double) * ctl.size()) || !up(act_d, act.data(), sizeof(int) * B)) return -3;
      // the residuals at the trial point with J, g, |xt| and J g there: an accepted step needs nothing more; a
      // rejected one loses nothing the next trial needs (that uses x, s1, s2 and the host's B_S, g_S)
      hipLaunchKernelGGL(poss_step_kernel, grid, blk, 0, s, D, Bf);
      launch_jac(1);
      if (!read_part()) return -3;
      for (int b = 0; b < B; ++b) {
        if (!act[b]) continue;
        nfev[b]++;
        const double sh = std::sqrt(psum(b, PF_STEP));
        const double cn = 0.5 * psum(b, PF_COST);
        if (!std::isfinite(cn)) {
          Delta[b] = 0.25 * sh;
          actual[b] = -1;
          continue;
        }
        cost_new[b] = cn;
        actual[b] = cost[b] - cn;
        double ratio;
        const double Dn = trf_update_tr_radius(Delta[b], actual[b], pred[b], sh, sh > 0.95 * Delta[b], ratio);
        const int term = trf_check_termination(actual[b], cost[b], sh, xnorm[b], ratio, ftol, xtol);
        if (term) {
          status[b] = term;
          trial[b] = 0;
          continue;
        }
        Delta[b] = Dn;
      }
    }
    // accepted steps: x = x_new, with J, g, |x| and J g as the animal's last trial evaluated them (trf.py:522-540)
    bool anya = false;
    for (int b = 0; b < B; ++b) {
      act[b] = state[b] == RUN && actual[b] > 0;
      if (!act[b]) continue;
      anya = true;
      njev[b]++;
      read_jac(b);
    }
    if (anya) {
      if (!up(act_d, act.data(), sizeof(int) * B)) return -3;
      hipLaunchKernelGGL(poss_accept_kernel, grid, blk, 0, s, D, Bf);
      if (!sync()) return -3;
    }
  }
  hipLaunchKernelGGL(poss_finish_kernel, grid, blk, 0, s, D, Bf, x, anorm);
  if (!sync()) return -3;
  for (int b = 0; b < B; ++b) {
    stats[8 * b + 1] = cost[b];
    stats[8 * b + 2] = (double)(njev[b] - 1);
    stats[8 * b + 3] = status[b];
    stats[8 * b + 4] = (double)nfev[b];
    stats[8 * b + 5] = (double)njev[b];
    stats[8 * b + 6] = lsmr_total[b];
    stats[8 * b + 7] = lsmr_max[b];
  }
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace mq
