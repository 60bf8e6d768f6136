// The two anipose consumers that choose among more than one candidate per (instance, joint): the
// n_possible > 1 Viterbi filter (mq_viterbi_filter_multi, filter_pose.py:26-120,151-186) and
// CameraGroup.triangulate_possible (mq_triangulate_possible, cameras.py:639-724).  The candidates come from
// the top-K heatmap decode (mq_decode_udp_topk, imgproc.hip).
// Compiled with -ffp-contract=off: every expression rounds like the numpy / scipy oracle and like the
// single-candidate kernels (geometry.hip), whose results K = 1 / P = 1 reproduce bit for bit.
#include "common.hpp"
#include "camera.hpp"
#include "candidates.hpp"
#include "dlt_dev.hpp"
#include "viterbi_dev.hpp"
#include "workspace.hpp"

namespace mq {

// ------------------------------------------------------------------ Viterbi, n_possible > 1
// filter_pose.py:26-46 (remove_dups), 48-120 (viterbi_path), 151-186 (filter_pose_viterbi) for
// kp (A, F, C, J, K, 3).  A frame has up to K * n_back <= 12 particles, so the n_back^2 register
// transitions of viterbi_dp_kernel do not carry over; here one wave owns one chain.  Per frame: lanes
// 0..K*n_back-1 each test one candidate and a ballot compacts the survivors into the frame's particle
// list in LDS; the up to 144 transitions (q of this frame, p of the last) are spread over the 64 lanes,
// computed on the fly (no scratch) and added to the predecessor's log-probability; then lane q walks its
// row in ascending p (np.max / np.argmax: first maximum, a NaN wins and sticks).  Back-pointers (int8)
// and then the backtracked path go to a [chain][F][K * n_back] scratch.
constexpr int VM_LANES = 64;  // one wave per chain
constexpr int VM_MAXP = 12;

struct VitMulti {
  const double* kp;
  int F, C, J, K, n_back;
  double score_thr;
  __device__ const double* at(int a, int c, int j, int f, int k) const {
    return kp + (((((size_t)a * F + f) * C + c) * J + j) * K + k) * 3;
  }
  // points_full[scores < thr] = NaN
  __device__ void cand(const double* p, double& x, double& y, double& s) const {
    s = p[2];
    const bool masked = s < score_thr;
    x = masked ? NAN : p[0];
    y = masked ? NAN : p[1];
  }
  // Candidate k of frame f is a particle iff its x is not NaN and remove_dups(thres=5) keeps it: no
  // lower-index candidate of the frame within 5 px (non-finite coordinates count as 1e9, as there).
  __device__ bool survives(int a, int c, int j, int f, int k, double& x, double& y, double& s) const {
    cand(at(a, c, j, f, k), x, y, s);
    if (x != x) return false;
    const double mx = isfinite(x) ? x : 1e9, my = isfinite(y) ? y : 1e9;
    for (int k2 = 0; k2 < k; ++k2) {
      double x2, y2, s2;
      cand(at(a, c, j, f, k2), x2, y2, s2);
      const double dx = mx - (isfinite(x2) ? x2 : 1e9), dy = my - (isfinite(y2) ? y2 : 1e9);
      if (dx * dx + dy * dy <= 25.0) return false;
    }
    return true;
  }
};

__global__ __launch_bounds__(VM_LANES) void viterbi_multi_kernel(VitMulti V, int chains, double thres_dist,
                                                                 int8_t* __restrict__ bk_all,
                                                                 double* __restrict__ out) {
  __shared__ double sx[2][VM_MAXP], sy[2][VM_MAXP], ss[2][VM_MAXP], sT[2][VM_MAXP];
  __shared__ double sV[VM_MAXP * VM_MAXP];  // sV[q][p] = T[p] + P(q | p)
  __shared__ int scnt[2];
  const int l = threadIdx.x;
  const int ch = blockIdx.x;
  if (ch >= chains) return;
  const int F = V.F, K = V.K, NB = V.n_back;
  const int P = K * NB;
  const int j = ch % V.J, c = (ch / V.J) % V.C, a = ch / (V.J * V.C);
  int8_t* bk = bk_all + (size_t)ch * F * P;
  // particles of frame i into buffer `buf`: lane l = jj * K + k looks at candidate k of frame i - jj;
  // survivors keep that order (frames i, i-1, ..., ascending k), scores times 2^-jj
  auto build = [&](int i, int buf) {
    bool sv = false;
    double x = 0, y = 0, s = 0;
    if (l < P) {
      const int jj = l / K, k = l % K;
      if (i - jj >= 0) {
        sv = V.survives(a, c, j, i - jj, k, x, y, s);
        double w = 1.0;
        for (int t = 0; t < jj; ++t) w = w * 0.5;
        s = s * w;
      }
    }
    const unsigned long long m = __ballot(sv);
    const int pos = __popcll(m & ((1ull << l) - 1ull));
    const int cnt = __popcll(m);
    if (sv) {
      sx[buf][pos] = x;
      sy[buf][pos] = y;
      ss[buf][pos] = s;
    }
    if (l == 0) {
      if (cnt == 0) {
        sx[buf][0] = -1;
        sy[buf][0] = -1;
        ss[buf][0] = 0.001;
      }
      scnt[buf] = cnt == 0 ? 1 : cnt;
    }
  };
  build(0, 0);
  __syncthreads();
  int va = scnt[0];
  if (l < VM_MAXP) sT[0][l] = (l < va) ? log(ss[0][l]) : -INFINITY;
  __syncthreads();
  int cur = 0;
  for (int i = 1; i < F; ++i) {
    const int nxt = cur ^ 1;
    build(i, nxt);
    __syncthreads();
    const int vb = scnt[nxt];
    for (int t = l; t < vb * va; t += VM_LANES) {
      const int q = t / va, p = t % va;
      const double bx = sx[nxt][q], by = sy[nxt][q];
      const double ax = sx[cur][p], ay = sy[cur][p];
      double Pt;
      if (bx == -1 || ax == -1) {
        Pt = log(0.001);
      } else {
        const double dx = ax - bx, dy = ay - by;
        Pt = trans_logprob(sqrt(dx * dx + dy * dy), thres_dist);
      }
      sV[q * VM_MAXP + p] = sT[cur][p] + Pt;
    }
    __syncthreads();
    if (l < vb) {
      double best = sV[l * VM_MAXP];
      int arg = 0;
      for (int p = 1; p < va; ++p) {
        const double v = sV[l * VM_MAXP + p];
        // np.max / np.argmax semantics: first maximum, a NaN wins and sticks
        if (!(best != best) && ((v != v) || v > best)) {
          best = v;
          arg = p;
        }
      }
      sT[nxt][l] = best + log(ss[nxt][l]);
      bk[(size_t)i * P + l] = (int8_t)arg;
    }
    __syncthreads();
    va = vb;
    cur = nxt;
  }
  // backtrack from the first argmax of the last frame; the path goes into slot 0 of each frame
  if (l == 0) {
    int at = 0;
    for (int p = 1; p < va; ++p)
      if (sT[cur][p] > sT[cur][at]) at = p;
    for (int i = F - 1; i >= 0; --i) {
      const int nx = i > 0 ? bk[(size_t)i * P + at] : 0;
      bk[(size_t)i * P] = (int8_t)at;
      at = nx;
    }
  }
  __syncthreads();
  // output rows: particle number bk[f][0] of frame f, found by walking the frame's particle order
  for (int f = l; f < F; f += VM_LANES) {
    const int want = bk[(size_t)f * P];
    double ox = -1, oy = -1, os = 0.001;
    int cnt = 0;
    bool found = false;
    double w = 1.0;
    for (int jj = 0; jj < NB && !found; ++jj) {
      if (f - jj < 0) break;
      for (int k = 0; k < K; ++k) {
        double x, y, s;
        if (!V.survives(a, c, j, f - jj, k, x, y, s)) continue;
        if (cnt == want) {
          ox = x;
          oy = y;
          os = s * w;
          found = true;
          break;
        }
        ++cnt;
      }
      w = w * 0.5;
    }
    double* o = out + ((((size_t)a * F + f) * V.C + c) * V.J + j) * 3;
    o[0] = ox;
    o[1] = oy;
    o[2] = os;
  }
}

namespace {

// the back-pointers [chain][F][K * n_back]; a frame's slot 0 holds the path once it is walked
int8_t* viterbi_multi_layout(Carver& c, int A, int F, int C, int J, int K, int n_back) {
  return c.take<int8_t>((size_t)A * C * J * F * K * n_back);
}

}  // namespace

size_t viterbi_multi_scratch_bytes(int A, int F, int C, int J, int K, int n_back) {
  return measure(viterbi_multi_layout, A, F, C, J, K, n_back);
}

int viterbi_filter_multi(const double* kp, int A, int F, int C, int J, int K, double score_thr, int n_back,
                         double thres_dist, void* scratch, size_t scratch_bytes, double* out, hipStream_t s) {
  const int chains = A * C * J;
  if (chains <= 0 || F <= 0) return 0;
  if (n_back > 3 || n_back < 1 || K < 1 || K > CAND_MAX) return -2;
  Carver c(scratch, scratch_bytes);
  int8_t* bk = viterbi_multi_layout(c, A, F, C, J, K, n_back);
  if (!c.fits()) return -5;
  VitMulti V{kp, F, C, J, K, n_back, score_thr};
  hipLaunchKernelGGL(viterbi_multi_kernel, dim3(chains), dim3(VM_LANES), 0, s, V, chains, thres_dist, bk, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------ triangulate_possible (cameras.py:639-724)
// and, with one candidate per camera, triangulate_ransac (cameras.py:726-743).

// DLT over the cameras of `use` whose undistortion succeeded (ux[c] not NaN) into p, then the mean
// reprojection error of p over the cameras of `use` (CameraGroup.reprojection_error(mean=True): NaN norms
// dropped, fewer than two -> NaN).  raw(c, u, v) gives the raw pixel of camera c.
template <int MAXC, class Raw>
__device__ __forceinline__ double reproj_mean_error(const double* cams, int C, unsigned use,
                                                    const double (&ux)[MAXC], const double (&uy)[MAXC], Raw raw,
                                                    double (&p)[3]) {
  unsigned ok = 0;
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (((use >> c) & 1u) && !(ux[c] != ux[c])) ok |= 1u << c;
  p[0] = p[1] = p[2] = NAN;
  if (__popc(ok) >= 2) dlt_point<MAXC>(cams, C, ux, uy, ok, p);
  double sum = 0.0, cnt = 0.0;
  for (int c = 0; c < C; ++c) {
    if (!((use >> c) & 1u)) continue;
    double u, v, ru, rv;
    cam_project(cam_at(cams, c), p[0], p[1], p[2], u, v);
    raw(c, ru, rv);
    const double ex = ru - u, ey = rv - v;
    const double nr = sqrt(ex * ex + ey * ey);
    if (!(nr != nr)) {
      sum = sum + nr;
      cnt = cnt + 1.0;
    }
  }
  return (cnt < 1.5) ? NAN : sum / cnt;
}

// The search of one wave over subsets 0..nsub-1 in the serial (itertools.product) order: lane l takes
// err_of(base + l) (NaN = subset not tried), 64 subsets at a time.  The first chunk holding an error
// < threshold ends the search at its first such subset, which reproduces the serial early exit exactly;
// otherwise the first strict minimum below 200 wins, or -1.  The result is uniform across the wave.
template <class ErrOf>
__device__ __forceinline__ int first_hit_or_min(int nsub, double threshold, ErrOf err_of) {
  const int lane = threadIdx.x;
  double best_err = 200.0;
  int best_s = 0x7fffffff;
  for (int base = 0; base < nsub; base += 64) {
    const int s = base + lane;
    double err = NAN;
    if (s < nsub) err = err_of(s);
    // first subset (smallest s) in this chunk with err < threshold
    const bool hit = err < threshold;
    const unsigned long long hits = __ballot(hit);
    if (hits) return base + __ffsll((long long)hits) - 1;
    // running strict minimum, ties keep the earlier subset
    double e = (err < 200.0) ? err : INFINITY;
    int es = (err < 200.0) ? s : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double e2 = __shfl_xor(e, o, 64);
      const int s2 = __shfl_xor(es, o, 64);
      if (e2 < e || (e2 == e && s2 < es)) {
        e = e2;
        es = s2;
      }
    }
    if (es != 0x7fffffff && (e < best_err || (e == best_err && es < best_s))) {
      best_err = e;
      best_s = es;
    }
  }
  return best_s != 0x7fffffff ? best_s : -1;
}

// One wave per point; the cameras with a non-NaN candidate take part, each with its candidates in
// ascending k and then "none", so a combination is a mixed-radix number whose slowest digit is the first
// camera (itertools.product order), searched by first_hit_or_min.  Raw and undistorted candidates sit in
// LDS; a lane gathers its combination into registers.
template <int MAXC>
__global__ __launch_bounds__(64) void possible_kernel(const double* __restrict__ cams, int C,
                                                      const double* __restrict__ pts, int N, int P, int min_cams,
                                                      double threshold, double* __restrict__ out_p3d,
                                                      uint8_t* __restrict__ out_picked,
                                                      double* __restrict__ out_p2d, double* __restrict__ out_err) {
  __shared__ double s_raw[MAXC * CAND_MAX][2], s_und[MAXC * CAND_MAX][2];
  __shared__ int s_cnt[MAXC];
  __shared__ uint8_t s_list[MAXC][CAND_MAX];
  const int n = blockIdx.x;
  const int lane = threadIdx.x;
  for (int t = lane; t < C * P; t += 64) {
    const int c = t / P, k = t % P;
    const size_t o = 2 * (((size_t)c * N + n) * P + k);
    const double u = pts[o], v = pts[o + 1];
    double x = NAN, y = NAN;
    if (!(u != u)) cam_undistort(cam_at(cams, c), u, v, x, y);
    s_raw[c * CAND_MAX + k][0] = u;
    s_raw[c * CAND_MAX + k][1] = v;
    s_und[c * CAND_MAX + k][0] = x;
    s_und[c * CAND_MAX + k][1] = y;
  }
  __syncthreads();
  if (lane < MAXC) {
    int cnt = 0;
    if (lane < C)
      for (int k = 0; k < P; ++k) {
        const double u = s_raw[lane * CAND_MAX + k][0];
        if (!(u != u)) s_list[lane][cnt++] = (uint8_t)k;
      }
    s_cnt[lane] = cnt;
  }
  __syncthreads();
  int rad[MAXC];  // options of camera c without "none"; 0 = the camera does not take part
  int m = 0, nsub = 1;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    rad[c] = s_cnt[c];
    if (rad[c] > 0) {
      ++m;
      nsub *= rad[c] + 1;
    }
  }
  // combination s -> cameras used (bit c of use), candidate of each (2 bits per camera in sel) and
  // their undistorted coordinates; the last camera is the fastest digit
  auto gather = [&](int s, unsigned& use, unsigned& sel, double (&ux)[MAXC], double (&uy)[MAXC]) {
    int rem = s;
    use = 0;
    sel = 0;
#pragma unroll
    for (int c = MAXC - 1; c >= 0; --c) {
      ux[c] = uy[c] = 0;
      if (rad[c] > 0) {
        const int r = rad[c] + 1;
        const int d = rem % r;
        rem /= r;
        if (d < rad[c]) {
          const int k = s_list[c][d];
          use |= 1u << c;
          sel |= (unsigned)k << (2 * c);
          ux[c] = s_und[c * CAND_MAX + k][0];
          uy[c] = s_und[c * CAND_MAX + k][1];
        }
      }
    }
  };
  // raw pixel of camera c in a combination whose candidates are sel
  const auto raw_of = [&](unsigned sel) {
    return [sel](int c, double& u, double& v) {
      const int k = (sel >> (2 * c)) & 3u;
      u = s_raw[c * CAND_MAX + k][0];
      v = s_raw[c * CAND_MAX + k][1];
    };
  };
  double ux[MAXC], uy[MAXC];
  int chosen = -1;
  if (m >= 2)
    chosen = first_hit_or_min(nsub, threshold, [&](int s) -> double {
      unsigned use, sel;
      gather(s, use, sel, ux, uy);
      const int k = __popc(use);
      if ((k < min_cams && k != m) || k < 2) return NAN;
      double p[3];
      return reproj_mean_error<MAXC>(cams, C, use, ux, uy, raw_of(sel), p);
    });
  if (lane != 0) return;
  double p[3] = {NAN, NAN, NAN};
  double err = 0.0;
  unsigned use = 0, sel = 0;
  if (chosen >= 0) {
    gather(chosen, use, sel, ux, uy);
    err = reproj_mean_error<MAXC>(cams, C, use, ux, uy, raw_of(sel), p);
  }
  out_p3d[3 * (size_t)n] = p[0];
  out_p3d[3 * (size_t)n + 1] = p[1];
  out_p3d[3 * (size_t)n + 2] = p[2];
  out_err[n] = err;
  for (int c = 0; c < C; ++c) {
    const bool on = (use >> c) & 1u;
    const int ks = (sel >> (2 * c)) & 3u;
    for (int k = 0; k < P; ++k) out_picked[((size_t)c * N + n) * P + k] = (on && k == ks) ? 1 : 0;
    out_p2d[2 * ((size_t)c * N + n)] = on ? s_raw[c * CAND_MAX + ks][0] : NAN;
    out_p2d[2 * ((size_t)c * N + n) + 1] = on ? s_raw[c * CAND_MAX + ks][1] : NAN;
  }
}

int triangulate_possible(const double* cams, int C, const double* pts, int N, int P, int min_cams, double threshold,
                         double* p3d, uint8_t* picked, double* p2d, double* err, hipStream_t s) {
  if (N <= 0) return 0;
  if (C < 1 || C > 16 || P < 1 || P > CAND_MAX) return -2;
  long combos = 1;
  for (int c = 0; c < C; ++c) {
    combos *= P + 1;
    if (combos > 65536) return -2;
  }
  if (C <= 8)
    hipLaunchKernelGGL(possible_kernel<8>, dim3(N), dim3(64), 0, s, cams, C, pts, N, P, min_cams, threshold, p3d,
                       picked, p2d, err);
  else
    hipLaunchKernelGGL(possible_kernel<16>, dim3(N), dim3(64), 0, s, cams, C, pts, N, P, min_cams, threshold, p3d,
                       picked, p2d, err);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// CameraGroup.triangulate_ransac is triangulate_possible with n_possible = 1: the same subsets in the same
// order, and picked [C][N][1] is [C][N].
int triangulate_ransac(const double* cams, int C, const double* pts, int N, int min_cams, double threshold,
                       double* p3d, uint8_t* picked, double* p2d, double* err, hipStream_t s) {
  return triangulate_possible(cams, C, pts, N, 1, min_cams, threshold, p3d, picked, p2d, err, s);
}

}  // namespace mq
