// More than one candidate per (instance, joint): the top-K heatmap peaks (mq_decode_udp_topk) and
// the two anipose consumers that choose among candidates, the n_possible > 1 Viterbi filter
// (mq_viterbi_filter_multi, filter_pose.py:26-120,151-186) and CameraGroup.triangulate_possible
// (mq_triangulate_possible, cameras.py:639-724).
// Compiled with -ffp-contract=off: every expression rounds like the numpy / scipy oracle and like
// the single-candidate kernels (imgproc.hip, geometry.hip), whose results slot 0 / K = 1 / P = 1
// reproduce bit for bit.
#include "common.hpp"
#include "camera.hpp"
#include "candidates.hpp"
#include "dlt_dev.hpp"
#include "viterbi_dev.hpp"

namespace mq {

// ------------------------------------------------------------------ top-K peaks + DARK-UDP decode
// The 11-tap Gaussian of decode_blur_kernel (imgproc.hip kGauss11; a __constant__ table cannot be
// shared across translation units): cv2.getGaussianKernel(11, sigma 0 -> 2.0) in float64, rounded
// to float32.  A CPU test pins both tables against oracle/decode.py:gaussian_kernel_1d.
__constant__ float kGauss11Cand[11] = {
    0.00881222914904356f, 0.027143577113747597f, 0.06511405855417252f, 0.12164907157421112f,
    0.17699836194515228f, 0.2005654126405716f,   0.17699836194515228f, 0.12164907157421112f,
    0.06511405855417252f, 0.027143577113747597f, 0.00881222914904356f};

constexpr int CAND_MAX = 4;

// Block argmax of (value, flat index) pairs: highest value, lowest index on ties; index 0x7fffffff
// = "nothing".  The result is left in red_v[0] / red_i[0]; the caller synchronises before reuse.
__device__ __forceinline__ void block_best(float bv, int bi, float* red_v, int* red_i) {
  red_v[threadIdx.x] = bv;
  red_i[threadIdx.x] = bi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      const float v2 = red_v[threadIdx.x + o];
      const int i2 = red_i[threadIdx.x + o];
      const float v1 = red_v[threadIdx.x];
      const int i1 = red_i[threadIdx.x];
      const bool none1 = i1 == 0x7fffffff, none2 = i2 == 0x7fffffff;
      if (!none2 && (none1 || v2 > v1 || (v2 == v1 && i2 < i1))) {
        red_v[threadIdx.x] = v2;
        red_i[threadIdx.x] = i2;
      }
    }
    __syncthreads();
  }
}

// Stage 1, one block per (instance, joint): decode_blur_kernel's first argmax, blur, rescale, clip and
// log with the same operations in the same order, plus the peak rule on the raw map before the blur
// overwrites it: peaks are flagged in parallel (into the not yet used row buffer), then n_cand - 1
// rounds of block argmax take the highest peak farther than min_sep (Chebyshev) from every peak taken.
__global__ __launch_bounds__(256) void topk_blur_kernel(const float* __restrict__ avg, int HH, int WW, int n_cand,
                                                        int min_sep, float min_score, float* __restrict__ work,
                                                        int32_t* __restrict__ peak, float* __restrict__ score) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int nk = blockIdx.x;
  const int plane = HH * WW;
  const int PR = HH + 10;  // padded rows
  float* hmap = sm;          // HH*WW
  float* rows = sm + plane;  // PR*WW (peak flags first, then the row-filtered padded rows)
  __shared__ float red_v[256];
  __shared__ int red_i[256];
  __shared__ int tk_i[CAND_MAX];
  __shared__ float tk_v[CAND_MAX];
  const float* src = avg + (int64_t)nk * plane;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < plane; i += blockDim.x) {
    const float v = src[i];
    hmap[i] = v;
    if (v > bv || (v == bv && i < bi) || (v != v && bv == bv)) {  // NaN counts as max (np.argmax)
      bv = v;
      bi = i;
    }
  }
  red_v[threadIdx.x] = bv;
  red_i[threadIdx.x] = bi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      const float v2 = red_v[threadIdx.x + o];
      const int i2 = red_i[threadIdx.x + o];
      const float v1 = red_v[threadIdx.x];
      const int i1 = red_i[threadIdx.x];
      const bool n1 = v1 != v1, n2 = v2 != v2;
      bool take2;
      if (n1 || n2)
        take2 = n2 && (!n1 || i2 < i1);
      else
        take2 = (v2 > v1) || (v2 == v1 && i2 < i1);
      if (take2) {
        red_v[threadIdx.x] = v2;
        red_i[threadIdx.x] = i2;
      }
    }
    __syncthreads();
  }
  const float origin_max = red_v[0];
  const int origin_arg = red_i[0];
  __syncthreads();  // red_* are reused below
  // ---- slots 1..: the peak rule on the raw map
  const bool any_peak = origin_max > fmaxf(0.f, min_score);  // false for a NaN maximum
  if (threadIdx.x == 0) {
    tk_i[0] = origin_arg;
    tk_v[0] = origin_max;
    for (int k = 1; k < CAND_MAX; ++k) {
      tk_i[k] = -1;
      tk_v[k] = 0.f;
    }
  }
  if (n_cand > 1 && any_peak) {
    for (int i = threadIdx.x; i < plane; i += blockDim.x) {
      const float v = hmap[i];
      const int y = i / WW, x = i % WW;
      bool pk = v > min_score;
      for (int dy = -1; dy <= 1 && pk; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= HH) continue;
        for (int dx = -1; dx <= 1; ++dx) {
          const int xx = x + dx;
          if ((dx == 0 && dy == 0) || xx < 0 || xx >= WW) continue;
          const int q = yy * WW + xx;
          const float hq = hmap[q];
          if (!(v > hq || (v == hq && i < q))) pk = false;
        }
      }
      rows[i] = pk ? 1.f : 0.f;
    }
    __syncthreads();
    for (int k = 1; k < n_cand; ++k) {
      float cv = -INFINITY;
      int ci = 0x7fffffff;
      for (int i = threadIdx.x; i < plane; i += blockDim.x) {
        if (rows[i] == 0.f) continue;
        const int y = i / WW, x = i % WW;
        bool far = true;
        for (int t = 0; t < k; ++t) {
          const int ty = tk_i[t] / WW, tx = tk_i[t] % WW;
          const int ax = x > tx ? x - tx : tx - x, ay = y > ty ? y - ty : ty - y;
          if ((ax > ay ? ax : ay) <= min_sep) far = false;
        }
        if (!far) continue;
        const float v = hmap[i];
        if (ci == 0x7fffffff || v > cv) {  // ascending i: the first of equal values stays
          cv = v;
          ci = i;
        }
      }
      block_best(cv, ci, red_v, red_i);
      const int got = red_i[0];
      const float gotv = red_v[0];
      __syncthreads();
      if (got == 0x7fffffff) break;  // no peak left (uniform across the block)
      if (threadIdx.x == 0) {
        tk_i[k] = got;
        tk_v[k] = gotv;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (threadIdx.x < n_cand) {
    peak[(int64_t)nk * n_cand + threadIdx.x] = tk_i[threadIdx.x];
    score[(int64_t)nk * n_cand + threadIdx.x] = tk_v[threadIdx.x];
  }
  __syncthreads();  // the peak flags in rows are dead from here
  // ---- decode_blur_kernel's blur: row pass over the padded map: rows[r][x] = sum_t g[t] * dr[r][x + t]
  for (int i = threadIdx.x; i < PR * WW; i += blockDim.x) {
    const int r = i / WW, x = i % WW;
    const int yy = r - 5;
    float acc;
    if (yy < 0 || yy >= HH) {
      acc = 0.f;
    } else {
      const float* hr = hmap + yy * WW;
      int c = x - 5;
      acc = kGauss11Cand[0] * ((c >= 0 && c < WW) ? hr[c] : 0.f);
      for (int t = 1; t < 11; ++t) {
        c = x + t - 5;
        acc = acc + kGauss11Cand[t] * ((c >= 0 && c < WW) ? hr[c] : 0.f);
      }
    }
    rows[i] = acc;
  }
  __syncthreads();
  // column pass -> blurred (stored back into hmap), track its max
  float lmax = -INFINITY;
  for (int i = threadIdx.x; i < plane; i += blockDim.x) {
    const int y = i / WW, x = i % WW;
    float acc = kGauss11Cand[0] * rows[y * WW + x];
    for (int t = 1; t < 11; ++t) acc = acc + kGauss11Cand[t] * rows[(y + t) * WW + x];
    hmap[i] = acc;
    lmax = fmaxf(lmax, acc);
  }
  __syncthreads();
  red_v[threadIdx.x] = lmax;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red_v[threadIdx.x] = fmaxf(red_v[threadIdx.x], red_v[threadIdx.x + o]);
    __syncthreads();
  }
  const float ratio = origin_max / red_v[0];
  float* dst = work + (int64_t)nk * plane;
  for (int i = threadIdx.x; i < plane; i += blockDim.x) {
    float v = hmap[i] * ratio;
    v = fminf(fmaxf(v, 0.001f), 50.0f);
    dst[i] = logf(v);
  }
}

// imgproc.hip's padded_at: element of numpy's flattened edge-padded (J, H+2, W+2) log map with Python
// negative-index wrap-around (slot 0 of a joint whose max <= 0 reads through it, loc = -1).
__device__ __forceinline__ float cand_padded_at(const float* work_inst, int K, int HH, int WW, long idx) {
  const long per = (long)(HH + 2) * (WW + 2);
  const long total = per * K;
  if (idx < 0) idx += total;
  const int k = (int)(idx / per);
  const int rem = (int)(idx % per);
  int pr = rem / (WW + 2) - 1, pc = rem % (WW + 2) - 1;
  pr = pr < 0 ? 0 : (pr >= HH ? HH - 1 : pr);
  pc = pc < 0 ? 0 : (pc >= WW ? WW - 1 : pc);
  return work_inst[((long)k * HH + pr) * WW + pc];
}

// Stage 2, one thread per (instance, joint, slot): decode_refine_kernel's DARK-UDP Newton step and
// image-space mapping, same arithmetic, started from the slot's peak.  Slot 0 keeps the loc = -1 rule
// for max <= 0; a slot >= 1 is a peak inside the map, so its reads stay inside its own joint's map.
__global__ void topk_refine_kernel(const float* __restrict__ work, const int32_t* __restrict__ peak,
                                   const float* __restrict__ score, int N, int K, int n_cand, int HH, int WW,
                                   const float* __restrict__ center, const float* __restrict__ scale, int in_w,
                                   int in_h, double* __restrict__ kp_img, float* __restrict__ kp_hm) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * K * n_cand) return;
  const int slot = t % n_cand;
  const int i = t / n_cand;
  const int n = i / K, k = i % K;
  if (slot > 0 && (peak[t] < 0 || peak[t] >= HH * WW)) {  // empty slot
    kp_img[2 * t] = NAN;
    kp_img[2 * t + 1] = NAN;
    if (kp_hm) {
      kp_hm[2 * t] = NAN;
      kp_hm[2 * t + 1] = NAN;
    }
    return;
  }
  const float* wi = work + (long)n * K * HH * WW;
  float lx, ly;
  if (slot == 0 && score[t] <= 0.f) {
    lx = -1.f;
    ly = -1.f;
  } else {
    lx = (float)(peak[t] % WW);
    ly = (float)(peak[t] / WW);
  }
  const int W2 = WW + 2;
  const float fidx = lx + 1.f + (ly + 1.f) * (float)W2;
  const long index = (long)fidx + (long)W2 * (HH + 2) * k;
  const float i_ = cand_padded_at(wi, K, HH, WW, index);
  const float ix1 = cand_padded_at(wi, K, HH, WW, index + 1);
  const float iy1 = cand_padded_at(wi, K, HH, WW, index + W2);
  const float ix1y1 = cand_padded_at(wi, K, HH, WW, index + W2 + 1);
  const float ix1_y1_ = cand_padded_at(wi, K, HH, WW, index - W2 - 1);
  const float ix1_ = cand_padded_at(wi, K, HH, WW, index - 1);
  const float iy1_ = cand_padded_at(wi, K, HH, WW, index - W2);
  const float dx = 0.5f * (ix1 - ix1_);
  const float dy = 0.5f * (iy1 - iy1_);
  const float dxx = ix1 - 2.f * i_ + ix1_;
  const float dxy = 0.5f * (ix1y1 - ix1 - iy1 + i_ + i_ - ix1_ - iy1_ + ix1_y1_);
  const float dyy = iy1 - 2.f * i_ + iy1_;
  const double eps = 1.1920928955078125e-07;
  // inv([[a b][c d]]) by LU with partial pivoting (LAPACK getrf/getrs order)
  double a = (double)dxx + eps, b = (double)dxy + 0.0, c = (double)dxy + 0.0, d = (double)dyy + eps;
  bool swap = fabs(c) > fabs(a);
  double p = swap ? c : a, q = swap ? d : b, r = swap ? a : c, s = swap ? b : d;
  const double l = r * (1.0 / p);
  const double u22 = s - l * q;
  double inv[2][2];
  for (int j = 0; j < 2; ++j) {
    double b1 = (j == 0) ? (swap ? 0.0 : 1.0) : (swap ? 1.0 : 0.0);
    double b2 = (j == 0) ? (swap ? 1.0 : 0.0) : (swap ? 0.0 : 1.0);
    b2 = b2 - l * b1;
    b2 = b2 / u22;
    b1 = b1 - b2 * q;
    b1 = b1 / p;
    inv[0][j] = b1;
    inv[1][j] = b2;
  }
  const double stx = inv[0][0] * (double)dx + inv[0][1] * (double)dy;
  const double sty = inv[1][0] * (double)dx + inv[1][1] * (double)dy;
  const float kx = (float)((double)lx - stx);
  const float ky = (float)((double)ly - sty);
  if (kp_hm) {
    kp_hm[2 * t] = kx;
    kp_hm[2 * t + 1] = ky;
  }
  const double ix = (double)kx / (double)(WW - 1) * (double)in_w;
  const double iy = (double)ky / (double)(HH - 1) * (double)in_h;
  const float s0 = scale[2 * n], s1 = scale[2 * n + 1];
  const float h0 = 0.5f * s0, h1 = 0.5f * s1;
  kp_img[2 * t] = ix / (double)in_w * (double)s0 + (double)center[2 * n] - (double)h0;
  kp_img[2 * t + 1] = iy / (double)in_h * (double)s1 + (double)center[2 * n + 1] - (double)h1;
}

int udp_decode_topk(const float* avg, int n, int joints, int h, int w, const float* center, const float* scale,
                    int in_w, int in_h, int n_cand, int min_sep, float min_score, float* work, double* kp_img,
                    float* score, int32_t* peak, float* kp_hm, hipStream_t s) {
  if (n <= 0) return 0;
  if (n_cand < 1 || n_cand > CAND_MAX) return -2;
  const size_t lds = (size_t)(h * w + (h + 10) * w) * sizeof(float);
  hipLaunchKernelGGL(topk_blur_kernel, dim3(n * joints), dim3(256), lds, s, avg, h, w, n_cand, min_sep, min_score,
                     work, peak, score);
  const int tot = n * joints * n_cand;
  hipLaunchKernelGGL(topk_refine_kernel, dim3((tot + 127) / 128), dim3(128), 0, s, work, peak, score, n, joints,
                     n_cand, h, w, center, scale, in_w, in_h, kp_img, kp_hm);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

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

size_t viterbi_multi_scratch_bytes(int A, int F, int C, int J, int K, int n_back) {
  return (size_t)A * C * J * F * K * n_back + 512;
}

// scratch: viterbi_multi_scratch_bytes() -- back-pointers, then the path.
int viterbi_filter_multi(const double* kp, int A, int F, int C, int J, int K, double score_thr, int n_back,
                         double thres_dist, void* scratch, double* out, hipStream_t s) {
  const int chains = A * C * J;
  if (chains <= 0 || F <= 0) return 0;
  if (n_back > 3 || n_back < 1 || K < 1 || K > CAND_MAX) return -2;
  VitMulti V{kp, F, C, J, K, n_back, score_thr};
  hipLaunchKernelGGL(viterbi_multi_kernel, dim3(chains), dim3(VM_LANES), 0, s, V, chains, thres_dist,
                     static_cast<int8_t*>(scratch), out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------ triangulate_possible (cameras.py:639-724)
// ransac_kernel for P candidates per camera.  One wave per point; the cameras with a non-NaN candidate
// take part, each with its candidates in ascending k and then "none", so a combination is a mixed-radix
// number whose slowest digit is the first camera (itertools.product order).  Lanes evaluate 64
// combinations at a time; the first chunk holding an error < threshold ends the search at its first
// such combination (the serial early exit), otherwise the first strict minimum below 200 wins.
// Raw and undistorted candidates sit in LDS; a lane gathers its combination into registers.
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
  // DLT over the used cameras whose undistortion succeeded, then the mean reprojection error over the
  // used cameras (CameraGroup.reprojection_error(mean=True): NaN norms dropped, fewer than two -> NaN)
  auto evaluate = [&](unsigned use, unsigned sel, const double (&ux)[MAXC], const double (&uy)[MAXC],
                      double (&p)[3]) -> double {
    unsigned ok = 0;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (((use >> c) & 1u) && !(ux[c] != ux[c])) ok |= 1u << c;
    p[0] = p[1] = p[2] = NAN;
    if (__popc(ok) >= 2) dlt_point<MAXC>(cams, C, ux, uy, ok, p);
    double sum = 0.0, cnt = 0.0;
    for (int c = 0; c < C; ++c) {
      if (!((use >> c) & 1u)) continue;
      const int k = (sel >> (2 * c)) & 3u;
      double u, v;
      cam_project(cam_at(cams, c), p[0], p[1], p[2], u, v);
      const double ex = s_raw[c * CAND_MAX + k][0] - u, ey = s_raw[c * CAND_MAX + k][1] - v;
      const double nr = sqrt(ex * ex + ey * ey);
      if (!(nr != nr)) {
        sum = sum + nr;
        cnt = cnt + 1.0;
      }
    }
    return (cnt < 1.5) ? NAN : sum / cnt;
  };
  int chosen = -1;
  double best_err = 200.0;
  int best_s = 0x7fffffff;
  double ux[MAXC], uy[MAXC];
  if (m >= 2) {
    for (int base = 0; base < nsub; base += 64) {
      const int s = base + lane;
      double err = NAN;
      if (s < nsub) {
        unsigned use, sel;
        gather(s, use, sel, ux, uy);
        const int k = __popc(use);
        if (!(k < min_cams && k != m) && k >= 2) {
          double p[3];
          err = evaluate(use, sel, ux, uy, p);
        }
      }
      // first combination (smallest s) in this chunk with err < threshold
      const bool hit = err < threshold;
      const unsigned long long hits = __ballot(hit);
      if (hits) {
        chosen = base + __ffsll((long long)hits) - 1;
        break;
      }
      // running strict minimum, ties keep the earlier combination
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
    if (chosen < 0 && best_s != 0x7fffffff) chosen = best_s;
  }
  if (lane != 0) return;
  double p[3] = {NAN, NAN, NAN};
  double err = 0.0;
  unsigned use = 0, sel = 0;
  if (chosen >= 0) {
    gather(chosen, use, sel, ux, uy);
    err = evaluate(use, sel, ux, uy, p);
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

}  // namespace mq
