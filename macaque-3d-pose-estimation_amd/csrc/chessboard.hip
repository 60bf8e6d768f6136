// Chessboard-corner detector for gfx950: the reference's cv2.findChessboardCorners + cv2.cornerSubPix
// (multicam_toolbox.py:22-72) as a detector of this project's own.  tests/chessboard_ref.py is the numpy restatement;
// stages 2-5 are integer and equal it exactly, the refinement is float64 without FMA contraction.
//   2. chess_response_kernel   3 x 3 binomial blur + ChESS ring response from one LDS tile (6-pixel halo)
//   3. chess_nms_kernel        9 x 9 maxima; a radix select of the K-th packed key (R << 32 | ~(y w + x), unique per
//      chess_hist / _scan /    pixel) over the survivor map, a gather of the keys at or above it and a bitonic sort:
//      _gather / _sort         the result does not depend on the order in which threads find survivors
//   4-5. chess_grid_kernel     one wave per image runs chessboard_dev.hpp's grid search and canonical order
//   6. corner_subpix_kernel    one wave per corner, all corners of all images in one launch
#include <hip/hip_runtime.h>

#include "chessboard.hpp"
#include "chessboard_dev.hpp"

namespace mq {

namespace {

int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }

// ------------------------------------------------------------------ 2. response
constexpr int RT_W = 64, RT_H = 16;                 // output tile
constexpr int RT_GW = RT_W + 12, RT_GH = RT_H + 12;  // gray tile: halo 6
constexpr int RT_BW = RT_W + 10, RT_BH = RT_H + 10;  // blurred tile: halo 5

__constant__ int8_t RING_DX[16] = {5, 5, 4, 2, 0, -2, -4, -5, -5, -5, -4, -2, 0, 2, 4, 5};
__constant__ int8_t RING_DY[16] = {0, 2, 4, 5, 5, 5, 4, 2, 0, -2, -4, -5, -5, -5, -4, -2};

__global__ __launch_bounds__(256) void chess_response_kernel(const uint8_t* __restrict__ gray, int h, int w,
                                                             int32_t* __restrict__ resp) {
  __shared__ uint8_t g[RT_GH][RT_GW];
  __shared__ uint8_t b[RT_BH][RT_BW + 2];
  const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
  const uint8_t* img = gray + (int64_t)blockIdx.z * h * w;
  for (int e = threadIdx.x; e < RT_GH * RT_GW; e += 256) {
    const int r = e / RT_GW, c = e % RT_GW;
    int yy = y0 + r - 6, xx = x0 + c - 6;
    yy = yy < 0 ? 0 : (yy > h - 1 ? h - 1 : yy);  // replicated border
    xx = xx < 0 ? 0 : (xx > w - 1 ? w - 1 : xx);
    g[r][c] = img[(int64_t)yy * w + xx];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < RT_BH * RT_BW; e += 256) {
    const int r = e / RT_BW, c = e % RT_BW;  // blurred (r, c) is gray (r + 1, c + 1)
    const int top = g[r][c] + 2 * g[r][c + 1] + g[r][c + 2];
    const int mid = g[r + 1][c] + 2 * g[r + 1][c + 1] + g[r + 1][c + 2];
    const int bot = g[r + 2][c] + 2 * g[r + 2][c + 1] + g[r + 2][c + 2];
    b[r][c] = (uint8_t)((top + 2 * mid + bot + 8) >> 4);
  }
  __syncthreads();
  const int tx = threadIdx.x % RT_W, ty = threadIdx.x / RT_W;
  const int x = x0 + tx;
  if (x >= w) return;
  for (int r = ty; r < RT_H; r += 256 / RT_W) {
    const int y = y0 + r;
    if (y >= h) break;
    int out = 0;
    if (x >= 5 && x < w - 5 && y >= 5 && y < h - 5) {
      int I[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) I[k] = b[r + 5 + RING_DY[k]][tx + 5 + RING_DX[k]];
      int SR = 0, DR = 0, S = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) SR += abs(I[k] + I[k + 8] - I[k + 4] - I[k + 12]);
#pragma unroll
      for (int k = 0; k < 8; ++k) DR += abs(I[k] - I[k + 8]);
#pragma unroll
      for (int k = 0; k < 16; ++k) S += I[k];
      const int L = b[r + 5][tx + 5] + b[r + 5][tx + 6] + b[r + 5][tx + 4] + b[r + 6][tx + 5] + b[r + 4][tx + 5];
      out = 5 * SR - 5 * DR - abs(5 * S - 16 * L);
      out = out < 0 ? 0 : out;
    }
    resp[((int64_t)blockIdx.z * h + y) * w + x] = out;
  }
}

// ------------------------------------------------------------------ 3. candidates
constexpr int NT_W = 64, NT_H = 16, NMS_R = 4;
constexpr int NT_TW = NT_W + 2 * NMS_R, NT_TH = NT_H + 2 * NMS_R;

__global__ __launch_bounds__(256) void chess_nms_kernel(const int32_t* __restrict__ resp, int h, int w,
                                                        int32_t* __restrict__ surv) {
  __shared__ int32_t t[NT_TH][NT_TW];
  __shared__ int32_t rm[NT_TH][NT_W];
  const int x0 = blockIdx.x * NT_W, y0 = blockIdx.y * NT_H;
  const int32_t* img = resp + (int64_t)blockIdx.z * h * w;
  for (int e = threadIdx.x; e < NT_TH * NT_TW; e += 256) {
    const int r = e / NT_TW, c = e % NT_TW;
    const int yy = y0 + r - NMS_R, xx = x0 + c - NMS_R;
    t[r][c] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? img[(int64_t)yy * w + xx] : 0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < NT_TH * NT_W; e += 256) {
    const int r = e / NT_W, c = e % NT_W;
    int m = 0;
#pragma unroll
    for (int k = 0; k <= 2 * NMS_R; ++k) m = max(m, t[r][c + k]);
    rm[r][c] = m;
  }
  __syncthreads();
  const int tx = threadIdx.x % NT_W, ty = threadIdx.x / NT_W;
  const int x = x0 + tx;
  if (x >= w) return;
  for (int r = ty; r < NT_H; r += 256 / NT_W) {
    const int y = y0 + r;
    if (y >= h) break;
    int m = 0;
#pragma unroll
    for (int k = 0; k <= 2 * NMS_R; ++k) m = max(m, rm[r + k][tx]);
    const int v = t[r + NMS_R][tx + NMS_R];
    surv[((int64_t)blockIdx.z * h + y) * w + x] = (v > 0 && v == m) ? v : 0;
  }
}

// state of one image's selection
struct SelState {
  unsigned long long prefix;  // the bits of the K-th largest key found so far
  int32_t krem;               // rank of the K-th key among the keys that share the prefix
  int32_t all;                // fewer than K survivors: every one is kept
  int32_t cnt;                // keys gathered
  int32_t pad;
};

__device__ __forceinline__ unsigned long long pack_key(int32_t v, unsigned idx) {
  return ((unsigned long long)(unsigned)v << 32) | (unsigned)(~idx);
}

__global__ void chess_sel_init_kernel(SelState* __restrict__ st, uint32_t* __restrict__ hist, int n, int K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    st[i].prefix = 0;
    st[i].krem = K;
    st[i].all = 0;
    st[i].cnt = 0;
    st[i].pad = 0;
  }
  if (i < n * 256) hist[i] = 0;
}

// histogram of byte `pass` (0 = most significant) of the keys that share the prefix above it
__global__ __launch_bounds__(256) void chess_hist_kernel(const int32_t* __restrict__ surv, int64_t hw, int pass,
                                                         const SelState* __restrict__ st,
                                                         uint32_t* __restrict__ hist) {
  __shared__ uint32_t lh[256];
  const int img = blockIdx.y;
  if (st[img].all) return;
  lh[threadIdx.x] = 0;
  __syncthreads();
  const int shift = 56 - 8 * pass;
  const unsigned long long prefix = st[img].prefix;
  const int32_t* s = surv + (int64_t)img * hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    const int32_t v = s[i];
    if (v <= 0) continue;
    const unsigned long long key = pack_key(v, (unsigned)i);
    if (pass > 0 && (key >> (shift + 8)) != (prefix >> (shift + 8))) continue;
    atomicAdd(&lh[(key >> shift) & 255], 1u);
  }
  __syncthreads();
  const uint32_t c = lh[threadIdx.x];
  if (c) atomicAdd(&hist[img * 256 + threadIdx.x], c);
}

// walks the histogram from the top: the bin that holds the K-th key extends the prefix
__global__ __launch_bounds__(256) void chess_scan_kernel(SelState* __restrict__ st, uint32_t* __restrict__ hist,
                                                         int pass) {
  const int img = blockIdx.x;
  uint32_t* hh = hist + img * 256;
  if (threadIdx.x == 0 && !st[img].all) {
    const int shift = 56 - 8 * pass;
    int64_t cum = 0;
    const int64_t krem = st[img].krem;
    int bin = -1;
    for (int b = 255; b >= 0; --b) {
      const int64_t c = hh[b];
      if (cum + c >= krem) {
        bin = b;
        break;
      }
      cum += c;
    }
    if (bin < 0) {
      st[img].all = 1;
    } else {
      st[img].prefix |= (unsigned long long)bin << shift;
      st[img].krem = (int32_t)(krem - cum);
    }
  }
  __syncthreads();
  hh[threadIdx.x] = 0;
}

__global__ __launch_bounds__(256) void chess_gather_kernel(const int32_t* __restrict__ surv, int64_t hw,
                                                           SelState* __restrict__ st,
                                                           unsigned long long* __restrict__ keys, int kpad) {
  const int img = blockIdx.y;
  const bool all = st[img].all != 0;
  const unsigned long long thr = st[img].prefix;
  const int32_t* s = surv + (int64_t)img * hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    const int32_t v = s[i];
    if (v <= 0) continue;
    const unsigned long long key = pack_key(v, (unsigned)i);
    if (!all && key < thr) continue;
    const int slot = atomicAdd(&st[img].cnt, 1);
    if (slot >= 0 && slot < kpad) keys[(int64_t)img * kpad + slot] = key;  // exactly K keys pass, or fewer
  }
}

// bitonic sort of at most K unique keys, descending; writes positions, responses and the count
__global__ __launch_bounds__(256) void chess_sort_kernel(const unsigned long long* __restrict__ keys,
                                                         const SelState* __restrict__ st, int K, int kpad, int w,
                                                         int32_t* __restrict__ pos, int32_t* __restrict__ val,
                                                         int32_t* __restrict__ count) {
  __shared__ unsigned long long k[CB_MAX_K];
  const int img = blockIdx.x;
  int cnt = st[img].cnt;
  cnt = cnt < 0 ? 0 : (cnt > K ? K : cnt);
  for (int i = threadIdx.x; i < kpad; i += 256) k[i] = i < cnt ? keys[(int64_t)img * kpad + i] : 0ull;
  __syncthreads();
  for (int size = 2; size <= kpad; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < kpad; i += 256) {
        const int j = i ^ stride;
        if (j > i) {
          const bool desc = (i & size) == 0;
          const unsigned long long a = k[i], b = k[j];
          if (desc ? a < b : a > b) {
            k[i] = b;
            k[j] = a;
          }
        }
      }
      __syncthreads();
    }
  for (int i = threadIdx.x; i < K; i += 256) {
    int32_t x = 0, y = 0, v = 0;
    if (i < cnt) {
      const unsigned idx = ~(unsigned)(k[i] & 0xffffffffull);
      x = (int32_t)(idx % (unsigned)w);
      y = (int32_t)(idx / (unsigned)w);
      v = (int32_t)(k[i] >> 32);
    }
    pos[((int64_t)img * K + i) * 2] = x;
    pos[((int64_t)img * K + i) * 2 + 1] = y;
    val[(int64_t)img * K + i] = v;
  }
  if (threadIdx.x == 0) count[img] = cnt;
}

int next_pow2(int v) {
  int p = 2;
  while (p < v) p <<= 1;
  return p;
}

// ------------------------------------------------------------------ 4-5. grid
__global__ __launch_bounds__(CB_LANES) void chess_grid_kernel(const int32_t* __restrict__ pos,
                                                              const int32_t* __restrict__ val,
                                                              const int32_t* __restrict__ count, int K, double scale,
                                                              int32_t* __restrict__ found, double* __restrict__ corners,
                                                              int32_t* __restrict__ idx) {
  __shared__ int32_t p[2 * CB_MAX_K];
  __shared__ int32_t order[CB_NC];
  __shared__ CbGrid g;
  const int img = blockIdx.x;
  int n = count[img];
  n = n < 0 ? 0 : (n > K ? K : n);
  n = n > CB_MAX_K ? CB_MAX_K : n;
  for (int i = threadIdx.x; i < 2 * n; i += CB_LANES) p[i] = pos[(int64_t)img * K * 2 + i];
  __syncthreads();
  const int seed = cb_find_grid(p, val + (int64_t)img * K, n, g, order);
  __syncthreads();
  if (threadIdx.x == 0) found[img] = seed >= 0 ? 1 : 0;
  for (int i = threadIdx.x; i < CB_NC; i += CB_LANES) {
    const int c = seed >= 0 ? order[i] : -1;
    const bool ok = c >= 0 && c < n;
    corners[((int64_t)img * CB_NC + i) * 2] = ok ? cb_full_res(p[2 * c], scale) : __builtin_nan("");
    corners[((int64_t)img * CB_NC + i) * 2 + 1] = ok ? cb_full_res(p[2 * c + 1], scale) : __builtin_nan("");
    if (idx) idx[(int64_t)img * CB_NC + i] = ok ? c : -1;
  }
}

// ------------------------------------------------------------------ 6. cornerSubPix
__global__ __launch_bounds__(CB_LANES) void corner_subpix_kernel(const uint8_t* __restrict__ gray, int h, int w,
                                                                 double* __restrict__ corners, int per_img,
                                                                 const int32_t* __restrict__ found, int win,
                                                                 int max_iter, double eps) {
  constexpr int PS_MAX = 2 * CB_MAX_WIN + 3;
  __shared__ double patch[PS_MAX * PS_MAX];
  __shared__ double wt[2 * CB_MAX_WIN + 1];
  const int64_t pt = blockIdx.x;
  const int img = (int)(pt / per_img);
  const int lane = threadIdx.x;
  double* out = corners + pt * 2;
  if (found && !found[img]) {
    if (lane == 0) out[0] = out[1] = __builtin_nan("");
    return;
  }
  const double x0 = out[0], y0 = out[1];
  if (!(x0 == x0 && y0 == y0)) return;
  const uint8_t* im = gray + (int64_t)img * h * w;
  for (int k = lane; k <= 2 * win; k += CB_LANES) {
    const double t = (double)(k - win) / (double)win;
    wt[k] = exp(-(t * t));
  }
  const int ps = 2 * win + 3;
  double x = x0, y = y0;
  for (int it = 0; it < (max_iter > 1 ? max_iter : 1); ++it) {
    int ix, iy;
    double fx, fy;
    if (!cb_patch_origin(x, y, ps, ix, iy, fx, fy)) break;
    __syncthreads();  // the previous iteration's reads of patch are done
    for (int e = lane; e < ps * ps; e += CB_LANES) patch[e] = cb_patch_sample(im, h, w, ix, iy, fx, fy, ps, e);
    __syncthreads();
    double acc[5];
    cb_subpix_partial(patch, wt, win, lane, acc);
#pragma unroll
    for (int k = 0; k < 5; ++k)
      for (int o = CB_LANES / 2; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, CB_LANES);
    if (cb_subpix_step(acc, eps * eps, w, h, x, y)) break;
  }
  cb_subpix_finish(x0, y0, win, x, y);
  if (lane == 0) {
    out[0] = x;
    out[1] = y;
  }
}

}  // namespace

ChessCandBufs chess_candidates_layout(Carver& c, int n, int h, int w, int K) {
  const size_t nn = (size_t)(n > 0 ? n : 0);
  ChessCandBufs b;
  b.surv = c.take<int32_t>(nn * (size_t)h * (size_t)w);
  b.hist = c.take<uint32_t>(nn * 256);
  b.st = c.take<SelState>(nn);
  b.keys = c.take<unsigned long long>(nn * (size_t)next_pow2(K));
  return b;
}

size_t chess_candidates_ws_bytes(int n, int h, int w, int K) { return measure(chess_candidates_layout, n, h, w, K); }

int chess_response(const uint8_t* gray, int n, int h, int w, int32_t* resp, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(chess_response_kernel, dim3((w + RT_W - 1) / RT_W, (h + RT_H - 1) / RT_H, n), dim3(256), 0, s,
                     gray, h, w, resp);
  return launched();
}

int chess_candidates(const int32_t* resp, int n, int h, int w, int K, int32_t* pos, int32_t* val, int32_t* count,
                     const ChessCandBufs& b, hipStream_t s) {
  if (n <= 0) return 0;
  if (K < 1 || K > CB_MAX_K || (int64_t)h * w >= ((int64_t)1 << 31)) return -1;
  const int64_t hw = (int64_t)h * w;
  const int kpad = next_pow2(K);
  int32_t* surv = b.surv;
  uint32_t* hist = b.hist;
  SelState* st = static_cast<SelState*>(b.st);
  unsigned long long* keys = b.keys;
  hipLaunchKernelGGL(chess_nms_kernel, dim3((w + NT_W - 1) / NT_W, (h + NT_H - 1) / NT_H, n), dim3(256), 0, s, resp,
                     h, w, surv);
  hipLaunchKernelGGL(chess_sel_init_kernel, dim3(n), dim3(256), 0, s, st, hist, n, K);
  int nb = (int)((hw + 4095) / 4096);
  nb = nb < 1 ? 1 : (nb > 256 ? 256 : nb);
  for (int pass = 0; pass < 8; ++pass) {
    hipLaunchKernelGGL(chess_hist_kernel, dim3(nb, n), dim3(256), 0, s, surv, hw, pass, st, hist);
    hipLaunchKernelGGL(chess_scan_kernel, dim3(n), dim3(256), 0, s, st, hist, pass);
  }
  hipLaunchKernelGGL(chess_gather_kernel, dim3(nb, n), dim3(256), 0, s, surv, hw, st, keys, kpad);
  hipLaunchKernelGGL(chess_sort_kernel, dim3(n), dim3(256), 0, s, keys, st, K, kpad, w, pos, val, count);
  return launched();
}

int chess_grid(const int32_t* pos, const int32_t* val, const int32_t* count, int n, int K, double scale,
               int32_t* found, double* corners, int32_t* idx, hipStream_t s) {
  if (n <= 0) return 0;
  if (K < 1 || K > CB_MAX_K) return -1;
  hipLaunchKernelGGL(chess_grid_kernel, dim3(n), dim3(CB_LANES), 0, s, pos, val, count, K, scale, found, corners,
                     idx);
  return launched();
}

int corner_subpix(const uint8_t* gray, int n, int h, int w, double* corners, int per_img, const int32_t* found,
                  int win, int max_iter, double eps, hipStream_t s) {
  if (n <= 0 || per_img <= 0) return 0;
  if (win < 1 || win > CB_MAX_WIN) return -1;
  hipLaunchKernelGGL(corner_subpix_kernel, dim3((unsigned)((int64_t)n * per_img)), dim3(CB_LANES), 0, s, gray, h, w,
                     corners, per_img, found, win, max_iter, eps);
  return launched();
}

}  // namespace mq
