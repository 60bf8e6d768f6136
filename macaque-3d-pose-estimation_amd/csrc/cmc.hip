// Camera-motion compensation for BoT-SORT on the GPU: boxmot 12.0.7 cmc/sift.py SIFT.apply restated stage by
// stage (gray + resize, mask, SIFT detect + describe as cv2.SIFT_create(nOctaveLayers=3, contrastThreshold=0.02,
// edgeThreshold=20), brute-force 2-NN match + boxmot's gates, 2-point RANSAC partial affine).  Compiled with
// -ffp-contract=off: every float32 / float64 step follows the operation order of tests/cmc_ref.py, the numpy
// restatement the tests compare against.  Histogram sums (orientation, descriptor) are 2^-20 fixed-point integer
// atomics in LDS, so they do not depend on arrival order; keypoint order comes from a flag map + scan and a
// rank sort, never from an atomic counter.  Every index is checked against the image size and the caps.
#include "cmc.hpp"

#include <cmath>
#include <cstring>

#include "common.hpp"

namespace mq {

namespace {

constexpr int N_LAYERS = 3;
constexpr int BORDER = 5;
constexpr float FIXF = 1048576.f;
constexpr float PREFILTER = (float)(0.5 * 0.02 / 3 * 255);
constexpr int MAX_TAPS = 31;
constexpr float INVALID_OCT = -100.f;

struct GaussK {
  int r;
  float k[MAX_TAPS];
};

GaussK make_gauss(double sigma) {
  GaussK g;
  int k = ((int)std::nearbyint(sigma * 8 + 1)) | 1;
  if (k > MAX_TAPS) k = MAX_TAPS;
  g.r = (k - 1) / 2;
  double w[MAX_TAPS], sum = 0.0;
  for (int i = 0; i < k; ++i) {
    const double d = (double)(i - g.r);
    w[i] = std::exp(-(d * d) / (2.0 * sigma * sigma));
    sum += w[i];
  }
  for (int i = 0; i < MAX_TAPS; ++i) g.k[i] = i < k ? (float)(w[i] / sum) : 0.f;
  return g;
}

__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  const int m = 2 * n - 2;
  i %= m;
  if (i < 0) i += m;
  return i >= n ? m - i : i;
}

// ------------------------------------------------------------------ 1. gray + resize
// cv2 resize taps for uint8 INTER_LINEAR: 11-bit weights, clamped edges
__device__ __forceinline__ void resize_taps(int d, int src, double inv_scale, int& s0, int& s1, int& a0, int& a1) {
  float fx = (float)(((double)d + 0.5) * inv_scale - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) {
    fx = 0.f;
    sx = 0;
  }
  if (sx >= src - 1) {
    fx = 0.f;
    sx = src - 1;
  }
  s0 = sx;
  s1 = sx + 1 < src ? sx + 1 : src - 1;
  a0 = (int)rintf((1.f - fx) * 2048.f);
  a1 = (int)rintf(fx * 2048.f);
}

__global__ void cmc_gray_resize_kernel(const uint8_t* __restrict__ frames, int64_t fstride, int H, int W, int h, int w,
                                       double inv_scale, uint8_t* __restrict__ out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y, n = blockIdx.z;
  if (x >= w || y >= h) return;
  int x0, x1, a0, a1, y0, y1, b0, b1;
  resize_taps(x, W, inv_scale, x0, x1, a0, a1);
  resize_taps(y, H, inv_scale, y0, y1, b0, b1);
  const uint8_t* img = frames + (int64_t)n * fstride;
  auto gray = [&](int yy, int xx) {
    const uint8_t* p = img + ((int64_t)yy * W + xx) * 3;
    return (p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + 8192) >> 14;
  };
  const int r0 = gray(y0, x0) * a0 + gray(y0, x1) * a1;
  const int r1 = gray(y1, x0) * a0 + gray(y1, x1) * a1;
  int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
  v = v < 0 ? 0 : (v > 255 ? 255 : v);
  out[((int64_t)n * h + y) * w + x] = (uint8_t)v;
}

// ------------------------------------------------------------------ 2. mask
__device__ __forceinline__ int scaled_int(double v, double scale, int hi) {
  double t = v * scale;
  if (!(t > -1e9)) t = -1e9;  // NaN too
  if (t > 1e9) t = 1e9;
  const int i = (int)t;  // truncation toward zero
  return i < 0 ? 0 : (i > hi ? hi : i);
}

__global__ void cmc_mask_kernel(const double* __restrict__ boxes, const int32_t* __restrict__ box_counts, int max_boxes,
                                int h, int w, double scale, uint8_t* __restrict__ mask) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y, n = blockIdx.z;
  if (x >= w || y >= h) return;
  const int ry0 = (int)(0.02 * (double)h), ry1 = (int)(0.98 * (double)h);
  const int rx0 = (int)(0.02 * (double)w), rx1 = (int)(0.98 * (double)w);
  uint8_t v = (y >= ry0 && y < ry1 && x >= rx0 && x < rx1) ? 255 : 0;
  int nb = box_counts ? box_counts[n] : 0;
  nb = nb < 0 ? 0 : (nb > max_boxes ? max_boxes : nb);
  for (int b = 0; b < nb && v; ++b) {
    const double* bb = boxes + ((int64_t)n * max_boxes + b) * 4;
    const int x1 = scaled_int(bb[0], scale, w), y1 = scaled_int(bb[1], scale, h);
    const int x2 = scaled_int(bb[2], scale, w), y2 = scaled_int(bb[3], scale, h);
    if (y >= y1 && y < y2 && x >= x1 && x < x2) v = 0;
  }
  mask[((int64_t)n * h + y) * w + x] = v;
}

// ------------------------------------------------------------------ 3. pyramid
// uint8 -> float32, with cv2's 2x INTER_LINEAR upsample when `up`
__global__ void sift_base_kernel(const uint8_t* __restrict__ gray, int h, int w, int up, float* __restrict__ out,
                                 int64_t out_stride) {
  const int bw = up ? 2 * w : w, bh = up ? 2 * h : h;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y, n = blockIdx.z;
  if (x >= bw || y >= bh) return;
  const uint8_t* img = gray + (int64_t)n * h * w;
  float v;
  if (!up) {
    v = (float)img[y * w + x];
  } else {
    auto taps = [](int d, int src, int& s0, int& s1, float& a0, float& a1) {
      float fx = (float)(((double)d + 0.5) * 0.5 - 0.5);
      int sx = (int)floorf(fx);
      fx -= (float)sx;
      if (sx < 0) {
        fx = 0.f;
        sx = 0;
      }
      if (sx >= src - 1) {
        fx = 0.f;
        sx = src - 1;
      }
      s0 = sx;
      s1 = sx + 1 < src ? sx + 1 : src - 1;
      a0 = 1.f - fx;
      a1 = fx;
    };
    int x0, x1, y0, y1;
    float a0, a1, b0, b1;
    taps(x, w, x0, x1, a0, a1);
    taps(y, h, y0, y1, b0, b1);
    const float r0 = (float)img[y0 * w + x0] * a0 + (float)img[y0 * w + x1] * a1;
    const float r1 = (float)img[y1 * w + x0] * a0 + (float)img[y1 * w + x1] * a1;
    v = r0 * b0 + r1 * b1;
  }
  out[(int64_t)n * out_stride + (int64_t)y * bw + x] = v;
}

// Separable Gaussian, BORDER_REFLECT_101, rows first, taps accumulated in ascending order.  One block per
// 16 x 64 output tile: the input tile with its halo and the row-filtered rows live in LDS.
constexpr int BT_H = 16, BT_W = 64, BR_MAX = (MAX_TAPS - 1) / 2;
__global__ __launch_bounds__(256) void sift_blur_kernel(const float* __restrict__ in, int64_t in_stride,
                                                        float* __restrict__ out, int64_t out_stride, int h, int w,
                                                        GaussK g) {
  __shared__ float tile[(BT_H + 2 * BR_MAX) * (BT_W + 2 * BR_MAX)];
  __shared__ float mid[(BT_H + 2 * BR_MAX) * BT_W];
  const int R = g.r, TW = BT_W + 2 * R, TH = BT_H + 2 * R;
  const int x0 = blockIdx.x * BT_W, y0 = blockIdx.y * BT_H, n = blockIdx.z;
  const float* src = in + (int64_t)n * in_stride;
  for (int i = threadIdx.x; i < TH * TW; i += blockDim.x) {
    const int ly = i / TW, lx = i - ly * TW;
    tile[i] = src[(int64_t)reflect101(y0 + ly - R, h) * w + reflect101(x0 + lx - R, w)];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TH * BT_W; i += blockDim.x) {
    const int ly = i / BT_W, lx = i - ly * BT_W;
    const float* p = tile + ly * TW + lx;
    float acc = g.k[0] * p[0];
    for (int t = 1; t <= 2 * R; ++t) acc = acc + g.k[t] * p[t];
    mid[i] = acc;
  }
  __syncthreads();
  float* dst = out + (int64_t)n * out_stride;
  for (int i = threadIdx.x; i < BT_H * BT_W; i += blockDim.x) {
    const int ly = i / BT_W, lx = i - ly * BT_W;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= h || x >= w) continue;
    float acc = g.k[0] * mid[ly * BT_W + lx];
    for (int t = 1; t <= 2 * R; ++t) acc = acc + g.k[t] * mid[(ly + t) * BT_W + lx];
    dst[(int64_t)y * w + x] = acc;
  }
}

// next octave's first layer: pixel (2y, 2x) of layer N_LAYERS
__global__ void sift_decimate_kernel(const float* __restrict__ in, int ih, int iw, float* __restrict__ out, int oh,
                                     int ow, int64_t stride) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y, n = blockIdx.z;
  if (x >= ow || y >= oh) return;
  const int sy = 2 * y < ih ? 2 * y : ih - 1, sx = 2 * x < iw ? 2 * x : iw - 1;
  out[(int64_t)n * stride + (int64_t)y * ow + x] = in[(int64_t)n * stride + (int64_t)sy * iw + sx];
}

__global__ void sift_dog_kernel(const float* __restrict__ gauss, float* __restrict__ dog, int plane, int64_t stride) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = blockIdx.z;
  if (i >= 5 * plane) return;
  const float* g = gauss + (int64_t)n * stride;
  dog[(int64_t)n * stride + i] = g[i + plane] - g[i];
}

// 26-neighbour extrema of DoG layers 1..3 (ties pass, |v| > PREFILTER): one flag byte per pixel
__global__ void sift_extrema_kernel(const float* __restrict__ dog, int64_t stride, int h, int w,
                                    uint8_t* __restrict__ flags, int64_t fstride) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y % h, layer = 1 + blockIdx.y / h, n = blockIdx.z;
  if (layer > N_LAYERS || c < BORDER || c >= w - BORDER || r < BORDER || r >= h - BORDER) return;
  const float* d = dog + (int64_t)n * stride;
  const int plane = h * w;
  const float v = d[layer * plane + r * w + c];
  if (!(fabsf(v) > PREFILTER)) return;
  bool is_max = v > 0.f, is_min = v < 0.f;
  for (int dl = -1; dl <= 1; ++dl)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        if (dl == 0 && dy == 0 && dx == 0) continue;
        const float nb = d[(layer + dl) * plane + (r + dy) * w + (c + dx)];
        is_max = is_max && v >= nb;
        is_min = is_min && v <= nb;
      }
  if (is_max || is_min) flags[(int64_t)n * fstride + (layer - 1) * plane + r * w + c] = 1;
}

// flag map -> candidate list in scan order: each thread counts a contiguous chunk, block scan, ordered write
__global__ __launch_bounds__(1024) void sift_compact_kernel(const uint8_t* __restrict__ flags, int total,
                                                            int32_t* __restrict__ cand, int32_t* __restrict__ cand_cnt) {
  __shared__ int cnt[1024];
  const int n = blockIdx.x, t = threadIdx.x;
  const uint8_t* f = flags + (int64_t)n * total;
  const int chunk = (total + 1023) / 1024;
  const int lo = t * chunk < total ? t * chunk : total;
  const int hi = lo + chunk < total ? lo + chunk : total;
  int c = 0;
  for (int i = lo; i < hi; ++i) c += f[i] != 0;
  cnt[t] = c;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = t >= o ? cnt[t - o] : 0;
    __syncthreads();
    cnt[t] += v;
    __syncthreads();
  }
  int pos = cnt[t] - c;
  for (int i = lo; i < hi && pos < CMC_KCAND; ++i)
    if (f[i]) cand[(int64_t)n * CMC_KCAND + pos++] = i;
  if (t == 1023) cand_cnt[n] = cnt[t] < CMC_KCAND ? cnt[t] : CMC_KCAND;
}

// One wave per candidate: cv2 adjustLocalExtrema (every lane computes the same refinement), the mask test,
// then calcOrientationHist over the wave with the 36-bin histogram in LDS, one output slot per peak.
__global__ __launch_bounds__(64) void sift_orient_kernel(const float* __restrict__ pyr, SiftGeom g,
                                                         const int32_t* __restrict__ cand,
                                                         const int32_t* __restrict__ cand_cnt,
                                                         const uint8_t* __restrict__ mask, float* __restrict__ slots) {
  __shared__ unsigned long long acc[36];
  __shared__ float tmp[36], hist[36];
  const int ci = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
  float* out = slots + ((int64_t)n * CMC_KCAND + ci) * CMC_MAXPEAK * CMC_KP;
  bool ok = ci < cand_cnt[n];
  int o = 0, layer = 1, r = 0, c = 0, h = 1, w = 1;
  float xc = 0.f, xr = 0.f, xi = 0.f, contr = 0.f;
  const float* arena = pyr + (int64_t)n * g.arena;
  if (ok) {
    int idx = cand[(int64_t)n * CMC_KCAND + ci];
    ok = idx >= 0 && idx < g.f_off[g.n_oct];
    if (ok) {
      while (o + 1 < g.n_oct && idx >= g.f_off[o + 1]) ++o;
      idx -= g.f_off[o];
      h = g.h[o];
      w = g.w[o];
      layer = 1 + idx / (h * w);
      r = (idx % (h * w)) / w;
      c = idx % w;
      ok = layer <= N_LAYERS && c >= BORDER && c < w - BORDER && r >= BORDER && r < h - BORDER;
    }
  }
  if (ok) {
    const float* dog = arena + g.d_off[o];
    const int plane = h * w;
    const float img_scale = 1.f / 255.f, deriv = img_scale * 0.5f, cross = img_scale * 0.25f;
    float g0 = 0, g1 = 0, g2 = 0, dxx = 0, dyy = 0, dxy = 0;
    int it = 0;
    for (; it < 5; ++it) {
      const float* m = dog + layer * plane;
      const float* p = m - plane;
      const float* q = m + plane;
      const int i0 = r * w + c;
      g0 = (m[i0 + 1] - m[i0 - 1]) * deriv;
      g1 = (m[i0 + w] - m[i0 - w]) * deriv;
      g2 = (q[i0] - p[i0]) * deriv;
      const float v2 = m[i0] * 2.f;
      dxx = (m[i0 + 1] + m[i0 - 1] - v2) * img_scale;
      dyy = (m[i0 + w] + m[i0 - w] - v2) * img_scale;
      const float dss = (q[i0] + p[i0] - v2) * img_scale;
      dxy = (m[i0 + w + 1] - m[i0 + w - 1] - m[i0 - w + 1] + m[i0 - w - 1]) * cross;
      const float dxs = (q[i0 + 1] - q[i0 - 1] - p[i0 + 1] + p[i0 - 1]) * cross;
      const float dys = (q[i0 + w] - q[i0 - w] - p[i0 + w] + p[i0 - w]) * cross;
      const float c00 = dyy * dss - dys * dys;
      const float c01 = dxs * dys - dxy * dss;
      const float c02 = dxy * dys - dxs * dyy;
      const float det = dxx * c00 + dxy * c01 + dxs * c02;
      if (!(det != 0.f) || !isfinite(det)) {
        ok = false;
        break;
      }
      const float c11 = dxx * dss - dxs * dxs;
      const float c12 = dxy * dxs - dxx * dys;
      const float c22 = dxx * dyy - dxy * dxy;
      xc = -((c00 * g0 + c01 * g1 + c02 * g2) / det);
      xr = -((c01 * g0 + c11 * g1 + c12 * g2) / det);
      xi = -((c02 * g0 + c12 * g1 + c22 * g2) / det);
      if (!(isfinite(xc) && isfinite(xr) && isfinite(xi))) {
        ok = false;
        break;
      }
      if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) break;
      if (fmaxf(fabsf(xi), fmaxf(fabsf(xr), fabsf(xc))) > (float)(2147483647 / 3)) {
        ok = false;
        break;
      }
      c += (int)rintf(xc);
      r += (int)rintf(xr);
      layer += (int)rintf(xi);
      if (layer < 1 || layer > N_LAYERS || c < BORDER || c >= w - BORDER || r < BORDER || r >= h - BORDER) {
        ok = false;
        break;
      }
    }
    if (it >= 5) ok = false;
    if (ok) {
      const float t = g0 * xc + g1 * xr + g2 * xi;
      contr = dog[layer * plane + r * w + c] * img_scale + t * 0.5f;
      if (fabsf(contr) * (float)N_LAYERS < 0.02f) ok = false;
      const float tr = dxx + dyy, det2 = dxx * dyy - dxy * dxy;
      const float lhs = tr * tr * 20.f, rhs = (20.f + 1.f) * (20.f + 1.f) * det2;
      if (det2 <= 0.f || lhs >= rhs) ok = false;
    }
  }
  float x = 0, y = 0, size = 0, scl = 0;
  if (ok) {
    const float osc = (float)(1 << o);
    x = ((float)c + xc) * osc;
    y = ((float)r + xr) * osc;
    size = 1.6f * exp2f(((float)layer + xi) / (float)N_LAYERS) * osc * 2.f;
    scl = size * 0.5f / osc;
    if (g.first_octave < 0) {
      x *= 0.5f;
      y *= 0.5f;
      size *= 0.5f;
    }
    const float px = rintf(x), py = rintf(y);
    if (!(px >= 0.f && px < (float)g.img_w && py >= 0.f && py < (float)g.img_h))
      ok = false;
    else if (mask && mask[((int64_t)n * g.img_h + (int)py) * g.img_w + (int)px] == 0)
      ok = false;
  }
  if (!ok) {  // uniform over the wave
    if (lane < CMC_MAXPEAK) out[lane * CMC_KP + 4] = INVALID_OCT;
    return;
  }
  const float* img = arena + g.g_off[o] + layer * h * w;
  int radius = (int)rintf(4.5f * scl);
  radius = radius > 64 ? 64 : radius;
  const float sigma = 1.5f * scl;
  const float escale = -1.f / (2.f * sigma * sigma);
  if (lane < 36) acc[lane] = 0ull;
  __syncthreads();
  const int side = 2 * radius + 1;
  for (int s = lane; s < side * side; s += 64) {
    const int i = s / side - radius, j = s % side - radius;
    const int yy = r + i, xx = c + j;
    if (yy <= 0 || yy >= h - 1 || xx <= 0 || xx >= w - 1) continue;
    const float dx = img[yy * w + xx + 1] - img[yy * w + xx - 1];
    const float dy = img[(yy - 1) * w + xx] - img[(yy + 1) * w + xx];
    const float wgt = expf((float)(i * i + j * j) * escale);
    float ori = atan2f(dy, dx) * 57.29577951308232f;
    if (ori < 0.f) ori = ori + 360.f;
    const float mag = sqrtf(dx * dx + dy * dy);
    int b = (int)rintf(0.1f * ori);
    if (b >= 36) b -= 36;
    if (b < 0) b += 36;
    b = b < 0 ? 0 : (b > 35 ? 35 : b);
    atomicAdd(&acc[b], (unsigned long long)llrintf((wgt * mag) * FIXF));
  }
  __syncthreads();
  if (lane < 36) tmp[lane] = (float)(long long)acc[lane] * (1.f / FIXF);
  __syncthreads();
  if (lane < 36) {
    const int j = lane;
    hist[j] = (tmp[(j + 34) % 36] + tmp[(j + 2) % 36]) * (1.f / 16.f) +
              (tmp[(j + 35) % 36] + tmp[(j + 1) % 36]) * (4.f / 16.f) + tmp[j] * (6.f / 16.f);
  }
  __syncthreads();
  float mx = hist[0];
  for (int j = 1; j < 36; ++j) mx = fmaxf(mx, hist[j]);
  const float thr = mx * 0.8f;
  bool pk = false;
  float hl = 0, hr = 0, hj = 0;
  if (lane < 36) {
    hl = hist[(lane + 35) % 36];
    hr = hist[(lane + 1) % 36];
    hj = hist[lane];
    pk = hj > hl && hj > hr && hj >= thr;
  }
  const unsigned long long pm = __ballot(pk);
  const int rank = __popcll(pm & ((1ull << lane) - 1ull));
  const int npk = __popcll(pm);
  if (pk && rank < CMC_MAXPEAK) {
    float b = (float)lane + 0.5f * (hl - hr) / (hl - 2.f * hj + hr);
    b = b < 0.f ? b + 36.f : (b >= 36.f ? b - 36.f : b);
    float ang = 360.f - 10.f * b;
    if (fabsf(ang - 360.f) < 1.1920929e-07f) ang = 0.f;
    float* kp = out + rank * CMC_KP;
    kp[0] = x;
    kp[1] = y;
    kp[2] = size;
    kp[3] = ang;
    kp[4] = (float)(o + g.first_octave);
    kp[5] = (float)layer;
    kp[6] = fabsf(contr);
  }
  if (lane < CMC_MAXPEAK && lane >= npk) out[lane * CMC_KP + 4] = INVALID_OCT;
}

// Rank sort of the valid slots by (octave, layer, y, x, angle), ties by slot: rank < max_kp is written out.
__device__ __forceinline__ bool kp_less(const float* a, int ia, const float* b, int ib) {
  if (a[4] != b[4]) return a[4] < b[4];
  if (a[5] != b[5]) return a[5] < b[5];
  if (a[1] != b[1]) return a[1] < b[1];
  if (a[0] != b[0]) return a[0] < b[0];
  if (a[3] != b[3]) return a[3] < b[3];
  return ia < ib;
}

__global__ __launch_bounds__(256) void sift_sort_kernel(const float* __restrict__ slots,
                                                        const int32_t* __restrict__ cand_cnt, int max_kp,
                                                        float* __restrict__ kps, int32_t* __restrict__ counts) {
  __shared__ float key[256 * 5];
  const int n = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  // only the slots of the image's candidates can be valid: the rest of the CMC_KCAND * CMC_MAXPEAK are skipped
  int nc = cand_cnt[n];
  nc = nc < 0 ? 0 : (nc > CMC_KCAND ? CMC_KCAND : nc);
  const int NS = (nc * CMC_MAXPEAK + 255) / 256 * 256;  // <= CMC_KCAND * CMC_MAXPEAK, a multiple of the tile
  if ((int)blockIdx.x * 256 >= NS) return;
  const float* base = slots + (int64_t)n * CMC_KCAND * CMC_MAXPEAK * CMC_KP;
  float me[CMC_KP];
  for (int k = 0; k < CMC_KP; ++k) me[k] = base[(int64_t)i * CMC_KP + k];
  const bool valid = me[4] != INVALID_OCT;
  int rank = 0;
  for (int t0 = 0; t0 < NS; t0 += 256) {
    const float* p = base + (int64_t)(t0 + threadIdx.x) * CMC_KP;
    __syncthreads();
    key[threadIdx.x * 5 + 0] = p[0];
    key[threadIdx.x * 5 + 1] = p[1];
    key[threadIdx.x * 5 + 2] = p[3];
    key[threadIdx.x * 5 + 3] = p[4];
    key[threadIdx.x * 5 + 4] = p[5];
    __syncthreads();
    if (!valid) continue;
    for (int j = 0; j < 256; ++j) {
      const float* q = key + j * 5;
      if (q[3] == INVALID_OCT) continue;
      const float other[CMC_KP] = {q[0], q[1], 0.f, q[2], q[3], q[4], 0.f};
      rank += kp_less(other, t0 + j, me, i) ? 1 : 0;
    }
  }
  if (valid && rank < max_kp) {
    float* dst = kps + ((int64_t)n * max_kp + rank) * CMC_KP;
    for (int k = 0; k < CMC_KP; ++k) dst[k] = me[k];
    atomicMax(&counts[n], rank + 1);
  }
}

// ------------------------------------------------------------------ descriptor
// cv2 calcSIFTDescriptor (d = 4, n = 8): one wave per keypoint, the (d+2)(d+2)(n+2) histogram in LDS.
__global__ __launch_bounds__(64) void sift_describe_kernel(const float* __restrict__ pyr, SiftGeom g,
                                                           const float* __restrict__ kps,
                                                           const int32_t* __restrict__ counts, int max_kp,
                                                           uint8_t* __restrict__ desc) {
  constexpr int D = 4, NB = 8, HL = (D + 2) * (D + 2) * (NB + 2);
  __shared__ unsigned long long hist[HL];
  const int k = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
  int cnt = counts[n];
  cnt = cnt < 0 ? 0 : (cnt > max_kp ? max_kp : cnt);
  if (k >= cnt) return;
  const float* kp = kps + ((int64_t)n * max_kp + k) * CMC_KP;
  uint8_t* out = desc + ((int64_t)n * max_kp + k) * 128;
  const int octave = (int)fminf(fmaxf(kp[4], -64.f), 64.f), layer = (int)fminf(fmaxf(kp[5], -1.f), 64.f);
  const int oi = octave - g.first_octave;
  bool ok = oi >= 0 && oi < g.n_oct && layer >= 0 && layer <= N_LAYERS + 2 && isfinite(kp[0]) && isfinite(kp[1]) &&
            isfinite(kp[2]) && isfinite(kp[3]) && kp[2] > 0.f;
  const float sc = ok ? (octave >= 0 ? 1.f / (float)(1 << octave) : (float)(1 << -octave)) : 1.f;
  const float ptx = kp[0] * sc, pty = kp[1] * sc, size = kp[2] * sc;
  ok = ok && fabsf(ptx) < 1e6f && fabsf(pty) < 1e6f && size < 1e6f;
  if (!ok) {
    out[lane] = 0;
    out[lane + 64] = 0;
    return;
  }
  const int rows = g.h[oi], cols = g.w[oi];
  const float* img = pyr + (int64_t)n * g.arena + g.g_off[oi] + layer * rows * cols;
  float ang = 360.f - kp[3];
  if (fabsf(ang - 360.f) < 1.1920929e-07f) ang = 0.f;
  const float scl = size * 0.5f;
  const int pc = (int)rintf(ptx), pr = (int)rintf(pty);
  const float rad = ang * 0.017453292519943295f;
  float cos_t = cosf(rad), sin_t = sinf(rad);
  const float hw = 3.f * scl;
  int radius = (int)rintf(hw * 1.4142135623730951f * 2.5f);
  const int diag = (int)sqrt((double)(cols * cols + rows * rows));
  radius = radius < diag ? radius : diag;
  radius = radius < 0 ? 0 : radius;
  cos_t = cos_t / hw;
  sin_t = sin_t / hw;
  for (int i = lane; i < HL; i += 64) hist[i] = 0ull;
  __syncthreads();
  const int side = 2 * radius + 1;
  for (int s = lane; s < side * side; s += 64) {
    const int i = s / side - radius, j = s % side - radius;
    const float fi = (float)i, fj = (float)j;
    const float c_rot = fj * cos_t - fi * sin_t;
    const float r_rot = fj * sin_t + fi * cos_t;
    const float rbin = r_rot + (float)(D / 2) - 0.5f;
    const float cbin = c_rot + (float)(D / 2) - 0.5f;
    const int r = pr + i, c = pc + j;
    if (!(rbin > -1.f && rbin < (float)D && cbin > -1.f && cbin < (float)D && r > 0 && r < rows - 1 && c > 0 &&
          c < cols - 1))
      continue;
    const float dx = img[r * cols + c + 1] - img[r * cols + c - 1];
    const float dy = img[(r - 1) * cols + c] - img[(r + 1) * cols + c];
    const float wgt = expf((c_rot * c_rot + r_rot * r_rot) * -0.125f);
    float ori = atan2f(dy, dx) * 57.29577951308232f;
    if (ori < 0.f) ori = ori + 360.f;
    const float mag = sqrtf(dx * dx + dy * dy) * wgt;
    const float obin = (ori - ang) * (float)(NB / 360.0);
    const float r0f = floorf(rbin), c0f = floorf(cbin), o0f = floorf(obin);
    const float fr = rbin - r0f, fc = cbin - c0f, fo = obin - o0f;
    const int r0 = (int)r0f, c0 = (int)c0f;
    int o0 = (int)o0f;
    if (o0 < 0) o0 += NB;
    if (o0 >= NB) o0 -= NB;
    if (r0 < -1 || r0 >= D || c0 < -1 || c0 >= D || o0 < 0 || o0 >= NB) continue;
    const float v_r1 = mag * fr, v_r0 = mag - v_r1;
    const float v_rc11 = v_r1 * fc, v_rc10 = v_r1 - v_rc11;
    const float v_rc01 = v_r0 * fc, v_rc00 = v_r0 - v_rc01;
    const int idx = ((r0 + 1) * (D + 2) + c0 + 1) * (NB + 2) + o0;
    const float vs[4] = {v_rc00, v_rc01, v_rc10, v_rc11};
    const int offs[4] = {0, NB + 2, (D + 2) * (NB + 2), (D + 3) * (NB + 2)};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float v1 = vs[q] * fo, v0 = vs[q] - v1;
      atomicAdd(&hist[idx + offs[q]], (unsigned long long)llrintf(v0 * FIXF));
      atomicAdd(&hist[idx + offs[q] + 1], (unsigned long long)llrintf(v1 * FIXF));
    }
  }
  __syncthreads();
  float v[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int t = lane + 64 * q;
    const int i = t / 32, j = (t / 8) % 4, b = t % 8;
    const int idx = ((i + 1) * (D + 2) + (j + 1)) * (NB + 2) + b;
    long long a = (long long)hist[idx];
    if (b < 2) a += (long long)hist[idx + NB];
    v[q] = (float)a * (1.f / FIXF);
  }
  float nrm2 = v[0] * v[0] + v[1] * v[1];
  for (int o = 32; o > 0; o >>= 1) nrm2 = nrm2 + __shfl_xor(nrm2, o, 64);
  const float thr = sqrtf(nrm2) * 0.2f;
  v[0] = fminf(v[0], thr);
  v[1] = fminf(v[1], thr);
  nrm2 = v[0] * v[0] + v[1] * v[1];
  for (int o = 32; o > 0; o >>= 1) nrm2 = nrm2 + __shfl_xor(nrm2, o, 64);
  const float sn = 512.f / fmaxf(sqrtf(nrm2), 1.1920929e-07f);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const float u = rintf(v[q] * sn);
    out[lane + 64 * q] = (uint8_t)(u < 0.f ? 0.f : (u > 255.f ? 255.f : u));
  }
}

// ------------------------------------------------------------------ 4. matcher
// Brute-force 2-NN on integer squared L2: one thread per query (descriptor in registers), the train
// descriptors streamed through LDS in tiles of 64; |q - t|^2 = q.q + t.t - 2 q.t with v_dot4_u32_u8.
__device__ __forceinline__ unsigned dot4(unsigned a, unsigned b, unsigned c) {
#if __has_builtin(__builtin_amdgcn_udot4)
  return __builtin_amdgcn_udot4(a, b, c, false);
#else
  return c + (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) +
         ((a >> 16) & 255u) * ((b >> 16) & 255u) + (a >> 24) * (b >> 24);
#endif
}

__global__ __launch_bounds__(64) void cmc_knn2_kernel(const uint8_t* __restrict__ query,
                                                      const int32_t* __restrict__ n_query,
                                                      const int32_t* __restrict__ q_index,
                                                      const uint8_t* __restrict__ train,
                                                      const int32_t* __restrict__ n_train, int max_kp,
                                                      int32_t* __restrict__ idx, int32_t* __restrict__ dist) {
  __shared__ unsigned tile[64 * 33];
  __shared__ unsigned tt[64];
  const int n = blockIdx.y, qi = blockIdx.x * 64 + threadIdx.x;
  const int qimg = q_index ? q_index[n] : n;
  int nq = n_query[qimg], nt = n_train[n];
  nq = nq < 0 ? 0 : (nq > max_kp ? max_kp : nq);
  nt = nt < 0 ? 0 : (nt > max_kp ? max_kp : nt);
  const bool live = qi < nq;
  unsigned q[32], qq = 0;
  const unsigned* qp = (const unsigned*)(query + ((int64_t)qimg * max_kp + (live ? qi : 0)) * 128);
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    q[k] = live ? qp[k] : 0u;
    qq = dot4(q[k], q[k], qq);
  }
  int d1 = 0x7fffffff, d2 = 0x7fffffff, i1 = -1, i2 = -1;
  const unsigned* tp = (const unsigned*)(train + (int64_t)n * max_kp * 128);
  for (int t0 = 0; t0 < nt; t0 += 64) {
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 32; i += 64) {
      const int row = i >> 5, col = i & 31;
      tile[row * 33 + col] = (t0 + row) < nt ? tp[(int64_t)(t0 + row) * 32 + col] : 0u;
    }
    __syncthreads();
    unsigned s = 0;
    for (int k = 0; k < 32; ++k) s = dot4(tile[threadIdx.x * 33 + k], tile[threadIdx.x * 33 + k], s);
    tt[threadIdx.x] = s;
    __syncthreads();
    const int lim = nt - t0 < 64 ? nt - t0 : 64;
    for (int j = 0; j < lim; ++j) {
      unsigned qt = 0;
#pragma unroll
      for (int k = 0; k < 32; ++k) qt = dot4(q[k], tile[j * 33 + k], qt);
      const int d = (int)(qq + tt[j] - 2u * qt);
      if (d < d1) {
        d2 = d1;
        i2 = i1;
        d1 = d;
        i1 = t0 + j;
      } else if (d < d2) {
        d2 = d;
        i2 = t0 + j;
      }
    }
  }
  if (qi < max_kp) {
    const int64_t o = ((int64_t)n * max_kp + qi) * 2;
    idx[o] = live ? i1 : -1;
    idx[o + 1] = live ? i2 : -1;
    dist[o] = live && i1 >= 0 ? d1 : -1;
    dist[o + 1] = live && i2 >= 0 ? d2 : -1;
  }
}

// Ordered compaction helper: thread t owns `per` consecutive items, `c` of them kept; returns the first
// output position of the thread and the total (256 threads).
__device__ __forceinline__ int block_offsets(int c, int* sh, int& total) {
  sh[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int i = 0; i < 256; ++i) {
      const int v = sh[i];
      sh[i] = s;
      s += v;
    }
    sh[256] = s;
  }
  __syncthreads();
  const int pos = sh[threadIdx.x];
  total = sh[256];
  __syncthreads();
  return pos;
}

__global__ __launch_bounds__(256) void cmc_filter_kernel(const int32_t* __restrict__ idx,
                                                         const int32_t* __restrict__ dist,
                                                         const float* __restrict__ prev_kps,
                                                         const int32_t* __restrict__ n_prev,
                                                         const int32_t* __restrict__ q_index,
                                                         const float* __restrict__ cur_kps,
                                                         const int32_t* __restrict__ n_cur, int max_kp, int h, int w,
                                                         double* __restrict__ tmp, double* __restrict__ good,
                                                         int32_t* __restrict__ n_knn, int32_t* __restrict__ n_good) {
  __shared__ int sh[257];
  __shared__ double stat[4];
  const int n = blockIdx.x, t = threadIdx.x;
  const int qimg = q_index ? q_index[n] : n;
  int nq = n_prev[qimg], nt = n_cur[n];
  nq = nq < 0 ? 0 : (nq > max_kp ? max_kp : nq);
  nt = nt < 0 ? 0 : (nt > max_kp ? max_kp : nt);
  const int per = (max_kp + 255) / 256;
  const float* pk = prev_kps + (int64_t)qimg * max_kp * CMC_KP;
  const float* ck = cur_kps + (int64_t)n * max_kp * CMC_KP;
  double* tp = tmp + (int64_t)n * max_kp * 4;
  double* gp = good + (int64_t)n * max_kp * 4;
  const double gx = 0.25 * (double)w, gy = 0.25 * (double)h;
  auto gate = [&](int qi, double* o) {
    if (qi >= nq) return false;
    const int64_t a = ((int64_t)n * max_kp + qi) * 2;
    const int i1 = idx[a], i2 = idx[a + 1];
    if (i1 < 0 || i1 >= nt || i2 < 0) return false;
    if (!(100ll * (long long)dist[a] < 81ll * (long long)dist[a + 1])) return false;
    o[0] = (double)pk[qi * CMC_KP];
    o[1] = (double)pk[qi * CMC_KP + 1];
    o[2] = (double)ck[i1 * CMC_KP];
    o[3] = (double)ck[i1 * CMC_KP + 1];
    return fabs(o[0] - o[2]) < gx && fabs(o[1] - o[3]) < gy;
  };
  double o[4];
  int c = 0;
  for (int k = 0; k < per; ++k) c += gate(t * per + k, o) ? 1 : 0;
  int total;
  int pos = block_offsets(c, sh, total);
  for (int k = 0; k < per; ++k)
    if (gate(t * per + k, o)) {
      for (int m = 0; m < 4; ++m) tp[(int64_t)pos * 4 + m] = o[m];
      ++pos;
    }
  __syncthreads();
  const int nk = total;
  if (t < 2 && nk > 0) {  // mean and population std of axis t, summed in list order
    double s = 0.0;
    for (int i = 0; i < nk; ++i) s += tp[(int64_t)i * 4 + t] - tp[(int64_t)i * 4 + 2 + t];
    const double mean = s / (double)nk;
    double s2 = 0.0;
    for (int i = 0; i < nk; ++i) {
      const double d = (tp[(int64_t)i * 4 + t] - tp[(int64_t)i * 4 + 2 + t]) - mean;
      s2 += d * d;
    }
    stat[t] = mean;
    stat[2 + t] = 2.5 * sqrt(s2 / (double)nk);
  }
  __syncthreads();
  auto keep = [&](int i) {
    if (i >= nk) return false;
    const double dx = tp[(int64_t)i * 4] - tp[(int64_t)i * 4 + 2], dy = tp[(int64_t)i * 4 + 1] - tp[(int64_t)i * 4 + 3];
    return (dx - stat[0]) < stat[2] && (dy - stat[1]) < stat[3];
  };
  c = 0;
  for (int k = 0; k < per; ++k) c += keep(t * per + k) ? 1 : 0;
  pos = block_offsets(c, sh, total);
  for (int k = 0; k < per; ++k)
    if (keep(t * per + k)) {
      for (int m = 0; m < 4; ++m) gp[(int64_t)pos * 4 + m] = tp[(int64_t)(t * per + k) * 4 + m];
      ++pos;
    }
  if (t == 0) {
    n_knn[n] = nk;
    n_good[n] = total;
  }
}

// ------------------------------------------------------------------ 5. partial affine
__device__ __forceinline__ unsigned hash32(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// 2-point RANSAC for [[a, -b, tx], [b, a, ty]]: one thread per hypothesis (up to 8 each), the matches
// streamed through LDS, block argmax (most inliers, lowest hypothesis), least-squares refit over the inliers.
__global__ __launch_bounds__(256) void cmc_ransac_kernel(const double* __restrict__ pts,
                                                         const int32_t* __restrict__ counts, int max_pts, double thr2,
                                                         double* __restrict__ warps, int32_t* __restrict__ info,
                                                         uint8_t* __restrict__ mask) {
  constexpr int TILE = 512, HPT = 8;
  __shared__ double tile[TILE * 4];
  __shared__ int red_c[256], red_h[256];
  __shared__ double best_p[4];
  const int n = blockIdx.x, t = threadIdx.x;
  const double* P = pts + (int64_t)n * max_pts * 4;
  uint8_t* mk = mask + (int64_t)n * max_pts;
  int N = counts[n];
  N = N < 0 ? 0 : (N > max_pts ? max_pts : N);
  for (int i = t; i < max_pts; i += 256) mk[i] = 0;
  double* W = warps + (int64_t)n * 6;
  auto identity = [&]() {
    if (t == 0) {
      W[0] = 1.0; W[1] = 0.0; W[2] = 0.0; W[3] = 0.0; W[4] = 1.0; W[5] = 0.0;
      info[2 * n] = -1;
      info[2 * n + 1] = 0;
    }
  };
  if (N <= 4) {
    identity();
    return;
  }
  const long long all_pairs = (long long)N * (N - 1) / 2;
  const bool exhaustive = all_pairs <= CMC_MAX_HYP;
  const int nh = exhaustive ? (int)all_pairs : CMC_MAX_HYP;
  double ha[HPT], hb[HPT], hx[HPT], hy[HPT];
  int cnt[HPT];
#pragma unroll
  for (int m = 0; m < HPT; ++m) {
    const int hyp = t + 256 * m;
    cnt[m] = -1;
    ha[m] = hb[m] = hx[m] = hy[m] = 0.0;
    if (hyp >= nh) continue;
    int i, j;
    if (exhaustive) {
      int rem = hyp;
      i = 0;
      while (rem >= N - 1 - i) {
        rem -= N - 1 - i;
        ++i;
      }
      j = i + 1 + rem;
    } else {
      i = (int)(hash32(2u * (unsigned)hyp) % (unsigned)N);
      j = (int)(((unsigned)i + 1u + hash32(2u * (unsigned)hyp + 1u) % (unsigned)(N - 1)) % (unsigned)N);
    }
    if (i < 0 || i >= N || j < 0 || j >= N) continue;
    const double pxi = P[i * 4], pyi = P[i * 4 + 1], qxi = P[i * 4 + 2], qyi = P[i * 4 + 3];
    const double dpx = P[j * 4] - pxi, dpy = P[j * 4 + 1] - pyi;
    const double dqx = P[j * 4 + 2] - qxi, dqy = P[j * 4 + 3] - qyi;
    const double den = dpx * dpx + dpy * dpy;
    if (!(den > 0.0)) continue;
    ha[m] = (dqx * dpx + dqy * dpy) / den;
    hb[m] = (dqy * dpx - dqx * dpy) / den;
    hx[m] = qxi - (ha[m] * pxi - hb[m] * pyi);
    hy[m] = qyi - (hb[m] * pxi + ha[m] * pyi);
    cnt[m] = 0;
  }
  for (int t0 = 0; t0 < N; t0 += TILE) {
    const int lim = N - t0 < TILE ? N - t0 : TILE;
    __syncthreads();
    for (int i = t; i < lim * 4; i += 256) tile[i] = P[(int64_t)t0 * 4 + i];
    __syncthreads();
#pragma unroll
    for (int m = 0; m < HPT; ++m) {
      if (cnt[m] < 0) continue;
      int c = 0;
      for (int k = 0; k < lim; ++k) {
        const double px = tile[k * 4], py = tile[k * 4 + 1];
        const double ex = ha[m] * px - hb[m] * py + hx[m] - tile[k * 4 + 2];
        const double ey = hb[m] * px + ha[m] * py + hy[m] - tile[k * 4 + 3];
        c += (ex * ex + ey * ey < thr2) ? 1 : 0;
      }
      cnt[m] += c;
    }
  }
  int bc = -1, bh = 0x7fffffff, bm = 0;
#pragma unroll
  for (int m = 0; m < HPT; ++m)
    if (cnt[m] > bc) {  // ascending hypothesis index: strict > keeps the lowest
      bc = cnt[m];
      bh = t + 256 * m;
      bm = m;
    }
  red_c[t] = bc;
  red_h[t] = bh;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      const int c2 = red_c[t + o], h2 = red_h[t + o];
      if (c2 > red_c[t] || (c2 == red_c[t] && h2 < red_h[t])) {
        red_c[t] = c2;
        red_h[t] = h2;
      }
    }
    __syncthreads();
  }
  const int best_c = red_c[0], best_h = red_h[0];
  if (best_c < 2) {
    identity();
    return;
  }
  if (bc == best_c && bh == best_h) {  // exactly one thread owns the winning hypothesis
    double a = 0, b = 0, x = 0, y = 0;
#pragma unroll
    for (int m = 0; m < HPT; ++m)
      if (m == bm) {
        a = ha[m];
        b = hb[m];
        x = hx[m];
        y = hy[m];
      }
    best_p[0] = a;
    best_p[1] = b;
    best_p[2] = x;
    best_p[3] = y;
  }
  __syncthreads();
  for (int k = t; k < N; k += 256) {
    const double px = P[k * 4], py = P[k * 4 + 1];
    const double ex = best_p[0] * px - best_p[1] * py + best_p[2] - P[k * 4 + 2];
    const double ey = best_p[1] * px + best_p[0] * py + best_p[3] - P[k * 4 + 3];
    mk[k] = (ex * ex + ey * ey < thr2) ? 1 : 0;
  }
  __syncthreads();
  if (t == 0) {
    double sx = 0, sy = 0, ux = 0, uy = 0;
    for (int k = 0; k < N; ++k)
      if (mk[k]) {
        sx += P[k * 4];
        sy += P[k * 4 + 1];
        ux += P[k * 4 + 2];
        uy += P[k * 4 + 3];
      }
    const double inv = (double)best_c;
    sx = sx / inv;
    sy = sy / inv;
    ux = ux / inv;
    uy = uy / inv;
    double na = 0, nb = 0, den = 0;
    for (int k = 0; k < N; ++k)
      if (mk[k]) {
        const double x = P[k * 4] - sx, y = P[k * 4 + 1] - sy, u = P[k * 4 + 2] - ux, v = P[k * 4 + 3] - uy;
        na += x * u + y * v;
        nb += x * v - y * u;
        den += x * x + y * y;
      }
    if (!(den > 0.0)) {
      W[0] = 1.0; W[1] = 0.0; W[2] = 0.0; W[3] = 0.0; W[4] = 1.0; W[5] = 0.0;
      info[2 * n] = -1;
      info[2 * n + 1] = 0;
    } else {
      const double a = na / den, b = nb / den;
      W[0] = a;
      W[1] = -b;
      W[2] = ux - (a * sx - b * sy);
      W[3] = b;
      W[4] = a;
      W[5] = uy - (b * sx + a * sy);
      info[2 * n] = best_h;
      info[2 * n + 1] = best_c;
    }
  }
}

__global__ void cmc_store_prev_kernel(const float* __restrict__ kps, const uint8_t* __restrict__ desc,
                                      const int32_t* __restrict__ counts, const int32_t* __restrict__ slots, int max_kp,
                                      float* __restrict__ prev_kps, uint8_t* __restrict__ prev_desc,
                                      int32_t* __restrict__ prev_counts) {
  const int n = blockIdx.y, slot = slots[n];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < max_kp * CMC_KP) prev_kps[(int64_t)slot * max_kp * CMC_KP + i] = kps[(int64_t)n * max_kp * CMC_KP + i];
  if (i < max_kp * 32)
    ((unsigned*)prev_desc)[(int64_t)slot * max_kp * 32 + i] = ((const unsigned*)desc)[(int64_t)n * max_kp * 32 + i];
  if (i == 0) prev_counts[slot] = counts[n];
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }

}  // namespace

// ------------------------------------------------------------------ host side
struct SiftWs {
  float* pyr = nullptr;       // n x arena
  float* base = nullptr;      // n x base_h x base_w (unblurred first image)
  uint8_t* flags = nullptr;   // n x flags_total
  int32_t* cand = nullptr;    // n x KCAND
  int32_t* cand_cnt = nullptr;
  float* slots = nullptr;     // n x KCAND x MAXPEAK x 7
  size_t pyr_b = 0, base_b = 0, flags_b = 0;
  int cap_n = 0;
  SiftGeom geom{};
  int built_n = 0;
};

SiftWs* sift_ws_create() { return new SiftWs(); }

void sift_ws_destroy(SiftWs* ws) {
  if (!ws) return;
  (void)hipFree(ws->pyr);
  (void)hipFree(ws->base);
  (void)hipFree(ws->flags);
  (void)hipFree(ws->cand);
  (void)hipFree(ws->cand_cnt);
  (void)hipFree(ws->slots);
  delete ws;
}

int sift_geometry(int h, int w, int first_octave, SiftGeom* g) {
  if (h < 2 || w < 2 || h > 4096 || w > 4096 || (first_octave != 0 && first_octave != -1)) return -1;
  std::memset(g, 0, sizeof(*g));
  g->first_octave = first_octave;
  g->img_h = h;
  g->img_w = w;
  int bh = first_octave < 0 ? 2 * h : h, bw = first_octave < 0 ? 2 * w : w;
  const int mn = bh < bw ? bh : bw;
  int n = (int)std::nearbyint(std::log((double)mn) / std::log(2.0) - 2) - first_octave;
  n = n < 1 ? 1 : (n > CMC_MAX_OCT ? CMC_MAX_OCT : n);
  int off = 0, foff = 0;
  for (int o = 0; o < n; ++o) {
    if ((bh < bw ? bh : bw) < 2 * BORDER + 1 && o > 0) break;
    g->h[o] = bh;
    g->w[o] = bw;
    g->g_off[o] = off;
    off += 6 * bh * bw;
    g->d_off[o] = off;
    off += 5 * bh * bw;
    g->f_off[o] = foff;
    foff += 3 * bh * bw;
    g->n_oct = o + 1;
    bh /= 2;
    bw /= 2;
  }
  g->f_off[g->n_oct] = foff;
  g->arena = off;
  return 0;
}

int64_t sift_dog_floats(const SiftGeom& g) {
  int64_t t = 0;
  for (int o = 0; o < g.n_oct; ++o) t += 5ll * g.h[o] * g.w[o];
  return t;
}

namespace {

template <class T>
int grow(T*& p, size_t& have, size_t need) {
  if (need <= have) return 0;
  (void)hipFree(p);
  p = nullptr;
  have = 0;
  if (hipMalloc((void**)&p, need) != hipSuccess) return -1;
  have = need;
  return 0;
}

int ws_reserve(SiftWs* ws, int n, const SiftGeom& g) {
  const size_t flags_total = (size_t)g.f_off[g.n_oct];
  if (grow(ws->pyr, ws->pyr_b, (size_t)n * g.arena * sizeof(float))) return -1;
  if (grow(ws->base, ws->base_b, (size_t)n * g.h[0] * g.w[0] * sizeof(float))) return -1;
  if (grow(ws->flags, ws->flags_b, (size_t)n * flags_total)) return -1;
  if (n > ws->cap_n) {
    (void)hipFree(ws->cand);
    (void)hipFree(ws->cand_cnt);
    (void)hipFree(ws->slots);
    ws->cand = nullptr;
    ws->cand_cnt = nullptr;
    ws->slots = nullptr;
    ws->cap_n = 0;
    if (hipMalloc((void**)&ws->cand, (size_t)n * CMC_KCAND * sizeof(int32_t)) != hipSuccess) return -1;
    if (hipMalloc((void**)&ws->cand_cnt, (size_t)n * sizeof(int32_t)) != hipSuccess) return -1;
    if (hipMalloc((void**)&ws->slots, (size_t)n * CMC_KCAND * CMC_MAXPEAK * CMC_KP * sizeof(float)) != hipSuccess)
      return -1;
    ws->cap_n = n;
  }
  return 0;
}

int build_pyramid(SiftWs* ws, const uint8_t* gray, int n, int h, int w, int first_octave, hipStream_t s) {
  SiftGeom g;
  if (sift_geometry(h, w, first_octave, &g)) return -1;
  if (ws_reserve(ws, n, g)) return -1;
  ws->geom = g;
  ws->built_n = 0;
  const double sigma = 1.6;
  const double k = std::pow(2.0, 1.0 / N_LAYERS);
  double sig[N_LAYERS + 3];
  sig[0] = sigma;
  for (int i = 1; i < N_LAYERS + 3; ++i) {
    const double prev = sigma * std::pow(k, (double)(i - 1));
    const double tot = prev * k;
    sig[i] = std::sqrt(tot * tot - prev * prev);
  }
  const int up = first_octave < 0 ? 1 : 0;
  const int bh = g.h[0], bw = g.w[0];
  hipLaunchKernelGGL(sift_base_kernel, dim3((bw + 63) / 64, bh, n), dim3(64), 0, s, gray, h, w, up, ws->base,
                     (int64_t)bh * bw);
  const double base_sigma = std::sqrt(std::fmax(sigma * sigma - (up ? 4 * 0.25 : 0.25), 0.01));
  const int64_t stride = g.arena;
  auto blur = [&](const float* in, int64_t in_stride, float* out, int hh, int ww, double sg) {
    hipLaunchKernelGGL(sift_blur_kernel, dim3((ww + BT_W - 1) / BT_W, (hh + BT_H - 1) / BT_H, n), dim3(256), 0, s, in,
                       in_stride, out, stride, hh, ww, make_gauss(sg));
  };
  blur(ws->base, (int64_t)bh * bw, ws->pyr + g.g_off[0], bh, bw, base_sigma);
  for (int o = 0; o < g.n_oct; ++o) {
    const int hh = g.h[o], ww = g.w[o], plane = hh * ww;
    float* go = ws->pyr + g.g_off[o];
    if (o > 0)
      hipLaunchKernelGGL(sift_decimate_kernel, dim3((ww + 63) / 64, hh, n), dim3(64), 0, s,
                         ws->pyr + g.g_off[o - 1] + N_LAYERS * g.h[o - 1] * g.w[o - 1], g.h[o - 1], g.w[o - 1], go, hh,
                         ww, stride);
    for (int i = 1; i < N_LAYERS + 3; ++i) blur(go + (i - 1) * plane, stride, go + i * plane, hh, ww, sig[i]);
    hipLaunchKernelGGL(sift_dog_kernel, dim3((5 * plane + 255) / 256, 1, n), dim3(256), 0, s, go,
                       ws->pyr + g.d_off[o], plane, stride);
  }
  if (launched()) return -1;
  ws->built_n = n;
  return 0;
}

}  // namespace

int cmc_preprocess(const uint8_t* frames, int64_t frame_stride, int n, int H, int W, double scale, uint8_t* gray,
                   hipStream_t s) {
  if (n <= 0) return 0;
  const int h = (int)std::nearbyint(H * scale), w = (int)std::nearbyint(W * scale);
  if (h < 1 || w < 1) return -1;
  hipLaunchKernelGGL(cmc_gray_resize_kernel, dim3((w + 63) / 64, h, n), dim3(64), 0, s, frames, frame_stride, H, W, h,
                     w, 1.0 / scale, gray);
  return launched();
}

int cmc_mask(const double* boxes, const int32_t* box_counts, int max_boxes, int n, int h, int w, double scale,
             uint8_t* mask, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(cmc_mask_kernel, dim3((w + 63) / 64, h, n), dim3(64), 0, s, boxes, box_counts, max_boxes, h, w,
                     scale, mask);
  return launched();
}

int sift_detect(SiftWs* ws, const uint8_t* gray, int n, int h, int w, int first_octave, const uint8_t* mask, int max_kp,
                float* kps, int32_t* counts, float* dog_out, hipStream_t s) {
  if (n <= 0) return 0;
  if (max_kp < 1 || max_kp > CMC_KMAX) return -1;
  if (build_pyramid(ws, gray, n, h, w, first_octave, s)) return -1;
  const SiftGeom& g = ws->geom;
  const int ftotal = g.f_off[g.n_oct];
  if (hipMemsetAsync(ws->flags, 0, (size_t)n * ftotal, s) != hipSuccess) return -1;
  if (hipMemsetAsync(counts, 0, (size_t)n * sizeof(int32_t), s) != hipSuccess) return -1;
  for (int o = 0; o < g.n_oct; ++o) {
    const int hh = g.h[o], ww = g.w[o];
    if (hh < 2 * BORDER + 1 || ww < 2 * BORDER + 1) continue;
    hipLaunchKernelGGL(sift_extrema_kernel, dim3((ww + 63) / 64, hh * N_LAYERS, n), dim3(64), 0, s,
                       ws->pyr + g.d_off[o], (int64_t)g.arena, hh, ww, ws->flags + g.f_off[o], (int64_t)ftotal);
  }
  hipLaunchKernelGGL(sift_compact_kernel, dim3(n), dim3(1024), 0, s, ws->flags, ftotal, ws->cand, ws->cand_cnt);
  hipLaunchKernelGGL(sift_orient_kernel, dim3(CMC_KCAND, n), dim3(64), 0, s, ws->pyr, g, ws->cand, ws->cand_cnt, mask,
                     ws->slots);
  hipLaunchKernelGGL(sift_sort_kernel, dim3(CMC_KCAND * CMC_MAXPEAK / 256, n), dim3(256), 0, s, ws->slots, ws->cand_cnt, max_kp,
                     kps, counts);
  if (launched()) return -1;
  if (dog_out) {
    const int64_t per = sift_dog_floats(g);
    for (int i = 0; i < n; ++i) {
      int64_t off = 0;
      for (int o = 0; o < g.n_oct; ++o) {
        const int64_t cnt = 5ll * g.h[o] * g.w[o];
        if (hipMemcpyAsync(dog_out + i * per + off, ws->pyr + (int64_t)i * g.arena + g.d_off[o], cnt * sizeof(float),
                           hipMemcpyDeviceToDevice, s) != hipSuccess)
          return -1;
        off += cnt;
      }
    }
  }
  return 0;
}

int sift_describe(SiftWs* ws, const uint8_t* gray, int n, int h, int w, int first_octave, const float* kps,
                  const int32_t* counts, int max_kp, uint8_t* desc, hipStream_t s) {
  if (n <= 0) return 0;
  if (max_kp < 1 || max_kp > CMC_KMAX) return -1;
  if (gray) {
    if (build_pyramid(ws, gray, n, h, w, first_octave, s)) return -1;
  } else if (ws->built_n < n || ws->geom.img_h != h || ws->geom.img_w != w || ws->geom.first_octave != first_octave) {
    return -1;
  }
  hipLaunchKernelGGL(sift_describe_kernel, dim3(max_kp, n), dim3(64), 0, s, ws->pyr, ws->geom, kps, counts, max_kp,
                     desc);
  return launched();
}

int desc_match_knn2(const uint8_t* query, const int32_t* n_query, const int32_t* q_index, const uint8_t* train,
                    const int32_t* n_train, int n, int max_kp, int32_t* idx, int32_t* dist, hipStream_t s) {
  if (n <= 0) return 0;
  if (max_kp < 1 || max_kp > CMC_KMAX) return -1;
  hipLaunchKernelGGL(cmc_knn2_kernel, dim3((max_kp + 63) / 64, n), dim3(64), 0, s, query, n_query, q_index, train,
                     n_train, max_kp, idx, dist);
  return launched();
}

int cmc_match_filter(const int32_t* idx, const int32_t* dist, const float* prev_kps, const int32_t* n_prev,
                     const int32_t* q_index, const float* cur_kps, const int32_t* n_cur, int n, int max_kp, int h, int w,
                     double* tmp, double* good, int32_t* n_knn, int32_t* n_good, hipStream_t s) {
  if (n <= 0) return 0;
  if (max_kp < 1 || max_kp > CMC_KMAX) return -1;
  hipLaunchKernelGGL(cmc_filter_kernel, dim3(n), dim3(256), 0, s, idx, dist, prev_kps, n_prev, q_index, cur_kps, n_cur,
                     max_kp, h, w, tmp, good, n_knn, n_good);
  return launched();
}

int affine_partial_ransac(const double* pts, const int32_t* counts, int n, int max_pts, double thresh, double* warps,
                          int32_t* info, uint8_t* mask, hipStream_t s) {
  if (n <= 0) return 0;
  if (max_pts < 1) return -1;
  hipLaunchKernelGGL(cmc_ransac_kernel, dim3(n), dim3(256), 0, s, pts, counts, max_pts, thresh * thresh, warps, info,
                     mask);
  return launched();
}

int cmc_store_prev(const float* kps, const uint8_t* desc, const int32_t* counts, const int32_t* slots, int n, int max_kp,
                   float* prev_kps, uint8_t* prev_desc, int32_t* prev_counts, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(cmc_store_prev_kernel, dim3((max_kp * 32 + 255) / 256, n), dim3(256), 0, s, kps, desc, counts,
                     slots, max_kp, prev_kps, prev_desc, prev_counts);
  return launched();
}

}  // namespace mq
