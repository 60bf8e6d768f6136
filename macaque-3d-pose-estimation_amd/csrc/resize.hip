// Bilinear image resize, uint8 BGR (n, H, W, 3) -> (n, h, w, 3), after cv2.resize's 8-bit INTER_LINEAR fixed-point
// scheme (step3_crossframematching.py visualize :1685 and visualize_result.py :164, :249: cv2.resize(img, [800, 600])).
// Compiled with -ffp-contract=off.  The rule is this project's restatement (tests/track_video_ref.py is the NumPy
// one, equal bit for bit); cv2 is not available to pin it against.
//
// Per axis, scale = (double)src / dst (computed once on the host), destination index d:
//   f = (float)((d + 0.5) * scale - 0.5);  s = floor(f);  f -= s;
//   s < 0: s = 0, f = 0;   s >= src - 1: s = src - 1, f = 0;   second tap s1 = min(s + 1, src - 1)
//   c1 = rint(f * 2048f), c0 = rint((1f - f) * 2048f)          float32, round half to even
// Horizontal pass in int32: R = I[s] * a0 + I[s1] * a1.
// Vertical pass: out = (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2.
//
// One thread per 16-byte chunk of an output row (at most 6 pixels), as overlay.hip's draw_chunk: the coefficients
// are computed per thread in the order above.  WIDE: every source row starts on a 4-byte boundary, and a pixel's
// three bytes come from one or two aligned dword loads; else byte loads.  VEC: 16-byte stores.
#include "common.hpp"
#include "resize.hpp"

namespace mq {

constexpr int RSZ_TILE_CHUNKS = 16;
constexpr int RSZ_TILE_ROWS = 16;
constexpr int RSZ_THREADS = RSZ_TILE_CHUNKS * RSZ_TILE_ROWS;
constexpr int RSZ_CHUNK_PIX = 6;

struct ResizeTap {
  int s0, s1, c0, c1;
};

__device__ __forceinline__ ResizeTap resize_tap(int d, double scale, int src) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  const float fl = floorf(f);
  int s = (int)fl;
  f -= fl;
  if (s < 0) {
    s = 0;
    f = 0.f;
  }
  if (s >= src - 1) {
    s = src - 1;
    f = 0.f;
  }
  ResizeTap t;
  t.s0 = s;
  t.s1 = min(s + 1, src - 1);
  t.c1 = (int)rintf(f * 2048.f);
  t.c0 = (int)rintf((1.f - f) * 2048.f);
  return t;
}

// the three bytes of source pixel x of a row, packed b | g << 8 | r << 16
template <bool WIDE>
__device__ __forceinline__ uint32_t resize_pixel(const uint8_t* __restrict__ row, int x) {
  const int p = 3 * x;
  if (WIDE) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(row + (p & ~3));
    const int sh = 8 * (p & 3);
    uint64_t v = q[0];
    if (sh >= 16) v |= (uint64_t)q[1] << 32;  // the row's length is a multiple of 4: q[1] lies inside it
    return (uint32_t)(v >> sh) & 0xffffffu;
  }
  return (uint32_t)row[p] | (uint32_t)row[p + 1] << 8 | (uint32_t)row[p + 2] << 16;
}

template <bool WIDE, bool VEC>
__global__ __launch_bounds__(RSZ_THREADS) void resize_bilinear_kernel(
    const uint8_t* __restrict__ src, int64_t src_stride, int H, int W, uint8_t* __restrict__ dst, int64_t dst_stride,
    int h, int w, double scale_y, double scale_x, int tiles_x) {
  const int n = blockIdx.y;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int row_bytes = 3 * w;
  const int chunk = tx * RSZ_TILE_CHUNKS + (threadIdx.x % RSZ_TILE_CHUNKS);
  const int y = ty * RSZ_TILE_ROWS + threadIdx.x / RSZ_TILE_CHUNKS;
  const int byte0 = 16 * chunk;
  if (y >= h || byte0 >= row_bytes) return;
  const int X0 = byte0 / 3, S = byte0 % 3;
  const ResizeTap ty_ = resize_tap(y, scale_y, H);
  const uint8_t* img = src + (size_t)n * (size_t)src_stride;
  const uint8_t* r0 = img + (size_t)ty_.s0 * 3 * W;
  const uint8_t* r1 = img + (size_t)ty_.s1 * 3 * W;

  uint32_t pix[RSZ_CHUNK_PIX];
#pragma unroll
  for (int k = 0; k < RSZ_CHUNK_PIX; ++k) {
    pix[k] = 0;
    const int X = X0 + k;
    if (X >= w) continue;
    const ResizeTap t = resize_tap(X, scale_x, W);
    const uint32_t p00 = resize_pixel<WIDE>(r0, t.s0), p01 = resize_pixel<WIDE>(r0, t.s1);
    const uint32_t p10 = resize_pixel<WIDE>(r1, t.s0), p11 = resize_pixel<WIDE>(r1, t.s1);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int R0 = (int)((p00 >> (8 * ch)) & 0xff) * t.c0 + (int)((p01 >> (8 * ch)) & 0xff) * t.c1;
      const int R1 = (int)((p10 >> (8 * ch)) & 0xff) * t.c0 + (int)((p11 >> (8 * ch)) & 0xff) * t.c1;
      const int v = (((ty_.c0 * (R0 >> 4)) >> 16) + ((ty_.c1 * (R1 >> 4)) >> 16) + 2) >> 2;
      pix[k] |= (uint32_t)min(max(v, 0), 255) << (8 * ch);
    }
  }
  uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int k = (i + S) / 3, ch = (i + S) % 3;
    uint32_t p = 0;
#pragma unroll
    for (int kk = 0; kk < RSZ_CHUNK_PIX; ++kk)  // a select chain, so that pix stays in registers
      if (kk == k) p = pix[kk];
    o[i >> 2] |= ((p >> (8 * ch)) & 0xffu) << (8 * (i & 3));
  }
  uint8_t* orow = dst + (size_t)n * (size_t)dst_stride + (size_t)y * row_bytes;
  if (VEC) {
    *reinterpret_cast<uint4*>(orow + byte0) = make_uint4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (byte0 + i < row_bytes) orow[byte0 + i] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
  }
}

int resize_bilinear(const uint8_t* src, int64_t src_stride, int n, int H, int W, uint8_t* dst, int64_t dst_stride, int h,
                    int w, hipStream_t s) {
  if (n <= 0) return 0;
  if (H <= 0 || W <= 0 || h <= 0 || w <= 0 || n > 65535) return -2;
  const int row_bytes = 3 * w;
  const int tiles_x = (row_bytes + 16 * RSZ_TILE_CHUNKS - 1) / (16 * RSZ_TILE_CHUNKS);
  const int tiles_y = (h + RSZ_TILE_ROWS - 1) / RSZ_TILE_ROWS;
  const double sy = (double)H / (double)h, sx = (double)W / (double)w;
  const bool wide = (3 * (int64_t)W) % 4 == 0 && src_stride % 4 == 0 && (uintptr_t)src % 4 == 0;
  const bool vec = row_bytes % 16 == 0 && dst_stride % 16 == 0 && (uintptr_t)dst % 16 == 0;
  const dim3 grid(tiles_x * tiles_y, n);
#define MQ_RSZ_LAUNCH(WD, VC)                                                                                      \
  hipLaunchKernelGGL((resize_bilinear_kernel<WD, VC>), grid, dim3(RSZ_THREADS), 0, s, src, src_stride, H, W, dst, \
                     dst_stride, h, w, sy, sx, tiles_x)
  if (wide && vec)
    MQ_RSZ_LAUNCH(true, true);
  else if (wide)
    MQ_RSZ_LAUNCH(true, false);
  else if (vec)
    MQ_RSZ_LAUNCH(false, true);
  else
    MQ_RSZ_LAUNCH(false, false);
#undef MQ_RSZ_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mq
