// Baseline JPEG decoder for Motion-JPEG frame stores (mq_jpeg_decode): n streams that share one header -> BGR
// frames.  The codec is stated in include/mq_hip.h and restated by tests/jpeg_dec_ref.py, which this equals byte for
// byte.  Integer arithmetic only; the one atomic on global memory is an atomicMax on a frame's status, whose result
// does not depend on the order.
//
// jpeg_dec_markers_kernel  one workgroup per frame walks [scan_offset, size) 16 KB at a time, 16 bytes per lane (one
//                          16-byte load when the slots are 16-byte aligned).  A lane's FF D0..D7 / FF D9 pairs are
//                          counted, a wave + workgroup prefix sum numbers them in stream order, and marker k < n_int
//                          is stored as the end of interval k and compared with the marker that must stand there.
//                          The frame is decoded only if its first EOI is marker n_int - 1 (else status 1).
// jpeg_dec_entropy_kernel  one lane per restart interval (jpeg_dec_dev.hpp jpeg_dec_interval): the tables are built in
//                          LDS from the by-value header by lanes 0..4; a lane writes only its non-zero coefficients,
//                          de-zigzagged, into int16 [frame][mcu][block][64] (zeroed by hipMemsetAsync before).
// jpeg_idct_kernel         one wave per MCU (four per workgroup): lane = (block, column) dequantises and runs the
//                          column pass into LDS, lane = (block, row) the row pass, clamps and stores 8 bytes of a
//                          component plane (MCU-padded extent).
// jpeg_colour_kernel       four pixels of a row per lane: chroma taken (4:4:4), replicated or interpolated by
//                          libjpeg's h2v1 / h2v2 rules with the neighbourhood clamped to the true chroma extent,
//                          fixed-point YCbCr -> RGB, three dword stores (byte stores at unaligned rows and row ends).
//
// Bounds.  Stream reads lie in [0, min(sizes[f], stream_stride)) of the frame's slot; interval ends are marker
// positions inside that range, in increasing order.  Coefficient writes lie in the lane's own n_mcus MCUs (index
// <= 63 within a block).  Planes are MCU-padded, so the IDCT stores whole blocks; the colour kernel reads chroma
// inside the true extent and writes pixels x < W, y < H of its own frame only.
#include "jpeg_dec.hpp"
#include "workspace.hpp"

#include <limits.h>
#include <string.h>

namespace mq {

// ------------------------------------------------------------------------------------------------ markers
constexpr int MRK_THREADS = 1024;  // 16 waves: one frame is walked by one workgroup, 16 KB per step

__device__ __forceinline__ bool is_end_marker(uint32_t m) { return (m >= 0xd0u && m <= 0xd7u) || m == 0xd9u; }

__global__ __launch_bounds__(MRK_THREADS) void jpeg_dec_markers_kernel(const uint8_t* __restrict__ streams,
                                                                       int64_t stream_stride,
                                                                       const int32_t* __restrict__ sizes,
                                                                       int64_t scan_offset, int n_int, int vec,
                                                                       int32_t* __restrict__ iv_end,
                                                                       int32_t* __restrict__ frame_ok,
                                                                       int32_t* __restrict__ status) {
  __shared__ int wave_cnt[MRK_THREADS / 64];
  __shared__ int s_bad, s_eoi;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = blockIdx.x;
  const uint8_t* src = streams + (size_t)f * (size_t)stream_stride;
  const int64_t size = min((int64_t)max(sizes[f], 0), stream_stride);
  int32_t* ends = iv_end + (size_t)f * n_int;
  if (tid == 0) {
    s_bad = 0;
    s_eoi = INT_MAX;
  }
  __syncthreads();
  int base = 0;  // markers before this chunk (saturates far below INT_MAX: at most size / 2)
  for (int64_t chunk = scan_offset & ~(int64_t)15; chunk < size; chunk += MRK_THREADS * 16) {
    const int64_t p0 = chunk + (int64_t)tid * 16;
    uint32_t b[17];
    if (vec && p0 + 16 <= size) {
      const uint4 q = *reinterpret_cast<const uint4*>(src + p0);
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) b[j] = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) b[j] = p0 + j < size ? src[p0 + j] : 0u;
    }
    b[16] = p0 + 16 < size ? src[p0 + 16] : 0u;
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j)  // the pair (p, p + 1) lies in [scan_offset, size)
      if (b[j] == 0xffu && is_end_marker(b[j + 1]) && p0 + j >= scan_offset && p0 + j + 1 < size) mask |= 1u << j;
    const int cnt = __popc(mask);
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wave_cnt[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < MRK_THREADS / 64; ++w) {
      if (w < wave) before += wave_cnt[w];
      total += wave_cnt[w];
    }
    int k = base + before + incl - cnt;
    bool bad = false;
    int eoi = INT_MAX;
    while (mask) {
      const int j = __ffs(mask) - 1;
      mask &= mask - 1;
      const uint32_t m = b[j + 1];
      if (k < n_int) {
        ends[k] = (int32_t)(p0 + j);
        bad |= m != (k == n_int - 1 ? 0xd9u : 0xd0u + (uint32_t)(k & 7));
      }
      if (m == 0xd9u) eoi = min(eoi, k);
      ++k;
    }
    if (bad) atomicOr(&s_bad, 1);
    if (eoi != INT_MAX) atomicMin(&s_eoi, eoi);
    __syncthreads();
    base += total;
    if (s_eoi != INT_MAX) break;  // the same value in every lane: read after the barrier
    __syncthreads();              // wave_cnt is rewritten by the next chunk
  }
  __syncthreads();
  if (tid == 0) {
    const int ok = s_eoi == n_int - 1 && !s_bad;
    frame_ok[f] = ok;
    status[f] = ok ? JPEG_ST_OK : JPEG_ST_MARKERS;
  }
}

// ------------------------------------------------------------------------------------------------ entropy
__global__ __launch_bounds__(64) void jpeg_dec_entropy_kernel(const uint8_t* __restrict__ streams,
                                                              int64_t stream_stride, mq_jpeg_info info, int n_mcu,
                                                              int ri, int n_int, const int32_t* __restrict__ iv_end,
                                                              const int32_t* __restrict__ frame_ok,
                                                              int16_t* __restrict__ coef,
                                                              int32_t* __restrict__ status) {
  __shared__ JpegDecTables T;
  const int lane = threadIdx.x, f = blockIdx.y;
  if (lane < 4) jpeg_dec_build_table(info, &T, lane);
  if (lane == 4) jpeg_dec_zigzag(T.zigzag);
  __syncthreads();
  const int i = blockIdx.x * 64 + lane;
  if (i >= n_int || !frame_ok[f]) return;
  const JpegDecShape shape = jpeg_dec_shape(info);
  const int32_t* ends = iv_end + (size_t)f * n_int;
  const int64_t begin = i == 0 ? info.scan_offset : (int64_t)ends[i - 1] + 2;
  const int64_t end = ends[i];
  const int m0 = i * ri;  // i < n_int = ceil(n_mcu / ri): no overflow
  const int st = jpeg_dec_interval(streams + (size_t)f * (size_t)stream_stride, begin, end, &T, shape,
                                   min(ri, n_mcu - m0), coef + ((size_t)f * n_mcu + m0) * shape.n_blocks * 64, nullptr);
  if (st) atomicMax(&status[f], st);
}

// --------------------------------------------------------------------------------------------------- IDCT
constexpr int IDCT_MCUS = 4;   // MCUs (waves) per workgroup
constexpr int MID_STRIDE = 72;  // ints per block of the column pass's output: 64 + 8, so the stores of a 32-lane half (4 blocks x 8 columns) fall on 32 banks

struct JpegDecQuant {
  uint8_t q[3][64];
};

__global__ __launch_bounds__(64 * IDCT_MCUS) void jpeg_idct_kernel(const int16_t* __restrict__ coef, int n_mcu,
                                                                   JpegDecGeom g, JpegDecQuant q,
                                                                   uint8_t* __restrict__ plane_y,
                                                                   uint8_t* __restrict__ plane_cb,
                                                                   uint8_t* __restrict__ plane_cr) {
  __shared__ __attribute__((aligned(16))) int16_t raw[IDCT_MCUS][6 * 64];
  __shared__ int32_t mid[IDCT_MCUS][6 * MID_STRIDE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = blockIdx.x * IDCT_MCUS + wave, f = blockIdx.y;
  const bool active = m < n_mcu && lane < g.n_blocks * 8;
  const int b = lane >> 3, x = lane & 7;
  if (active)
    *reinterpret_cast<uint4*>(&raw[wave][lane * 8]) =
        *reinterpret_cast<const uint4*>(coef + ((size_t)f * n_mcu + m) * g.n_blocks * 64 + lane * 8);
  __syncthreads();
  if (active) {  // (block, column x)
    const int comp = b < g.n_luma ? 0 : b - g.n_luma + 1;
    int32_t in[8], out[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) in[y] = (int32_t)raw[wave][b * 64 + y * 8 + x] * (int32_t)q.q[comp][y * 8 + x];
    jpeg_idct_islow_1d<11>(in, out);
#pragma unroll
    for (int y = 0; y < 8; ++y) mid[wave][b * MID_STRIDE + y * 8 + x] = out[y];
  }
  __syncthreads();
  if (active) {  // (block, row y)
    const int y = x;
    int32_t in[8], out[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = mid[wave][b * MID_STRIDE + y * 8 + k];
    jpeg_idct_islow_1d<18>(in, out);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= (uint32_t)min(max(out[k] + 128, 0), 255) << (8 * k);
      hi |= (uint32_t)min(max(out[k + 4] + 128, 0), 255) << (8 * k);
    }
    const int my = m / g.mcus_x, mx = m % g.mcus_x;
    uint8_t* dst;
    if (b < g.n_luma) {
      const int bx = mx * g.h + b % g.h, by = my * g.v + b / g.h;
      dst = plane_y + (size_t)f * g.y_bytes + (size_t)(by * 8 + y) * g.y_stride + (size_t)bx * 8;
    } else {
      dst = (b == g.n_luma ? plane_cb : plane_cr) + (size_t)f * g.c_bytes + (size_t)(my * 8 + y) * g.c_stride +
            (size_t)mx * 8;
    }
    *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
  }
}

// ------------------------------------------------------------------------------------------------- colour
constexpr int COL_THREADS = 256;

// the chroma sample of output pixel (y, x) from plane c (stride g.c_stride)
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ c, const JpegDecGeom& g, int y, int x) {
  if (g.h == 1) return c[(size_t)y * g.c_stride + x];
  const int cx = x >> 1;
  if (!g.fancy) return c[(size_t)(g.v == 2 ? y >> 1 : y) * g.c_stride + cx];
  const int ox = (x & 1) ? min(cx + 1, g.cw - 1) : max(cx - 1, 0);
  if (g.v == 1) {
    const uint8_t* r = c + (size_t)y * g.c_stride;
    return (3 * r[cx] + r[ox] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int cy = y >> 1;
  const int oy = (y & 1) ? min(cy + 1, g.ch - 1) : max(cy - 1, 0);
  const uint8_t *r = c + (size_t)cy * g.c_stride, *o = c + (size_t)oy * g.c_stride;
  const int s = 3 * r[cx] + o[cx], t = 3 * r[ox] + o[ox];
  return (3 * s + t + ((x & 1) ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(COL_THREADS) void jpeg_colour_kernel(const uint8_t* __restrict__ plane_y,
                                                                  const uint8_t* __restrict__ plane_cb,
                                                                  const uint8_t* __restrict__ plane_cr, JpegDecGeom g,
                                                                  uint8_t* __restrict__ frames, int64_t frame_stride) {
  const int x0 = (blockIdx.x * COL_THREADS + threadIdx.x) * 4;
  const int y = blockIdx.y, f = blockIdx.z;
  if (x0 >= g.W) return;
  const uint8_t* py = plane_y + (size_t)f * g.y_bytes + (size_t)y * g.y_stride;
  const uint8_t* pcb = plane_cb + (size_t)f * g.c_bytes;
  const uint8_t* pcr = plane_cr + (size_t)f * g.c_bytes;
  const int n = min(4, g.W - x0);
  uint8_t px[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = min(x0 + k, g.W - 1);
    const int Y = py[x];
    int B = Y, G = Y, R = Y;
    if (g.n_comp == 3) {
      const int cb = chroma_at(pcb, g, y, x) - 128, cr = chroma_at(pcr, g, y, x) - 128;
      R = Y + ((91881 * cr + 32768) >> 16);
      G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
      B = Y + ((116130 * cb + 32768) >> 16);
    }
    px[3 * k] = (uint8_t)min(max(B, 0), 255);
    px[3 * k + 1] = (uint8_t)min(max(G, 0), 255);
    px[3 * k + 2] = (uint8_t)min(max(R, 0), 255);
  }
  uint8_t* dst = frames + (size_t)f * (size_t)frame_stride + ((size_t)y * g.W + x0) * 3;
  if (n == 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int w = 0; w < 3; ++w)
      d[w] = px[4 * w] | ((uint32_t)px[4 * w + 1] << 8) | ((uint32_t)px[4 * w + 2] << 16) |
             ((uint32_t)px[4 * w + 3] << 24);
  } else {
    for (int j = 0; j < 3 * n; ++j) dst[j] = px[j];
  }
}

// -------------------------------------------------------------------------------------------------- host
int jpeg_dec_geom(const mq_jpeg_info& info, JpegDecGeom& g) {
  if (info.height < 1 || info.height > 65535 || info.width < 1 || info.width > 65535) return -2;
  if (info.n_comp != 1 && info.n_comp != 3) return -2;
  const int h = info.n_comp == 3 ? info.h_luma : 1, v = info.n_comp == 3 ? info.v_luma : 1;
  if (!((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2))) return -2;
  if (info.restart_interval < 0 || info.restart_interval > 65535 || info.scan_offset < 2) return -2;
  for (int c = 0; c < 3; ++c)
    if (info.dc_sel[c] > 1 || info.ac_sel[c] > 1) return -2;
  g.H = info.height;
  g.W = info.width;
  g.n_comp = info.n_comp;
  g.h = h;
  g.v = v;
  g.n_luma = h * v;
  g.n_blocks = info.n_comp == 3 ? g.n_luma + 2 : 1;
  g.mcus_x = (g.W + 8 * h - 1) / (8 * h);
  g.mcus_y = (g.H + 8 * v - 1) / (8 * v);
  g.n_mcu = g.mcus_x * g.mcus_y;  // <= 8192^2 = 2^26
  g.ri = info.restart_interval ? info.restart_interval : g.n_mcu;
  g.n_int = (g.n_mcu + g.ri - 1) / g.ri;
  g.y_stride = g.mcus_x * 8 * h;
  g.y_bytes = (int64_t)g.y_stride * g.mcus_y * 8 * v;
  g.c_stride = g.mcus_x * 8;
  g.c_bytes = info.n_comp == 3 ? (int64_t)g.c_stride * g.mcus_y * 8 : 0;
  g.cw = (g.W + h - 1) / h;
  g.ch = (g.H + v - 1) / v;
  g.fancy = h == 2 && g.cw > 2;
  return 0;
}

namespace {

struct JpegDecBufs {
  int16_t* coef;  // [n][n_mcu][n_blocks][64]
  size_t n_coef;
  uint8_t *plane_y, *plane_cb, *plane_cr;
  int32_t *iv_end, *frame_ok;
};

JpegDecBufs jpeg_dec_layout(Carver& c, int n, const JpegDecGeom& g) {
  JpegDecBufs b;
  b.n_coef = (size_t)n * g.n_mcu * g.n_blocks * 64;
  b.coef = c.take<int16_t>(b.n_coef);
  b.plane_y = c.take<uint8_t>((size_t)n * g.y_bytes);
  b.plane_cb = c.take<uint8_t>((size_t)n * g.c_bytes);
  b.plane_cr = c.take<uint8_t>((size_t)n * g.c_bytes);
  b.iv_end = c.take<int32_t>((size_t)n * g.n_int);
  b.frame_ok = c.take<int32_t>(n);
  return b;
}

}  // namespace

size_t jpeg_dec_workspace_bytes(int n, const JpegDecGeom& g) { return measure(jpeg_dec_layout, n, g); }

int jpeg_decode(const uint8_t* streams, int64_t stream_stride, const int32_t* sizes, int n, const mq_jpeg_info& info,
                const JpegDecGeom& g, uint8_t* frames, int64_t frame_stride, int32_t* status, void* ws, size_t ws_bytes,
                hipStream_t s) {
  Carver c(ws, ws_bytes);
  const JpegDecBufs b = jpeg_dec_layout(c, n, g);
  if (!c.fits()) return -5;
  int16_t* coef = b.coef;
  uint8_t *plane_y = b.plane_y, *plane_cb = b.plane_cb, *plane_cr = b.plane_cr;
  int32_t *iv_end = b.iv_end, *frame_ok = b.frame_ok;

  if (hipMemsetAsync(coef, 0, b.n_coef * sizeof(int16_t), s) != hipSuccess) return -1;
  const int vec = (uintptr_t)streams % 16 == 0 && stream_stride % 16 == 0;
  hipLaunchKernelGGL(jpeg_dec_markers_kernel, dim3(n), dim3(MRK_THREADS), 0, s, streams, stream_stride, sizes,
                     (int64_t)info.scan_offset, g.n_int, vec, iv_end, frame_ok, status);
  hipLaunchKernelGGL(jpeg_dec_entropy_kernel, dim3((g.n_int + 63) / 64, n), dim3(64), 0, s, streams, stream_stride,
                     info, g.n_mcu, g.ri, g.n_int, iv_end, frame_ok, coef, status);
  JpegDecQuant q;
  memcpy(q.q, info.quant, sizeof(q.q));
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((g.n_mcu + IDCT_MCUS - 1) / IDCT_MCUS, n), dim3(64 * IDCT_MCUS), 0, s,
                     coef, g.n_mcu, g, q, plane_y, plane_cb, plane_cr);
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3((g.W + 4 * COL_THREADS - 1) / (4 * COL_THREADS), g.H, n),
                     dim3(COL_THREADS), 0, s, plane_y, plane_cb, plane_cr, g, frames, frame_stride);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mq
