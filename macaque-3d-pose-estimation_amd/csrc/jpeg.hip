// Baseline JPEG encoder for the overlay frames (mq_jpeg_encode): 8-bit sequential DCT, YCbCr 4:2:0, one
// interleaved scan, the Annex K tables, a restart marker every RI MCUs.  Integer arithmetic only: the stream is
// tests/jpeg_ref.py's byte for byte.  No floating point, no atomics on global memory, no data-dependent order.
//
// jpeg_dct_quant_kernel  one wave per MCU (four per workgroup).  16 x 16 BGR pixels (16-byte loads staged through
//                        LDS when every row starts on a 16-byte boundary, clamped byte loads otherwise; the
//                        clamp is the edge replication) -> Y, 2 x 2-averaged Cb / Cr (bias 1, 2, 1, 2, ...), level shift; per 8 x 8 block
//                        A = (T X + 1024) >> 11, B = A T^T, q = sign(B) ((|B| + (Q << 14)) / (Q << 15)) with the
//                        division as >> 15 and an exact multiply by ceil(2^20 / Q); int16 [frame][mcu][6][64],
//                        zigzag order.
// jpeg_entropy_kernel    one wave per restart interval, one lane per zigzag coefficient of the current block.  A
//                        ballot of the non-zero lanes gives each its zero run; a lane forms ZRLs + code + extra
//                        bits (<= 59 bits), a wave prefix sum places them, LDS atomic ORs write them into a 4 KB
//                        bit buffer.  When the next block might not fit, or the interval ends, the whole bytes
//                        are stuffed (ballot + prefix of the 0xFF bytes) into the interval's worst-case slot of
//                        the scratch buffer; the partial byte carries over.
// jpeg_scan_kernel       one wave per frame: exclusive scan of the interval lengths -> byte offsets, out_size.
// jpeg_gather_kernel     one wave per interval: its bytes, its RSTn (or EOI) marker, and (interval 0) the header
//                        into the caller's slot.  Split from the scan so that a frame is copied by every CU,
//                        not by one workgroup.
//
// Bounds.  A block codes at most JPEG_BLOCK_MAX_BITS = 20 + 63 * 26 bits: a DC code has at most 9 bits and 11 extra
// bits; an AC code has at most 16 bits and 10 extra bits (|AC| <= 840 < 1024 by the matrix norms), and a ZRL
// replaces 16 coefficients by at most 11 bits.  An interval of RI MCUs is padded to a byte, so it has at most
// ceil(RI * 6 * JPEG_BLOCK_MAX_BITS / 8) bytes before stuffing and twice that after: the slot.  Every write to a
// slot and to `out` is also guarded by the slot's and the caller's stride.
#include "jpeg.hpp"
#include "workspace.hpp"

#include <string.h>

#include <algorithm>

namespace mq {

// ------------------------------------------------------------------------------------------------ tables
// T[u][x] = rint(8192 c_u / 2 cos((2x + 1) u pi / 16)), c_0 = sqrt(1/2)
__device__ constexpr int K_T[8][8] = {
    {2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},       {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
    {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784},   {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
    {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896},   {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
    {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567},   {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

// natural index (u * 8 + v) of the k-th coefficient of the scan
constexpr uint8_t K_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
struct ZigzagPos {
  uint8_t p[64];
};
constexpr ZigzagPos make_zigzag_pos() {
  ZigzagPos z{};
  for (int k = 0; k < 64; ++k) z.p[K_ZIGZAG[k]] = (uint8_t)k;
  return z;
}
__constant__ const ZigzagPos K_ZZPOS = make_zigzag_pos();  // scan position of natural index n

// Annex K.1 / K.2, natural order
constexpr uint8_t K_Q_LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t K_Q_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                    99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// Annex K.3 - K.6: code counts per length 1..16, then the symbols
constexpr uint8_t K_DC_L_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t K_DC_C_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t K_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t K_AC_L_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
constexpr uint8_t K_AC_L_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14,
    0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09,
    0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a,
    0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65,
    0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88,
    0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9,
    0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea,
    0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t K_AC_C_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
constexpr uint8_t K_AC_C_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32,
    0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16,
    0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39,
    0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64,
    0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86,
    0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8,
    0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9,
    0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// canonical codes (Annex C): entry = (code << 5) | length, 0 for a symbol the table does not hold
struct HuffTab {
  uint32_t e[256];
};
constexpr HuffTab make_huff(const uint8_t* bits, const uint8_t* vals) {
  HuffTab t{};
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) t.e[vals[k++]] = (code++ << 5) | (uint32_t)len;
    code <<= 1;
  }
  return t;
}
// [0] luma, [1] chroma
__constant__ const HuffTab K_DC_TAB[2] = {make_huff(K_DC_L_BITS, K_DC_VALS), make_huff(K_DC_C_BITS, K_DC_VALS)};
__constant__ const HuffTab K_AC_TAB[2] = {make_huff(K_AC_L_BITS, K_AC_L_VALS), make_huff(K_AC_C_BITS, K_AC_C_VALS)};

// --------------------------------------------------------------------------------------------- DCT + quant
constexpr int DCT_MCUS = 4;  // MCUs (waves) per workgroup

template <bool VEC>
__global__ __launch_bounds__(64 * DCT_MCUS) void jpeg_dct_quant_kernel(const uint8_t* __restrict__ frames,
                                                                       int64_t frame_stride, int H, int W, int mcus_x,
                                                                       int n_mcu, JpegQuant q,
                                                                       int16_t* __restrict__ coef) {
  __shared__ __attribute__((aligned(16))) uint8_t raw[DCT_MCUS][16 * 48];
  __shared__ int X[DCT_MCUS][6 * 64];
  __shared__ int A[DCT_MCUS][6 * 64];
  __shared__ __attribute__((aligned(16))) int16_t O[DCT_MCUS][6 * 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = blockIdx.x * DCT_MCUS + wave;
  const bool active = m < n_mcu;
  const int my = active ? m / mcus_x : 0, mx = active ? m % mcus_x : 0;
  const uint8_t* img = frames + (size_t)blockIdx.y * (size_t)frame_stride;
  const size_t row_bytes = (size_t)3 * W;

  if (VEC) {  // W % 16 == 0: the MCU's rows are 48 whole bytes, 16-byte aligned
    if (active && lane < 48) {
      const int row = lane / 3, ch = lane % 3;
      const int gy = min(my * 16 + row, H - 1);
      *reinterpret_cast<uint4*>(&raw[wave][row * 48 + ch * 16]) =
          *reinterpret_cast<const uint4*>(img + (size_t)gy * row_bytes + (size_t)mx * 48 + ch * 16);
    }
    __syncthreads();
  }
  if (active) {  // one 2 x 2 quad per lane
    const int qy = lane >> 3, qx = lane & 7;
    int cb = 0, cr = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int py = 2 * qy + (d >> 1), px = 2 * qx + (d & 1);
      int b, g, r;
      if (VEC) {
        const uint8_t* p = &raw[wave][py * 48 + px * 3];
        b = p[0], g = p[1], r = p[2];
      } else {
        const int gy = min(my * 16 + py, H - 1), gx = min(mx * 16 + px, W - 1);
        const uint8_t* p = img + (size_t)gy * row_bytes + (size_t)gx * 3;
        b = p[0], g = p[1], r = p[2];
      }
      const int y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
      cb += min(max(((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128, 0), 255);
      cr += min(max(((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128, 0), 255);
      X[wave][((py >> 3) * 2 + (px >> 3)) * 64 + (py & 7) * 8 + (px & 7)] = y - 128;
    }
    const int bias = 1 + (qx & 1);  // libjpeg's h2v2 rule: 1, 2, 1, 2, ... along a chroma row, so ties do not all round up
    X[wave][4 * 64 + qy * 8 + qx] = ((cb + bias) >> 2) - 128;
    X[wave][5 * 64 + qy * 8 + qx] = ((cr + bias) >> 2) - 128;
  }
  __syncthreads();
  if (active && lane < 48) {  // (block, column x): A[u][x] = (sum_y T[u][y] X[y][x] + 1024) >> 11
    const int b = lane >> 3, x = lane & 7;
    int xs[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) xs[y] = X[wave][b * 64 + y * 8 + x];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int acc = 0;
#pragma unroll
      for (int y = 0; y < 8; ++y) acc += K_T[u][y] * xs[y];
      A[wave][b * 64 + u * 8 + x] = (acc + 1024) >> 11;
    }
  }
  __syncthreads();
  if (active && lane < 48) {  // (block, row u): B[u][v] = sum_x A[u][x] T[v][x], quantised into scan order
    const int b = lane >> 3, u = lane & 7, t = b >= 4;
    int as[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) as[x] = A[wave][b * 64 + u * 8 + x];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      int acc = 0;
#pragma unroll
      for (int x = 0; x < 8; ++x) acc += as[x] * K_T[v][x];
      const int nat = u * 8 + v;
      const uint32_t Q = q.q[t][nat];
      // (|B| + (Q << 14)) / (Q << 15) = ((|B| + (Q << 14)) >> 15) / Q;  the dividend is < 2^11, so the multiply by
      // ceil(2^20 / Q) is exact (2^11 * 255 < 2^20)
      const uint32_t mag = ((uint32_t)abs(acc) + (Q << 14)) >> 15;
      const int qv = (int)((mag * q.recip[t][nat]) >> 20);
      O[wave][b * 64 + K_ZZPOS.p[nat]] = (int16_t)(acc < 0 ? -qv : qv);
    }
  }
  __syncthreads();
  if (active && lane < 48)
    *reinterpret_cast<uint4*>(coef + ((size_t)blockIdx.y * n_mcu + m) * 384 + lane * 8) =
        *reinterpret_cast<const uint4*>(&O[wave][lane * 8]);
}

// ------------------------------------------------------------------------------------------------ entropy
// OR `len` (1..64) bits, right-aligned in `bits`, into the big-endian bit stream `buf` at bit `p`
__device__ __forceinline__ void put_bits(uint32_t* buf, int p, uint64_t bits, int len) {
  const uint64_t V = bits << (64 - len);
  const int w = p >> 5, sh = p & 31;
  const uint32_t a = (uint32_t)(V >> (32 + sh)), b = (uint32_t)(V >> sh),
                 c = (uint32_t)(((V & 0xffffffffull) << 32) >> sh);
  if (a) atomicOr(&buf[w], a);
  if (b) atomicOr(&buf[w + 1], b);
  if (c) atomicOr(&buf[w + 2], c);
}

// The bit buffer of a wave: 4 KB, flushed when the next block might not fit (or the interval ends).  A block adds at
// most JPEG_BLOCK_MAX_BITS, the closing pad 7, and put_bits touches two words past the one it starts in.
constexpr int ENT_WORDS = 1024;
constexpr int ENT_FLUSH_BITS = ENT_WORDS * 32 - 2 * JPEG_BLOCK_MAX_BITS - 128;

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, int n_mcu, int ri,
                                                          int n_int, uint8_t* __restrict__ scratch, int slot,
                                                          int32_t* __restrict__ lens) {
  __shared__ uint32_t buf[ENT_WORDS];
  const int lane = threadIdx.x;
  const int i = blockIdx.x, f = blockIdx.y;
  const int m0 = i * ri, n_blk = (min(m0 + ri, n_mcu) - m0) * 6;
  const int16_t* c = coef + ((size_t)f * n_mcu + m0) * 384;
  uint8_t* dst = scratch + ((size_t)f * n_int + i) * (size_t)slot;
  const uint64_t below = (1ull << lane) - 1;
  int used = 0, pos = 0;        // bits in the buffer, bytes written to the slot
  int pred_y = 0, pred_cb = 0, pred_cr = 0;   // lane 0: the DC predictors
  for (int w = lane; w < ENT_WORDS; w += 64) buf[w] = 0;
  __syncthreads();
  int v_next = c[lane];
  for (int blk = 0; blk < n_blk; ++blk) {
    const int b = blk % 6, t = b >= 4;
    int v = v_next;
    if (blk + 1 < n_blk) v_next = c[(blk + 1) * 64 + lane];
    if (lane == 0) {
      const int dc = v;
      if (b < 4) {
        v -= pred_y;
        pred_y = dc;
      } else if (b == 4) {
        v -= pred_cb;
        pred_cb = dc;
      } else {
        v -= pred_cr;
        pred_cr = dc;
      }
    }
    const uint64_t mask = __ballot(lane > 0 && v != 0);
    const int av = abs(v);
    const int s = av ? 32 - __clz(av) : 0;
    const uint32_t extra = (uint32_t)(v >= 0 ? v : v + (1 << s) - 1) & ((1u << s) - 1);
    uint64_t bits = 0;
    int len = 0;
    if (lane == 0) {
      const uint32_t e = K_DC_TAB[t].e[s];
      bits = ((uint64_t)(e >> 5) << s) | extra;
      len = (int)(e & 31) + s;
    } else if (v != 0) {
      const uint64_t pm = mask & below;
      const int run = pm ? lane - 1 - (63 - __clzll(pm)) : lane - 1;
      const uint32_t z = K_AC_TAB[t].e[0xF0];
      for (int k = run >> 4; k > 0; --k) {
        bits = (bits << (z & 31)) | (z >> 5);
        len += (int)(z & 31);
      }
      const uint32_t e = K_AC_TAB[t].e[((run & 15) << 4) | s];
      bits = (((bits << (e & 31)) | (e >> 5)) << s) | extra;
      len += (int)(e & 31) + s;
    } else if (lane == 63) {  // coefficient 63 is zero: EOB
      const uint32_t e = K_AC_TAB[t].e[0];
      bits = e >> 5;
      len = (int)(e & 31);
    }
    int incl = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    // the pieces of different blocks never share a bit, so the ORs of successive blocks need no barrier between them
    if (len) put_bits(buf, used + incl - len, bits, len);
    used += __shfl(incl, 63);
    const bool last = blk == n_blk - 1;
    if (!last && used <= ENT_FLUSH_BITS) continue;

    __syncthreads();
    if (last && (used & 7)) {  // the interval ends: 1-bits up to the byte
      const int r = 8 - (used & 7);
      if (lane == 0) put_bits(buf, used, (1u << r) - 1, r);
      used += r;
      __syncthreads();
    }
    const int n_full = used >> 3, rem = used & 7;
    for (int base = 0; base < n_full; base += 64) {  // whole bytes, each 0xFF followed by a zero byte
      const int idx = base + lane;
      const bool valid = idx < n_full;
      const uint32_t byte = valid ? (buf[idx >> 2] >> (24 - 8 * (idx & 3))) & 0xffu : 0u;
      const bool ff = valid && byte == 0xffu;
      const uint64_t fm = __ballot(ff);
      const int o = pos + lane + __popcll(fm & below);
      if (valid && o < slot) dst[o] = (uint8_t)byte;
      if (ff && o + 1 < slot) dst[o + 1] = 0;
      pos += min(64, n_full - base) + __popcll(fm);
    }
    const uint32_t cb = rem ? (buf[n_full >> 2] >> (24 - 8 * (n_full & 3))) & 0xffu : 0u;
    __syncthreads();
    for (int w = lane; w <= (n_full >> 2) + 2 && w < ENT_WORDS; w += 64) buf[w] = w == 0 ? cb << 24 : 0u;
    used = rem;  // the partial byte carries over
    __syncthreads();
  }
  if (lane == 0) lens[(size_t)f * n_int + i] = min(pos, slot);
}

// ------------------------------------------------------------------------------------------- scan + gather
__global__ __launch_bounds__(64) void jpeg_scan_kernel(const int32_t* __restrict__ lens, int n_int,
                                                       int32_t* __restrict__ offs, int32_t* __restrict__ out_size) {
  const int lane = threadIdx.x, f = blockIdx.x;
  const int32_t* l = lens + (size_t)f * n_int;
  int32_t* o = offs + (size_t)f * n_int;
  const int per = (n_int + 63) / 64;
  const int i0 = min(lane * per, n_int), i1 = min(i0 + per, n_int);
  int sum = 0;
  for (int i = i0; i < i1; ++i) sum += l[i];
  int incl = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  // interval i starts after the header, the intervals before it and their i RSTn markers
  int run = JPEG_HEADER_BYTES + incl - sum;
  for (int i = i0; i < i1; ++i) {
    o[i] = run + 2 * i;
    run += l[i];
  }
  if (lane == 63) out_size[f] = JPEG_HEADER_BYTES + incl + 2 * n_int;
}

__global__ __launch_bounds__(64) void jpeg_gather_kernel(const uint8_t* __restrict__ scratch, int slot,
                                                         const int32_t* __restrict__ lens,
                                                         const int32_t* __restrict__ offs, int n_int, JpegHeader hdr,
                                                         uint8_t* __restrict__ out, int64_t out_stride) {
  const int lane = threadIdx.x, i = blockIdx.x, f = blockIdx.y;
  const size_t k = (size_t)f * n_int + i;
  const int len = lens[k];
  const int64_t o = offs[k];
  const uint8_t* src = scratch + k * (size_t)slot;
  uint8_t* dst = out + (size_t)f * (size_t)out_stride;
  for (int j = lane; j < len; j += 64)
    if (o + j < out_stride) dst[o + j] = src[j];
  if (i == 0)
    for (int j = lane; j < JPEG_HEADER_BYTES; j += 64)
      if (j < out_stride) dst[j] = hdr.bytes[j];
  if (lane == 0 && i > 0 && o <= out_stride) {
    dst[o - 2] = 0xff;
    dst[o - 1] = (uint8_t)(0xd0 + ((i - 1) & 7));
  }
  if (lane == 0 && i == n_int - 1 && o + len + 2 <= out_stride) {
    dst[o + len] = 0xff;
    dst[o + len + 1] = 0xd9;
  }
}

// -------------------------------------------------------------------------------------------------- host
size_t jpeg_max_bytes(int H, int W, int ri) {
  if (H < 1 || W < 1 || H > 65535 || W > 65535 || ri < 1 || ri > JPEG_MAX_RI) return 0;
  return JPEG_HEADER_BYTES + (size_t)jpeg_n_intervals(H, W, ri) * (jpeg_slot_bytes(ri) + 2);
}

namespace {

struct JpegBufs {
  int16_t* coef;      // [n][n_mcu][6 blocks][64]
  uint8_t* scratch;   // [n][n_int] entropy-coded slots
  int32_t *lens, *offs;
};

JpegBufs jpeg_layout(Carver& c, int n, int H, int W, int ri) {
  const size_t n_int = (size_t)n * jpeg_n_intervals(H, W, ri);
  JpegBufs b;
  b.coef = c.take<int16_t>((size_t)n * jpeg_n_mcu(H, W) * 384);
  b.scratch = c.take<uint8_t>(n_int * jpeg_slot_bytes(ri));
  b.lens = c.take<int32_t>(n_int);
  b.offs = c.take<int32_t>(n_int);
  return b;
}

}  // namespace

size_t jpeg_workspace_bytes(int n, int H, int W, int ri) { return measure(jpeg_layout, n, H, W, ri); }

int jpeg_make_header(int H, int W, int quality, int ri, JpegHeader& hdr, JpegQuant& q) {
  if (quality < 1 || quality > 100) return -2;
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int n = 0; n < 64; ++n) {
      const int base = t ? K_Q_CHROMA[n] : K_Q_LUMA[n];
      const int Q = std::min(std::max((base * scale + 50) / 100, 1), 255);
      q.q[t][n] = (uint8_t)Q;
      q.recip[t][n] = (uint32_t)(((1u << 20) + Q - 1) / Q);
    }
  memset(&hdr, 0, sizeof(hdr));
  uint8_t* p = hdr.bytes;
  auto seg = [&](int marker, const uint8_t* payload, int len) {
    *p++ = 0xff;
    *p++ = (uint8_t)marker;
    *p++ = (uint8_t)((len + 2) >> 8);
    *p++ = (uint8_t)((len + 2) & 0xff);
    memcpy(p, payload, len);
    p += len;
  };
  *p++ = 0xff;
  *p++ = 0xd8;
  const uint8_t app0[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  seg(0xe0, app0, 14);
  for (int t = 0; t < 2; ++t) {
    uint8_t dqt[65];
    dqt[0] = (uint8_t)t;
    for (int k = 0; k < 64; ++k) dqt[1 + k] = q.q[t][K_ZIGZAG[k]];
    seg(0xdb, dqt, 65);
  }
  const uint8_t sof[15] = {8, (uint8_t)(H >> 8), (uint8_t)(H & 0xff), (uint8_t)(W >> 8), (uint8_t)(W & 0xff), 3, 1, 0x22, 0,
                           2, 0x11, 1, 3, 0x11, 1};
  seg(0xc0, sof, 15);
  const struct {
    int id;
    const uint8_t *bits, *vals;
    int n;
  } dht[4] = {{0x00, K_DC_L_BITS, K_DC_VALS, 12},
              {0x10, K_AC_L_BITS, K_AC_L_VALS, 162},
              {0x01, K_DC_C_BITS, K_DC_VALS, 12},
              {0x11, K_AC_C_BITS, K_AC_C_VALS, 162}};
  for (const auto& d : dht) {
    uint8_t buf[1 + 16 + 162];
    buf[0] = (uint8_t)d.id;
    memcpy(buf + 1, d.bits, 16);
    memcpy(buf + 17, d.vals, d.n);
    seg(0xc4, buf, 17 + d.n);
  }
  const uint8_t dri[2] = {(uint8_t)(ri >> 8), (uint8_t)(ri & 0xff)};
  seg(0xdd, dri, 2);
  const uint8_t sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  seg(0xda, sos, 10);
  return (p - hdr.bytes) == JPEG_HEADER_BYTES ? 0 : -1;
}

int jpeg_encode(const uint8_t* frames, int64_t frame_stride, int n, int H, int W, int ri, const JpegHeader& hdr,
                const JpegQuant& q, uint8_t* out, int64_t out_stride, int32_t* out_size, void* ws, size_t ws_bytes,
                hipStream_t s) {
  const int mcus_x = (W + 15) / 16;
  const int n_mcu = (int)jpeg_n_mcu(H, W), n_int = (int)jpeg_n_intervals(H, W, ri);
  const int slot = (int)jpeg_slot_bytes(ri);
  Carver c(ws, ws_bytes);
  const JpegBufs b = jpeg_layout(c, n, H, W, ri);
  if (!c.fits()) return -5;
  int16_t* coef = b.coef;
  uint8_t* scratch = b.scratch;
  int32_t *lens = b.lens, *offs = b.offs;

  const dim3 g_dct((n_mcu + DCT_MCUS - 1) / DCT_MCUS, n);
  // 16-byte loads when every row of every frame starts on a 16-byte boundary and holds whole MCUs
  const bool vec = W % 16 == 0 && frame_stride % 16 == 0 && (uintptr_t)frames % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(jpeg_dct_quant_kernel<true>, g_dct, dim3(64 * DCT_MCUS), 0, s, frames, frame_stride, H, W,
                       mcus_x, n_mcu, q, coef);
  else
    hipLaunchKernelGGL(jpeg_dct_quant_kernel<false>, g_dct, dim3(64 * DCT_MCUS), 0, s, frames, frame_stride, H, W,
                       mcus_x, n_mcu, q, coef);
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(n_int, n), dim3(64), 0, s, coef, n_mcu, ri, n_int, scratch, slot, lens);
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(n), dim3(64), 0, s, lens, n_int, offs, out_size);
  hipLaunchKernelGGL(jpeg_gather_kernel, dim3(n_int, n), dim3(64), 0, s, scratch, slot, lens, offs, n_int, hdr, out,
                     out_stride);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mq
