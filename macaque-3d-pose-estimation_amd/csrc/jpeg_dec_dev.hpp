// The sequential core of the baseline JPEG decoder (mq_jpeg_decode, include/mq_hip.h): decoding tables, the bit
// reader and the per-restart-interval entropy decode, as plain inline C++ on raw pointers.  csrc/jpeg_dec.hip runs
// one lane per interval with the tables in LDS; a host program compiles the same text with the tables in an array
// (tests/jpeg_dec_check.cpp, under the address and undefined-behaviour sanitizers).  tests/jpeg_dec_ref.py restates it.
//
// Defined for any input bits: every read of `src` lies in [begin, end), every coefficient index in [0, 63], every
// table index inside its table, and no signed arithmetic can overflow.
#pragma once
#include <stdint.h>

#include "mq_hip.h"

#if defined(__HIPCC__)
#define MQ_JPEG_HD __host__ __device__ inline
#else
#define MQ_JPEG_HD inline
#endif

namespace mq {

constexpr int JPEG_DEC_LOOK_BITS = 9;  // first-level lookup; longer codes take the maxcode walk
enum { JPEG_ST_OK = 0, JPEG_ST_MARKERS = 1, JPEG_ST_NO_CODE = 2, JPEG_ST_RUN = 3, JPEG_ST_EXHAUSTED = 4 };

// Table t: 0, 1 the DC tables, 2, 3 the AC tables.
struct JpegDecTables {
  uint16_t look[4][1 << JPEG_DEC_LOOK_BITS];  // (length << 8) | symbol of the code the next 9 bits start with, or 0
  int32_t maxcode[4][18];                     // largest code of a length, -1 if it has none
  int32_t valoff[4][18];                      // index of a length's first symbol less its first code
  uint8_t vals[4][256];
  uint8_t zigzag[64];                         // natural index of the k-th coefficient of the scan
};

// Blocks of one MCU: luma first (row-major), then Cb, Cr.
struct JpegDecShape {
  int n_blocks, n_luma;
  uint8_t dc_tab[3], ac_tab[3];  // table t per component
};

MQ_JPEG_HD JpegDecShape jpeg_dec_shape(const mq_jpeg_info& info) {
  JpegDecShape s;
  s.n_luma = info.n_comp == 3 ? info.h_luma * info.v_luma : 1;
  s.n_blocks = info.n_comp == 3 ? s.n_luma + 2 : 1;
  for (int c = 0; c < 3; ++c) {
    s.dc_tab[c] = (uint8_t)(info.dc_sel[c] & 1);
    s.ac_tab[c] = (uint8_t)(2 + (info.ac_sel[c] & 1));
  }
  return s;
}

// Build table t (0..3) of T.  Canonical codes, Annex C; bounded for any bits[] (the parser already refuses what is
// no prefix code).
MQ_JPEG_HD void jpeg_dec_build_table(const mq_jpeg_info& info, JpegDecTables* T, int t) {
  const mq_jpeg_huff& h = t < 2 ? info.dc[t] : info.ac[t - 2];
  constexpr int N = 1 << JPEG_DEC_LOOK_BITS;
  for (int e = 0; e < N; ++e) T->look[t][e] = 0;
  for (int i = 0; i < 256; ++i) T->vals[t][i] = h.vals[i];
  T->maxcode[t][0] = T->maxcode[t][17] = -1;
  T->valoff[t][0] = T->valoff[t][17] = 0;
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    T->valoff[t][len] = k - (int32_t)code;
    const int cnt = h.bits[len - 1];
    for (int i = 0; i < cnt; ++i) {
      if (len <= JPEG_DEC_LOOK_BITS && k < 256) {
        const uint32_t lo = code << (JPEG_DEC_LOOK_BITS - len);
        for (uint32_t e = lo; e < lo + (1u << (JPEG_DEC_LOOK_BITS - len)) && e < (uint32_t)N; ++e)
          T->look[t][e] = (uint16_t)((len << 8) | h.vals[k]);
      }
      ++code;
      ++k;
    }
    T->maxcode[t][len] = cnt ? (int32_t)code - 1 : -1;
    code <<= 1;  // at most 255 * 2^16 + ...: no overflow of 32 bits
  }
}

MQ_JPEG_HD void jpeg_dec_zigzag(uint8_t* zz) {
  // walk the anti-diagonals: up-right on even sums, down-left on odd ones
  int k = 0;
  for (int s = 0; s < 15; ++s)
    for (int i = 0; i <= s; ++i) {
      const int u = (s & 1) ? i : s - i, v = s - u;
      if (u < 8 && v < 8) zz[k++] = (uint8_t)(u * 8 + v);
    }
}

// MSB-first bit reader over src[p, end) with FF 00 -> FF.  `acc` holds `cnt` valid bits at its top, zeros below.
// Bytes are loaded one at a time (DESIGN.md section 3.8 on why not more).
struct JpegBitReader {
  const uint8_t* src;
  int64_t p, end;
  uint64_t acc;
  int cnt;
};

MQ_JPEG_HD void jpeg_br_fill(JpegBitReader& r) {
  while (r.cnt <= 56 && r.p < r.end) {
    const uint32_t b = r.src[r.p++];
    if (b == 0xffu && r.p < r.end && r.src[r.p] == 0) ++r.p;
    r.acc |= (uint64_t)b << (56 - r.cnt);
    r.cnt += 8;
  }
}
MQ_JPEG_HD uint32_t jpeg_br_peek16(const JpegBitReader& r) { return (uint32_t)(r.acc >> 48); }
MQ_JPEG_HD void jpeg_br_skip(JpegBitReader& r, int n) {  // 0 <= n <= min(cnt, 16)
  r.acc <<= n;
  r.cnt -= n;
}

// Decode `n_mcus` MCUs of one restart interval, src[begin, end), into coef[(mcu * n_blocks + block) * 64 + natural]
// (int16, zeroed by the caller: only non-zero values are written).  Returns the interval's status.
MQ_JPEG_HD int jpeg_dec_interval(const uint8_t* src, int64_t begin, int64_t end, const JpegDecTables* T,
                                 const JpegDecShape& shape, int n_mcus, int16_t* coef, uint32_t* long_codes) {
  JpegBitReader r{src, begin, end, 0, 0};
  int pred[3] = {0, 0, 0};
  for (int m = 0; m < n_mcus; ++m) {
    for (int b = 0; b < shape.n_blocks; ++b) {
      const int comp = b < shape.n_luma ? 0 : b - shape.n_luma + 1;
      int16_t* out = coef + ((int64_t)m * shape.n_blocks + b) * 64;
      int k = 0;
      while (k < 64) {
        const int t = k == 0 ? shape.dc_tab[comp] : shape.ac_tab[comp];
        jpeg_br_fill(r);  // a symbol takes at most 16 + 15 bits: after this, cnt < 31 only at the interval's end
        const uint32_t v = jpeg_br_peek16(r);
        const uint32_t e = T->look[t][v >> (16 - JPEG_DEC_LOOK_BITS)];
        int len = (int)(e >> 8), sym = (int)(e & 255u);
        if (!e) {
          len = 0;
          for (int ln = JPEG_DEC_LOOK_BITS + 1; ln <= 16; ++ln) {
            const int32_t c = (int32_t)(v >> (16 - ln));
            if (c <= T->maxcode[t][ln]) {
              len = ln;
              sym = T->vals[t][(T->valoff[t][ln] + c) & 255];
              break;
            }
          }
          if (!len) return r.cnt < 16 ? JPEG_ST_EXHAUSTED : JPEG_ST_NO_CODE;
          if (long_codes) ++*long_codes;
        }
        if (len > r.cnt) return JPEG_ST_EXHAUSTED;
        jpeg_br_skip(r, len);
        const int s = sym & 15;
        if (s > r.cnt) return JPEG_ST_EXHAUSTED;
        const int bits = s ? (int)(jpeg_br_peek16(r) >> (16 - s)) : 0;
        jpeg_br_skip(r, s);
        const int val = s && bits < (1 << (s - 1)) ? bits - (1 << s) + 1 : bits;  // |val| < 2^15
        if (k == 0) {
          pred[comp] = (int16_t)(uint16_t)(uint32_t)(pred[comp] + val);  // int16, wrapping
          if (pred[comp]) out[0] = (int16_t)pred[comp];
          k = 1;
          continue;
        }
        const int run = sym >> 4;
        if (s == 0) {
          if (run != 15) break;  // EOB
          k += 16;
          if (k > 64) return JPEG_ST_RUN;
          continue;
        }
        k += run;
        if (k > 63) return JPEG_ST_RUN;
        out[T->zigzag[k]] = (int16_t)val;
        ++k;
      }
    }
  }
  return JPEG_ST_OK;
}

// ---------------------------------------------------------------------------------------------------- IDCT
// One pass of libjpeg's jpeg_idct_islow on eight inputs: out[i] = (sum_i + (1 << (SHIFT - 1))) >> SHIFT, in unsigned
// 32-bit arithmetic that wraps; the shift is arithmetic on the wrapped value.
template <int SHIFT>
MQ_JPEG_HD void jpeg_idct_islow_1d(const int32_t in[8], int32_t out[8]) {
  const uint32_t i0 = (uint32_t)in[0], i1 = (uint32_t)in[1], i2 = (uint32_t)in[2], i3 = (uint32_t)in[3],
                 i4 = (uint32_t)in[4], i5 = (uint32_t)in[5], i6 = (uint32_t)in[6], i7 = (uint32_t)in[7];
  uint32_t z1 = (i2 + i6) * 4433u;
  const uint32_t tmp2 = z1 - i6 * 15137u, tmp3 = z1 + i2 * 6270u;
  const uint32_t tmp0 = (i0 + i4) << 13, tmp1 = (i0 - i4) << 13;
  const uint32_t t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
  uint32_t t0 = i7, t1 = i5, t2 = i3, t3 = i1;
  z1 = t0 + t3;
  uint32_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  t0 *= 2446u;
  t1 *= 16819u;
  t2 *= 25172u;
  t3 *= 12299u;
  z1 = 0u - z1 * 7373u;
  z2 = 0u - z2 * 20995u;
  z3 = z5 - z3 * 16069u;
  z4 = z5 - z4 * 3196u;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  constexpr uint32_t R = 1u << (SHIFT - 1);
  out[0] = (int32_t)(t10 + t3 + R) >> SHIFT;
  out[7] = (int32_t)(t10 - t3 + R) >> SHIFT;
  out[1] = (int32_t)(t11 + t2 + R) >> SHIFT;
  out[6] = (int32_t)(t11 - t2 + R) >> SHIFT;
  out[2] = (int32_t)(t12 + t1 + R) >> SHIFT;
  out[5] = (int32_t)(t12 - t1 + R) >> SHIFT;
  out[3] = (int32_t)(t13 + t0 + R) >> SHIFT;
  out[4] = (int32_t)(t13 - t0 + R) >> SHIFT;
}

}  // namespace mq
