// Host parser of a baseline JPEG header (mq_jpeg_parse, include/mq_hip.h).  Plain C++, no HIP include: the host
// compiler builds it alone.  tests/jpeg_dec_ref.py parse() is the restatement, equal field by field and code by code;
// the checks are made in the same order there.  Every read is bounded by `size`.
#include <string.h>

#include "mq_hip.h"

static_assert(sizeof(mq_jpeg_info) == 1320, "mq_jpeg_info is passed to kernels by value: keep it small and fixed");

namespace {

constexpr uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.3 - K.6 (what a stream without DHT means)
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

void set_huff(mq_jpeg_huff& h, const uint8_t* bits, const uint8_t* vals, int n) {
  memset(&h, 0, sizeof(h));
  memcpy(h.bits, bits, 16);
  memcpy(h.vals, vals, (size_t)n);
}

// a prefix code: at most 256 symbols, and the canonical code never outgrows its length
bool huff_ok(const uint8_t* bits, const uint8_t* vals, int n, bool dc) {
  uint32_t code = 0;
  for (int len = 1; len <= 16; ++len) {
    code += bits[len - 1];
    if (code > (1u << len)) return false;
    code <<= 1;
  }
  if (dc)
    for (int i = 0; i < n; ++i)
      if (vals[i] > 15) return false;
  return true;
}

struct Comp {
  int id, h, v, tq;
};

}  // namespace

extern "C" int mq_jpeg_parse(const uint8_t* d, int64_t n, mq_jpeg_info* out) {
  if (!out) return -1;
  memset(out, 0, sizeof(*out));
  if (!d || n < 2 || d[0] != 0xff || d[1] != 0xd8) return MQ_JPEG_E_NOT_JPEG;
  mq_jpeg_info info;
  memset(&info, 0, sizeof(info));
  uint8_t qt[4][64];
  bool have_qt[4] = {false, false, false, false};
  mq_jpeg_huff dht[2][2];
  bool have_dht[2][2] = {{false, false}, {false, false}};
  bool any_dht = false, have_sof = false;
  int adobe = -1;
  Comp comps[3] = {};
  int64_t pos = 2;
  for (;;) {
    if (pos + 4 > n) return MQ_JPEG_E_TRUNCATED;
    if (d[pos] != 0xff) return MQ_JPEG_E_NOT_JPEG;
    const int m = d[pos + 1];
    if (m == 0xff) {  // fill byte
      ++pos;
      continue;
    }
    const int64_t seglen = ((int64_t)d[pos + 2] << 8) | d[pos + 3];
    if (seglen < 2 || pos + 2 + seglen > n) return MQ_JPEG_E_TRUNCATED;
    const uint8_t* p = d + pos + 4;
    const int len = (int)seglen - 2;
    pos += 2 + seglen;
    if (m == 0xc0) {
      if (have_sof) return MQ_JPEG_E_SOF;
      if (len < 6) return MQ_JPEG_E_TRUNCATED;
      if (p[0] != 8) return MQ_JPEG_E_PRECISION;
      info.height = (p[1] << 8) | p[2];
      info.width = (p[3] << 8) | p[4];
      const int nc = p[5];
      if (nc != 1 && nc != 3) return MQ_JPEG_E_COMPONENTS;
      if (len != 6 + 3 * nc) return MQ_JPEG_E_TRUNCATED;
      if (info.height == 0 || info.width == 0) return MQ_JPEG_E_SIZE;
      for (int c = 0; c < nc; ++c) comps[c] = {p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c]};
      info.n_comp = nc;
      have_sof = true;
    } else if (m >= 0xc1 && m <= 0xcf && m != 0xc4 && m != 0xc8) {
      return MQ_JPEG_E_SOF;
    } else if (m == 0xdb) {
      int k = 0;
      while (k < len) {
        if ((p[k] >> 4) || (p[k] & 15) > 3) return MQ_JPEG_E_DQT;
        if (k + 65 > len) return MQ_JPEG_E_TRUNCATED;
        const int id = p[k] & 15;
        for (int z = 0; z < 64; ++z) qt[id][ZIGZAG[z]] = p[k + 1 + z];
        have_qt[id] = true;
        k += 65;
      }
    } else if (m == 0xc4) {
      int k = 0;
      while (k < len) {
        if (k + 17 > len) return MQ_JPEG_E_TRUNCATED;
        const int tc = p[k] >> 4, th = p[k] & 15;
        int count = 0;
        for (int i = 0; i < 16; ++i) count += p[k + 1 + i];
        if (tc > 1 || th > 1 || count > 256) return MQ_JPEG_E_HUFFMAN;
        if (k + 17 + count > len) return MQ_JPEG_E_TRUNCATED;
        if (!huff_ok(p + k + 1, p + k + 17, count, tc == 0)) return MQ_JPEG_E_HUFFMAN;
        set_huff(dht[tc][th], p + k + 1, p + k + 17, count);
        have_dht[tc][th] = any_dht = true;
        k += 17 + count;
      }
    } else if (m == 0xdd) {
      if (len != 2) return MQ_JPEG_E_TRUNCATED;
      info.restart_interval = (p[0] << 8) | p[1];
    } else if (m == 0xee && len >= 12 && memcmp(p, "Adobe", 5) == 0) {
      adobe = p[11];
    } else if (m == 0xda) {
      if (!have_sof) return MQ_JPEG_E_SOF;
      if (len < 1 || len != 4 + 2 * p[0]) return MQ_JPEG_E_TRUNCATED;
      if (p[0] != info.n_comp) return MQ_JPEG_E_SCANS;
      for (int c = 0; c < info.n_comp; ++c) {
        if (p[1 + 2 * c] != comps[c].id) return MQ_JPEG_E_SCANS;
        info.dc_sel[c] = p[2 + 2 * c] >> 4;
        info.ac_sel[c] = p[2 + 2 * c] & 15;
      }
      const uint8_t* t = p + 1 + 2 * info.n_comp;
      if (t[0] != 0 || t[1] != 63 || t[2] != 0) return MQ_JPEG_E_SCANS;
      break;
    } else if (m == 0xd8 || m == 0xd9 || (m >= 0xd0 && m <= 0xd7) || m == 0x01 || m == 0x00) {
      return MQ_JPEG_E_NOT_JPEG;
    }
    // APPn, COM, anything else with a length: skipped
  }
  if (info.n_comp == 3) {
    if (adobe >= 0 && adobe != 1) return MQ_JPEG_E_COMPONENTS;
    if (comps[1].h != 1 || comps[1].v != 1 || comps[2].h != 1 || comps[2].v != 1) return MQ_JPEG_E_SAMPLING;
    const int h = comps[0].h, v = comps[0].v;
    if (!((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2))) return MQ_JPEG_E_SAMPLING;
    info.h_luma = h;
    info.v_luma = v;
  } else {
    info.h_luma = info.v_luma = 1;  // a single component is never interleaved: its factors do not matter
  }
  if (!any_dht) {
    set_huff(dht[0][0], K_DC_L_BITS, K_DC_VALS, 12);
    set_huff(dht[0][1], K_DC_C_BITS, K_DC_VALS, 12);
    set_huff(dht[1][0], K_AC_L_BITS, K_AC_L_VALS, 162);
    set_huff(dht[1][1], K_AC_C_BITS, K_AC_C_VALS, 162);
    have_dht[0][0] = have_dht[0][1] = have_dht[1][0] = have_dht[1][1] = true;
  }
  for (int c = 0; c < info.n_comp; ++c) {
    if (comps[c].tq > 3 || !have_qt[comps[c].tq] || info.dc_sel[c] > 1 || info.ac_sel[c] > 1 ||
        !have_dht[0][info.dc_sel[c]] || !have_dht[1][info.ac_sel[c]])
      return MQ_JPEG_E_TABLE;
    memcpy(info.quant[c], qt[comps[c].tq], 64);
  }
  for (int t = 0; t < 2; ++t) {
    if (have_dht[0][t]) info.dc[t] = dht[0][t];
    if (have_dht[1][t]) info.ac[t] = dht[1][t];
  }
  info.scan_offset = pos;
  for (;;) {  // the scan: only stuffing, fill bytes and RSTn up to the first EOI
    const void* f = pos < n ? memchr(d + pos, 0xff, (size_t)(n - pos)) : nullptr;
    if (!f) return MQ_JPEG_E_NO_EOI;
    pos = (const uint8_t*)f - d;
    if (pos + 1 >= n) return MQ_JPEG_E_NO_EOI;
    const int m = d[pos + 1];
    if (m == 0xd9) break;
    if (m == 0xff)
      pos += 1;
    else if (m == 0 || (m >= 0xd0 && m <= 0xd7))
      pos += 2;
    else
      return MQ_JPEG_E_SCANS;
  }
  *out = info;
  return 0;
}
