// Host check program of the baseline JPEG decoder: csrc/jpeg_parse.cpp and the per-interval body of
// csrc/jpeg_dec_dev.hpp, compiled for the CPU (tests/test_jpeg_dec_host.py builds it with the address and
// undefined-behaviour sanitizers and runs it on valid, truncated and mutated streams).
//
//   jpeg_dec_check <records>     records: repeated [uint32 little-endian length][bytes]
//
// One line per record: "<parse code> <status> <sum of (2 i + 1) * uint16(coef[i]) mod 2^64> <long codes>", status -1 when
// the header was refused and -2 when the frame has more than 65536 blocks (a mutated size; not decoded here).
// Each stream is copied into an allocation of exactly its length, so a read past its end is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jpeg_dec_dev.hpp"

using namespace mq;

// tests/jpeg_dec_ref.py intervals(): the sequential statement of jpeg_dec_markers_kernel
static bool find_intervals(const uint8_t* d, int64_t n, int64_t scan_offset, int64_t want, std::vector<int64_t>& ends) {
  ends.clear();
  for (int64_t p = scan_offset; p + 1 < n;) {
    if (d[p] != 0xff) {
      ++p;
      continue;
    }
    const int m = d[p + 1];
    if (m == 0xd9 || (m >= 0xd0 && m <= 0xd7)) {
      const int64_t k = (int64_t)ends.size();
      if (k >= want || m != (k == want - 1 ? 0xd9 : 0xd0 + (int)(k & 7))) return false;
      ends.push_back(p);
      if (m == 0xd9) return true;
      p += 2;
    } else {
      ++p;
    }
  }
  return false;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  JpegDecTables* T = new JpegDecTables;
  for (;;) {
    uint8_t lb[4];
    if (fread(lb, 1, 4, f) != 4) break;
    const uint32_t len = lb[0] | (lb[1] << 8) | (lb[2] << 16) | ((uint32_t)lb[3] << 24);
    uint8_t* d = (uint8_t*)malloc(len ? len : 1);
    if (len && fread(d, 1, len, f) != len) return 2;
    mq_jpeg_info info;
    const int rc = mq_jpeg_parse(len ? d : nullptr, len, &info);
    int status = -1;
    uint64_t hash = 0;
    uint32_t long_codes = 0;
    if (rc == 0) {
      const JpegDecShape shape = jpeg_dec_shape(info);
      const int h = info.n_comp == 3 ? info.h_luma : 1, v = info.n_comp == 3 ? info.v_luma : 1;
      const int64_t n_mcu = (int64_t)((info.width + 8 * h - 1) / (8 * h)) * ((info.height + 8 * v - 1) / (8 * v));
      if (n_mcu * shape.n_blocks > 65536) {
        status = -2;
      } else {
        const int64_t ri = info.restart_interval ? info.restart_interval : n_mcu;
        const int64_t n_int = (n_mcu + ri - 1) / ri;
        std::vector<int64_t> ends;
        if (!find_intervals(d, len, info.scan_offset, n_int, ends)) {
          status = JPEG_ST_MARKERS;
        } else {
          for (int t = 0; t < 4; ++t) jpeg_dec_build_table(info, T, t);
          jpeg_dec_zigzag(T->zigzag);
          std::vector<int16_t> coef((size_t)(n_mcu * shape.n_blocks * 64), 0);
          status = 0;
          for (int64_t i = 0; i < n_int; ++i) {
            const int64_t begin = i == 0 ? info.scan_offset : ends[i - 1] + 2;
            const int64_t m0 = i * ri;
            const int st = jpeg_dec_interval(d, begin, ends[i], T, shape, (int)(ri < n_mcu - m0 ? ri : n_mcu - m0),
                                             coef.data() + m0 * shape.n_blocks * 64, &long_codes);
            if (st > status) status = st;
          }
          for (size_t i = 0; i < coef.size(); ++i) hash += (uint64_t)(uint16_t)coef[i] * (2 * (uint64_t)i + 1);
          // the IDCT on whatever the stream produced: its arithmetic has to be defined (it wraps)
          int32_t sink = 0;
          for (size_t b = 0; b < coef.size() / 64; ++b) {
            const int blk = (int)(b % shape.n_blocks);
            const int comp = blk < shape.n_luma ? 0 : blk - shape.n_luma + 1;
            int32_t mid[64];
            for (int x = 0; x < 8; ++x) {
              int32_t in[8], out[8];
              for (int y = 0; y < 8; ++y) in[y] = (int32_t)coef[b * 64 + y * 8 + x] * (int32_t)info.quant[comp][y * 8 + x];
              jpeg_idct_islow_1d<11>(in, out);
              for (int y = 0; y < 8; ++y) mid[y * 8 + x] = out[y];
            }
            for (int y = 0; y < 8; ++y) {
              int32_t out[8];
              jpeg_idct_islow_1d<18>(mid + y * 8, out);
              for (int k = 0; k < 8; ++k) sink ^= out[k];
            }
          }
          if (sink == 0x7fffffff) fputc(' ', stderr);  // keeps the loop alive
        }
      }
    }
    printf("%d %d %016llx %u\n", rc, status, (unsigned long long)hash, long_codes);
    free(d);
  }
  delete T;
  fclose(f);
  return 0;
}
