// Host run of csrc/aruco_dev.hpp (the per-quad core: quad choice, sub-pixel sides, cells, border test, dictionary
// match) on cases that tests/test_aruco_ref.py writes out; built with -fsanitize=address,undefined and run directly.
// No GPU.
//   in:  quads <h> <w> <raw image file> <max_correction_bits> <border_errors> <n_codes> <codes...> <count>
//        <max_quads> then min(count, max_quads) x 16 candidate fields        (n_codes -1: no dictionary)
//   out: quads then per processed candidate "ok id rot code" and 8 corner coordinates as %.17g
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "aruco_dev.hpp"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: aruco_core_check <in> <out>\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  FILE* out = std::fopen(argv[2], "w");
  if (!in || !out) return 2;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string kind;
    ss >> kind;
    if (kind == "quads") {
      int h = 0, w = 0, corr = 0, berr = 0, n_codes = 0, count = 0, max_quads = 0;
      std::string path;
      ss >> h >> w >> path >> corr >> berr >> n_codes;
      if (!ss || h < 1 || w < 1 || n_codes < -1 || n_codes > mq::AR_MAX_CODES) return 3;
      std::vector<uint16_t> dict((size_t)(n_codes > 0 ? n_codes : 0));   // exact sizes: ASan sees any overrun
      for (auto& c : dict) {
        int v = 0;
        ss >> v;
        c = (uint16_t)v;
      }
      ss >> count >> max_quads;
      if (!ss || count < 0 || max_quads < 1 || max_quads > mq::AR_MAX_QUADS) return 3;
      const int n = count < max_quads ? count : max_quads;
      std::vector<int32_t> cand((size_t)n * mq::AR_CAND);
      for (auto& v : cand) ss >> v;
      if (!ss) return 3;
      std::vector<uint8_t> img((size_t)h * w);
      FILE* f = std::fopen(path.c_str(), "rb");
      if (!f || std::fread(img.data(), 1, img.size(), f) != img.size()) return 3;
      std::fclose(f);
      std::fprintf(out, "quads");
      for (int k = 0; k < n; ++k) {
        mq::ArQuad q;
        mq::ar_quad_host(img.data(), h, w, cand.data() + (size_t)k * mq::AR_CAND, n_codes >= 0 ? dict.data() : nullptr,
                         n_codes > 0 ? n_codes : 0, corr, berr, q);
        std::fprintf(out, " %d %d %d %d", q.ok, q.id, q.rot, q.code);
        for (int e = 0; e < 8; ++e) std::fprintf(out, " %.17g", q.c[e]);
      }
      std::fprintf(out, "\n");
    } else if (!kind.empty()) {
      return 3;
    }
  }
  std::fclose(out);
  return 0;
}
