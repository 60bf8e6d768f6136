// Host run of csrc/chessboard_dev.hpp (the grid search with its canonical order, and cornerSubPix) on cases that
// tests/test_chessboard_ref.py writes out; built with -fsanitize=address,undefined and run directly.  No GPU.
//   in:  grid <count> then count x "x y r"                      out: grid <seed> <54 candidate indices, or none>
//        subpix <h> <w> <win> <max_iter> <eps> <raw image file> <n> then n x "x y"
//                                                               out: subpix <n x "x y" as %.17g>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "chessboard_dev.hpp"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: chessboard_core_check <in> <out>\n");
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
    if (kind == "grid") {
      int count = 0;
      ss >> count;
      if (count < 0 || count > mq::CB_MAX_K) return 3;
      std::vector<int32_t> pos(2 * (size_t)count), val((size_t)count);   // exact sizes: ASan sees any overrun
      for (int k = 0; k < count; ++k) ss >> pos[2 * k] >> pos[2 * k + 1] >> val[k];
      if (!ss) return 3;
      auto* g = new mq::CbGrid;
      int32_t order[mq::CB_NC];
      const int seed = mq::cb_find_grid(pos.data(), val.data(), count, *g, order);
      delete g;
      std::fprintf(out, "grid %d", seed);
      if (seed >= 0)
        for (int k = 0; k < mq::CB_NC; ++k) std::fprintf(out, " %d", order[k]);
      std::fprintf(out, "\n");
    } else if (kind == "subpix") {
      int h = 0, w = 0, win = 0, max_iter = 0, n = 0;
      double eps = 0;
      std::string path;
      ss >> h >> w >> win >> max_iter >> eps >> path >> n;
      if (!ss || h < 1 || w < 1 || win < 1 || win > mq::CB_MAX_WIN || n < 0) return 3;
      std::vector<uint8_t> img((size_t)h * w);
      FILE* f = std::fopen(path.c_str(), "rb");
      if (!f || std::fread(img.data(), 1, img.size(), f) != img.size()) return 3;
      std::fclose(f);
      std::vector<double> patch((size_t)(2 * win + 3) * (2 * win + 3));
      std::fprintf(out, "subpix");
      for (int k = 0; k < n; ++k) {
        double x = 0, y = 0;
        ss >> x >> y;
        if (!ss) return 3;
        mq::cb_subpix_host(img.data(), h, w, win, max_iter, eps, patch.data(), x, y);
        std::fprintf(out, " %.17g %.17g", x, y);
      }
      std::fprintf(out, "\n");
    } else if (!kind.empty()) {
      return 3;
    }
  }
  std::fclose(out);
  return 0;
}
