// The per-image and per-corner cores of the chessboard-corner detector (chessboard.hip): growing the 9 x 6 grid from
// corner candidates, its canonical order, and cornerSubPix.  Every function compiles for the host too
// (tests/chessboard_core_check.cpp runs them under the sanitizers); tests/chessboard_ref.py states the same in numpy.
//
// It replaces what the reference takes from OpenCV in analyze_chessboardvid (multicam_toolbox.py:22-72:
// cv2.findChessboardCorners :58, cv2.cornerSubPix :61).  OpenCV is not part of this project: the grid search is this
// project's own, and cornerSubPix is cv2's algorithm as documented, not pinned against cv2.
//
// The grid core is integer arithmetic on int32 candidate positions (products in int64: positions stay below 2^15, so
// the largest product, 4 (u.d)^2, stays below 2^63).  Every loop has a fixed bound and every index into the candidate
// and cell arrays is range-checked.
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define CB_HD __host__ __device__ inline
#else
#define CB_HD inline
#endif

namespace mq {

constexpr int CB_NC = 54;          // inner corners of the 9 x 6 pattern
constexpr int CB_FAST = 9, CB_SLOW = 6;
constexpr int CB_MAX_SEEDS = 54;
constexpr int CB_MAX_PASSES = 55;
constexpr int CB_OFF = 10;         // cells live in [-CB_OFF, CB_OFF]^2 around the seed
constexpr int CB_G = 2 * CB_OFF + 1;
constexpr int CB_MAX_CELLS = 55;   // growth stops once more than 54 are placed
constexpr int CB_MAX_K = 1024;     // most candidates per image any entry point accepts
constexpr int CB_GATE = 4;         // the grid uses the candidates with CB_GATE * R >= the strongest R
constexpr int CB_MAX_WIN = 16;     // largest cornerSubPix half-window

// The grid search is written for CB_LANES cooperating lanes that share one CbGrid: one wave on the device (a
// workgroup of exactly 64 threads), one thread on the host.  Control flow is uniform: every branch depends only on
// shared state and on reductions every lane receives.  Lane 0 alone writes the shared state, then all lanes meet.
constexpr int CB_LANES = 64;

CB_HD int cb_lane() {
#if defined(__HIP_DEVICE_COMPILE__)
  return (int)threadIdx.x;
#else
  return 0;
#endif
}
CB_HD int cb_stride() {
#if defined(__HIP_DEVICE_COMPILE__)
  return CB_LANES;
#else
  return 1;
#endif
}
CB_HD void cb_sync() {
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();
#endif
}
// smallest value over the lanes, the same in every lane
CB_HD int64_t cb_min64(int64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  for (int o = CB_LANES / 2; o > 0; o >>= 1) {
    const int64_t t = __shfl_xor((long long)v, o, CB_LANES);
    v = t < v ? t : v;
  }
#endif
  return v;
}
constexpr int64_t CB_NONE = INT64_MAX;

struct CbCell {
  int16_t i, j;
  int32_t c;
};

// Working state of one image's grid search (about 3 KB: LDS on the device, the stack on the host).
struct CbGrid {
  int32_t grid[CB_G * CB_G];   // candidate index per cell, -1 empty
  CbCell cells[CB_MAX_CELLS];
  uint8_t used[CB_MAX_K];
  int n_cells;
  int flag;
};

// the prefix of the (R descending) candidates the grid may use
CB_HD int cb_gated_count(const int32_t* resp, int count) {
  const int n = count < 0 ? 0 : (count > CB_MAX_K ? CB_MAX_K : count);
  const int64_t r0 = n > 0 ? resp[0] : 0;
  int64_t last = CB_NONE;  // minus (1 + the last index that passes the gate)
  for (int k = cb_lane(); k < n; k += cb_stride())
    if ((int64_t)CB_GATE * resp[k] >= r0 && -(int64_t)(k + 1) < last) last = -(int64_t)(k + 1);
  last = cb_min64(last);
  return last == CB_NONE ? 0 : (int)(-last);
}

// nearest candidate to (x, y) among [0, n) except `skip`; ties go to the lowest index
// (squared distances stay below 2^40 for positions below 2^15 and predictions within three times that; the key
// d2 * 1024 + index orders by distance, then index)
CB_HD int cb_nearest(const int32_t* pos, int n, int64_t x, int64_t y, int skip, int64_t* d2) {
  int64_t best = CB_NONE;
  for (int c = cb_lane(); c < n; c += cb_stride()) {
    if (c == skip) continue;
    const int64_t dx = pos[2 * c] - x, dy = pos[2 * c + 1] - y;
    const int64_t key = (dx * dx + dy * dy) * CB_MAX_K + c;
    best = key < best ? key : best;
  }
  best = cb_min64(best);
  if (best == CB_NONE) return -1;
  *d2 = best / CB_MAX_K;
  return (int)(best % CB_MAX_K);
}

// -2 outside the cell array (neither empty nor placed), -1 empty, else the candidate
CB_HD int cb_at(const CbGrid& g, int i, int j) {
  if (i < -CB_OFF || i > CB_OFF || j < -CB_OFF || j > CB_OFF) return -2;
  return g.grid[(j + CB_OFF) * CB_G + (i + CB_OFF)];
}

CB_HD bool cb_put(CbGrid& g, int n, int i, int j, int c) {
  if (i < -CB_OFF || i > CB_OFF || j < -CB_OFF || j > CB_OFF) return false;
  if (c < 0 || c >= n || c >= CB_MAX_K || g.n_cells >= CB_MAX_CELLS) return false;
  cb_sync();  // every lane has read n_cells
  if (cb_lane() == 0) {
    g.grid[(j + CB_OFF) * CB_G + (i + CB_OFF)] = c;
    g.used[c] = 1;
    g.cells[g.n_cells].i = (int16_t)i;
    g.cells[g.n_cells].j = (int16_t)j;
    g.cells[g.n_cells].c = c;
    ++g.n_cells;
  }
  cb_sync();
  return true;
}

// Grows the grid from seed s over candidates [0, n).  Returns the number of cells placed, or 0 when the seed is
// given up (no second axis, or more than 54 cells).  Collective over the lanes.
CB_HD int cb_grow(const int32_t* pos, int n, int s, CbGrid& g) {
  if (n > CB_MAX_K) n = CB_MAX_K;
  if (s < 0 || s >= n) return 0;
  cb_sync();
  for (int k = cb_lane(); k < CB_G * CB_G; k += cb_stride()) g.grid[k] = -1;
  for (int k = cb_lane(); k < n; k += cb_stride()) g.used[k] = 0;
  if (cb_lane() == 0) g.n_cells = 0;
  cb_sync();
  const int64_t sx = pos[2 * s], sy = pos[2 * s + 1];
  int64_t du = 0;
  const int a = cb_nearest(pos, n, sx, sy, s, &du);
  if (a < 0 || du == 0) return 0;
  const int64_t ux = pos[2 * a] - sx, uy = pos[2 * a + 1] - sy;
  int64_t bk = CB_NONE;
  for (int c = cb_lane(); c < n; c += cb_stride()) {
    if (c == s || c == a) continue;
    const int64_t dx = pos[2 * c] - sx, dy = pos[2 * c + 1] - sy;
    const int64_t dd = dx * dx + dy * dy, dot = ux * dx + uy * dy;
    if (dd == 0 || 4 * dot * dot >= 3 * du * dd) continue;  // within 30 degrees of +-u
    const int64_t key = dd * CB_MAX_K + c;
    bk = key < bk ? key : bk;
  }
  bk = cb_min64(bk);
  if (bk == CB_NONE) return 0;
  const int b = (int)(bk % CB_MAX_K);
  const int64_t dv = bk / CB_MAX_K;
  if (4 * dv > 25 * du) return 0;  // |v| > 2.5 |u|
  cb_put(g, n, 0, 0, s);
  cb_put(g, n, 1, 0, a);
  cb_put(g, n, 0, 1, b);
  const int DI[4] = {1, -1, 0, 0}, DJ[4] = {0, 0, 1, -1};
  for (int pass = 0; pass < CB_MAX_PASSES; ++pass) {
    const int snap = g.n_cells;
    for (int k = 0; k < snap && k < CB_MAX_CELLS; ++k) {
      const int i = g.cells[k].i, j = g.cells[k].j, c = g.cells[k].c;
      if (c < 0 || c >= n) return 0;
      const int64_t px = pos[2 * c], py = pos[2 * c + 1];
      for (int d = 0; d < 4; ++d) {
        const int di = DI[d], dj = DJ[d];
        if (cb_at(g, i + di, j + dj) != -1) continue;
        int64_t qx = 0, qy = 0;
        bool have = false;
        const int o = cb_at(g, i - di, j - dj);
        if (o >= 0 && o < n) {
          qx = 2 * px - pos[2 * o];
          qy = 2 * py - pos[2 * o + 1];
          have = true;
        } else {
          const int qi = dj < 0 ? -dj : dj, qj = di < 0 ? -di : di;
          for (int sg = 1; sg >= -1 && !have; sg -= 2) {
            const int q = cb_at(g, i + sg * qi, j + sg * qj);
            const int qd = cb_at(g, i + sg * qi + di, j + sg * qj + dj);
            if (q >= 0 && q < n && qd >= 0 && qd < n) {
              qx = px + pos[2 * qd] - pos[2 * q];
              qy = py + pos[2 * qd + 1] - pos[2 * q + 1];
              have = true;
            }
          }
        }
        if (!have) continue;
        const int64_t step = (qx - px) * (qx - px) + (qy - py) * (qy - py);
        if (step == 0) continue;
        int64_t d2 = 0;
        const int c2 = cb_nearest(pos, n, qx, qy, -1, &d2);
        if (c2 < 0 || g.used[c2] || 100 * d2 > 9 * step) continue;  // within 0.3 of the predicted step
        if (!cb_put(g, n, i + di, j + dj, c2)) continue;
        if (g.n_cells > CB_NC) return 0;
      }
    }
    if (g.n_cells == snap) break;
  }
  return g.n_cells;
}

// The 54 candidate indices in objp's order: 9 along the fast axis, 6 along the slow one, not mirrored
// (cross(c[1] - c[0], c[9] - c[0]) > 0 with y down), and of the two orders 180 degrees apart the one whose first
// corner has the smaller (y, x).  False when the cells are no complete 9 x 6 / 6 x 9 block.
CB_HD bool cb_canonical(const int32_t* pos, int n, const CbGrid& g, int32_t* order) {
  if (g.n_cells != CB_NC) return false;
  int i0 = CB_OFF, i1 = -CB_OFF, j0 = CB_OFF, j1 = -CB_OFF;
  for (int k = 0; k < CB_NC; ++k) {
    const int i = g.cells[k].i, j = g.cells[k].j;
    i0 = i < i0 ? i : i0;
    i1 = i > i1 ? i : i1;
    j0 = j < j0 ? j : j0;
    j1 = j > j1 ? j : j1;
  }
  const int ni = i1 - i0 + 1, nj = j1 - j0 + 1;
  const bool wide = ni == CB_FAST && nj == CB_SLOW;
  if (!wide && !(ni == CB_SLOW && nj == CB_FAST)) return false;
  int32_t t[CB_NC];
  for (int k = 0; k < CB_NC; ++k) t[k] = -1;
  for (int k = 0; k < CB_NC; ++k) {
    const int i = g.cells[k].i - i0, j = g.cells[k].j - j0, c = g.cells[k].c;
    const int r = wide ? j : i, f = wide ? i : j;
    if (r < 0 || r >= CB_SLOW || f < 0 || f >= CB_FAST || c < 0 || c >= n) return false;
    t[r * CB_FAST + f] = c;
  }
  for (int k = 0; k < CB_NC; ++k)
    if (t[k] < 0) return false;
  const int64_t ax = pos[2 * t[0]], ay = pos[2 * t[0] + 1];
  const int64_t cross = (pos[2 * t[1]] - ax) * (pos[2 * t[CB_FAST] + 1] - ay) -
                        (pos[2 * t[1] + 1] - ay) * (pos[2 * t[CB_FAST]] - ax);
  if (cross == 0) return false;
  const bool mirror = cross < 0;
  // after the un-mirroring, the first corner is t[0][mirror ? 8 : 0] and the last t[5][mirror ? 0 : 8]
  const int cf = t[mirror ? CB_FAST - 1 : 0], cl = t[(CB_SLOW - 1) * CB_FAST + (mirror ? 0 : CB_FAST - 1)];
  const int64_t fy = pos[2 * cf + 1], fx = pos[2 * cf], ly = pos[2 * cl + 1], lx = pos[2 * cl];
  const bool turn = ly < fy || (ly == fy && lx < fx);
  for (int r = 0; r < CB_SLOW; ++r)
    for (int f = 0; f < CB_FAST; ++f) {
      int rr = r, ff = mirror ? CB_FAST - 1 - f : f;
      if (turn) {
        rr = CB_SLOW - 1 - r;
        ff = CB_FAST - 1 - ff;
      }
      order[r * CB_FAST + f] = t[rr * CB_FAST + ff];
    }
  return true;
}

// Stages 4 and 5 of one image: seeds in candidate order.  Returns the seed that gave the board, or -1; order
// (54 candidate indices) is written when found.
CB_HD int cb_find_grid(const int32_t* pos, const int32_t* resp, int count, CbGrid& g, int32_t* order) {
  const int n = cb_gated_count(resp, count);
  if (n < CB_NC) return -1;
  for (int s = 0; s < n && s < CB_MAX_SEEDS; ++s) {
    if (cb_grow(pos, n, s, g) != CB_NC) continue;
    cb_sync();
    if (cb_lane() == 0) g.flag = cb_canonical(pos, n, g, order) ? 1 : 0;
    cb_sync();
    if (g.flag) return s;
  }
  return -1;
}

// detection pixel -> full-frame pixel
CB_HD double cb_full_res(int32_t p, double scale) { return (double)p / scale + (1.0 / scale - 1.0) / 2.0; }

// ----------------------------------------------------------------------------- cornerSubPix
// One corner is refined by CB_LANES cooperating lanes (one wave on the device; the host check runs the lanes one
// after another with the same partial sums and the same butterfly, so both add in the same order).

CB_HD int cb_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// cv2.getRectSubPix: sample `e` (row-major index) of the size x size patch centred on (cx, cy): bilinear,
// replicated border.  ix, iy = floor of the patch's top-left corner, fx, fy its fractions.
CB_HD double cb_patch_sample(const uint8_t* img, int h, int w, int ix, int iy, double fx, double fy, int size, int e) {
  const int r = e / size, c = e % size;
  const int x0 = cb_clampi(ix + c, w - 1), x1 = cb_clampi(ix + c + 1, w - 1);
  const int y0 = cb_clampi(iy + r, h - 1), y1 = cb_clampi(iy + r + 1, h - 1);
  const double t00 = img[(int64_t)y0 * w + x0], t01 = img[(int64_t)y0 * w + x1];
  const double t10 = img[(int64_t)y1 * w + x0], t11 = img[(int64_t)y1 * w + x1];
  const double top = t00 * (1.0 - fx) + t01 * fx;
  const double bot = t10 * (1.0 - fx) + t11 * fx;
  return top * (1.0 - fy) + bot * fy;
}

// where the patch starts; false when the centre is too far out for the int arithmetic (|c| > 2^24)
CB_HD bool cb_patch_origin(double cx, double cy, int size, int& ix, int& iy, double& fx, double& fy) {
  const double x0 = cx - (size - 1) * 0.5, y0 = cy - (size - 1) * 0.5;
  if (!(x0 > -16777216.0 && x0 < 16777216.0 && y0 > -16777216.0 && y0 < 16777216.0)) return false;
  const double flx = std::floor(x0), fly = std::floor(y0);
  ix = (int)flx;
  iy = (int)fly;
  fx = x0 - flx;
  fy = y0 - fly;
  return true;
}

// lane's share of the five sums over the (2 win + 1)^2 window: elements lane, lane + CB_LANES, ...
// patch is (2 win + 3)^2, wt[k] = exp(-((k - win) / win)^2).  acc = a, b, c, bb1, bb2.
CB_HD void cb_subpix_partial(const double* patch, const double* wt, int win, int lane, double acc[5]) {
  const int ww = 2 * win + 1, ps = ww + 2;
  for (int k = 0; k < 5; ++k) acc[k] = 0.0;
  for (int e = lane; e < ww * ww; e += CB_LANES) {
    const int i = e / ww, j = e % ww;
    const double m = wt[i] * wt[j];
    const double gx = patch[(i + 1) * ps + j + 2] - patch[(i + 1) * ps + j];
    const double gy = patch[(i + 2) * ps + j + 1] - patch[i * ps + j + 1];
    const double gxx = gx * gx * m, gxy = gx * gy * m, gyy = gy * gy * m;
    const double px = (double)(j - win), py = (double)(i - win);
    acc[0] += gxx;
    acc[1] += gxy;
    acc[2] += gyy;
    acc[3] += gxx * px + gxy * py;
    acc[4] += gxy * px + gyy * py;
  }
}

// One iteration's update from the reduced sums.  Returns true when the iteration loop ends.
CB_HD bool cb_subpix_step(const double s[5], double eps2, int w, int h, double& x, double& y) {
  const double a = s[0], b = s[1], c = s[2], bb1 = s[3], bb2 = s[4];
  const double det = a * c - b * b;
  const double tiny = 2.220446049250313e-16 * 2.220446049250313e-16;
  if (std::fabs(det) <= tiny || !(det == det)) return true;
  const double sc = 1.0 / det;
  const double nx = x + (c * sc * bb1 - b * sc * bb2);
  const double ny = y + (a * sc * bb2 - b * sc * bb1);
  const double err = (nx - x) * (nx - x) + (ny - y) * (ny - y);
  x = nx;
  y = ny;
  if (!(x >= 0.0 && x < (double)w && y >= 0.0 && y < (double)h)) return true;
  return err <= eps2;
}

// a corner that moved more than win in x or y returns to its start
CB_HD void cb_subpix_finish(double x0, double y0, int win, double& x, double& y) {
  if (!(std::fabs(x - x0) <= (double)win && std::fabs(y - y0) <= (double)win)) {
    x = x0;
    y = y0;
  }
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole refinement of one corner on the host, lane by lane: what one wave of corner_subpix_kernel does.
// patch: (2 win + 3)^2 doubles of scratch.
inline void cb_subpix_host(const uint8_t* img, int h, int w, int win, int max_iter, double eps, double* patch,
                           double& x, double& y) {
  if (!(x == x && y == y) || win < 1 || win > CB_MAX_WIN) return;
  double wt[2 * CB_MAX_WIN + 1];
  for (int k = 0; k <= 2 * win; ++k) {
    const double t = (double)(k - win) / (double)win;
    wt[k] = std::exp(-(t * t));
  }
  const int ps = 2 * win + 3;
  const double x0 = x, y0 = y;
  for (int it = 0; it < (max_iter > 1 ? max_iter : 1); ++it) {
    int ix, iy;
    double fx, fy;
    if (!cb_patch_origin(x, y, ps, ix, iy, fx, fy)) break;
    for (int e = 0; e < ps * ps; ++e) patch[e] = cb_patch_sample(img, h, w, ix, iy, fx, fy, ps, e);
    double part[CB_LANES][5];
    for (int l = 0; l < CB_LANES; ++l) cb_subpix_partial(patch, wt, win, l, part[l]);
    for (int o = CB_LANES / 2; o > 0; o >>= 1) {  // the wave's xor butterfly
      double nxt[CB_LANES][5];
      for (int l = 0; l < CB_LANES; ++l)
        for (int k = 0; k < 5; ++k) nxt[l][k] = part[l][k] + part[l ^ o][k];
      for (int l = 0; l < CB_LANES; ++l)
        for (int k = 0; k < 5; ++k) part[l][k] = nxt[l][k];
    }
    if (cb_subpix_step(part[0], eps * eps, w, h, x, y)) break;
  }
  cb_subpix_finish(x0, y0, win, x, y);
}
#endif

}  // namespace mq
