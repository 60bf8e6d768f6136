// The per-quad core of the ArUco-marker detector (aruco.hip): from a component's extreme pixels to a quad, its
// sub-pixel corners, the 6 x 6 cells, the border test and the dictionary match.  Every function compiles for the host
// too (tests/aruco_core_check.cpp runs them under the sanitizers); tests/aruco_ref.py states the same in numpy.
//
// It replaces what the reference takes from OpenCV in analyze_aruco_marker_vid / analyze_aruco_cube_vid
// (multicam_toolbox.py:244-391: aruco.detectMarkers :283, :356).  OpenCV is not part of this project: the detector
// is this project's own, for 4 x 4 codes given by the caller, and is not pinned against cv2.aruco.
//
// One quad is worked on by AR_LANES cooperating lanes (one wave on the device; the host runs the lanes one after
// another with the same partial sums and the same butterfly, so both add in the same order).  float64, compiled
// without FMA contraction.  Every loop has a fixed bound and every image read is clamped to the image.
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define AR_HD __host__ __device__ inline
#else
#define AR_HD inline
#endif

namespace mq {

constexpr int AR_LANES = 64;
constexpr int AR_THR_R = 11;         // half window of the adaptive threshold
constexpr int AR_THR_C = 7;          // its constant
constexpr int AR_MIN_AREA = 100;     // dark pixels of a component
constexpr int AR_MIN_BOX = 12;       // bounding-box side
constexpr int AR_MAX_QUADS = 64;     // candidates per image any entry point accepts
constexpr int AR_MAX_CODES = 1024;   // dictionary entries
constexpr int AR_CAND = 16;          // int32 per candidate: label, area, x0, y0, x1, y1, 8 extremes, 2 spare
constexpr int AR_MIN_SIDE = 10;      // pixels between adjacent corners
constexpr int AR_FILL_LO_N = 1, AR_FILL_LO_D = 16;  // component area / quad area >= 1 / 16 (a hollowed outline)
constexpr int AR_FILL_HI_N = 5, AR_FILL_HI_D = 4;   // ... <= 5 / 4
constexpr int AR_N_PROF = 16;        // profiles per side: 4 sides x 16 = one per lane
constexpr int AR_PROF_N = 13;        // samples per profile, from -3 to +3 px in steps of 0.5
constexpr double AR_MIN_EDGE = 20.0;
constexpr int AR_MIN_PROFILES = 8;
constexpr double AR_MAX_MOVE = 4.0;
constexpr double AR_MIN_CONTRAST = 30.0;

// the eight directions x, x+y, y, y-x, -x, -x-y, -y, x-y; the diagonal set clockwise from the top-left and the axis
// set clockwise from the top (y down)
AR_HD int ar_dir_x(int d) { return d == 0 || d == 1 || d == 7 ? 1 : (d == 2 || d == 6 ? 0 : -1); }
AR_HD int ar_dir_y(int d) { return d == 1 || d == 2 || d == 3 ? 1 : (d == 0 || d == 4 ? 0 : -1); }

struct ArQuad {
  int32_t ok, id, rot, code;
  double c[8];  // x0 y0 ... x3 y3 in detection pixels, corner 0 the marker's top-left, clockwise
};

AR_HD int64_t ar_shoelace2(const int32_t* q) {
  int64_t a = 0;
  for (int k = 0; k < 4; ++k) {
    const int n = (k + 1) & 3;
    a += (int64_t)q[2 * k] * q[2 * n + 1] - (int64_t)q[2 * n] * q[2 * k + 1];
  }
  return a;
}

// candidate row -> the pixel quad q (x0 y0 ... x3 y3), clockwise; false when it is no marker's outline
AR_HD bool ar_pick_quad(const int32_t* cand, int h, int w, int32_t* q) {
  const int diag[4] = {5, 7, 1, 3}, axis[4] = {6, 0, 2, 4};
  int32_t qd[8], qa[8];
  for (int k = 0; k < 4; ++k) {
    const int32_t ed = cand[6 + diag[k]], ea = cand[6 + axis[k]];
    if (ed < 0 || ea < 0 || (int64_t)ed >= (int64_t)h * w || (int64_t)ea >= (int64_t)h * w) return false;
    qd[2 * k] = ed % w;
    qd[2 * k + 1] = ed / w;
    qa[2 * k] = ea % w;
    qa[2 * k + 1] = ea / w;
  }
  const bool use_d = ar_shoelace2(qd) >= ar_shoelace2(qa);
  for (int k = 0; k < 8; ++k) q[k] = use_d ? qd[k] : qa[k];
  const int64_t a2 = ar_shoelace2(q);
  for (int k = 0; k < 4; ++k) {
    const int n = (k + 1) & 3, m = (k + 2) & 3;
    const int64_t e0x = q[2 * n] - q[2 * k], e0y = q[2 * n + 1] - q[2 * k + 1];
    const int64_t e1x = q[2 * m] - q[2 * n], e1y = q[2 * m + 1] - q[2 * n + 1];
    if (e0x * e1y - e0y * e1x <= 0 || e0x * e0x + e0y * e0y < (int64_t)AR_MIN_SIDE * AR_MIN_SIDE) return false;
  }
  const int64_t area = cand[1];
  if (2 * area * AR_FILL_LO_D < AR_FILL_LO_N * a2 || 2 * area * AR_FILL_HI_D > AR_FILL_HI_N * a2) return false;
  return true;
}

AR_HD int ar_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// bilinear sample with replicated border
AR_HD double ar_sample(const uint8_t* img, int h, int w, double x, double y) {
  if (!(x > -1.0e6 && x < 1.0e6 && y > -1.0e6 && y < 1.0e6)) return 0.0;
  const double flx = std::floor(x), fly = std::floor(y);
  const double fx = x - flx, fy = y - fly;
  const int xi = (int)flx, yi = (int)fly;
  const int xa = ar_clampi(xi, w - 1), xb = ar_clampi(xi + 1, w - 1);
  const int ya = ar_clampi(yi, h - 1), yb = ar_clampi(yi + 1, h - 1);
  const double g00 = img[(int64_t)ya * w + xa], g01 = img[(int64_t)ya * w + xb];
  const double g10 = img[(int64_t)yb * w + xa], g11 = img[(int64_t)yb * w + xb];
  const double top = (1.0 - fx) * g00 + fx * g01;
  const double bot = (1.0 - fx) * g10 + fx * g11;
  return (1.0 - fy) * top + fy * bot;
}

// lane's profile across side lane / 16 at 0.2 + 0.6 (j + 0.5) / 16 along it: where it rises through its mid-level
AR_HD bool ar_profile(const uint8_t* img, int h, int w, const int32_t* q, int lane, double& ex, double& ey) {
  const int k = (lane >> 4) & 3, j = lane & 15, n = (k + 1) & 3;
  const double ax = q[2 * k], ay = q[2 * k + 1];
  const double dx = (double)q[2 * n] - ax, dy = (double)q[2 * n + 1] - ay;
  const double ln = std::sqrt(dx * dx + dy * dy);
  ex = ey = 0.0;
  if (!(ln > 0.0)) return false;
  const double tx = dx / ln, ty = dy / ln;
  const double nx = ty, ny = -tx;  // outward for a clockwise quad, y down
  const double s = 0.2 + 0.6 * (((double)j + 0.5) / (double)AR_N_PROF);
  const double bx = ax + s * dx, by = ay + s * dy;
  double p[AR_PROF_N];
  double lo = 1.0e30, hi = -1.0e30;
  for (int m = 0; m < AR_PROF_N; ++m) {
    const double u = -3.0 + 0.5 * (double)m;
    p[m] = ar_sample(img, h, w, bx + u * nx, by + u * ny);
    lo = p[m] < lo ? p[m] : lo;
    hi = p[m] > hi ? p[m] : hi;
  }
  if (hi - lo < AR_MIN_EDGE) return false;
  const double mid = 0.5 * (lo + hi);
  for (int m = 0; m < AR_PROF_N - 1; ++m)
    if (p[m] < mid && mid <= p[m + 1]) {
      const double us = (-3.0 + 0.5 * (double)m) + 0.5 * (mid - p[m]) / (p[m + 1] - p[m]);
      ex = bx + us * nx;
      ey = by + us * ny;
      return true;
    }
  return false;
}

// direction of the total-least-squares line from the centred second moments
AR_HD bool ar_line_dir(double sxx, double sxy, double syy, double& vx, double& vy) {
  const double hd = 0.5 * (sxx - syy);
  const double lam = 0.5 * (sxx + syy) + std::sqrt(hd * hd + sxy * sxy);
  double a, b;
  if (sxx >= syy) {
    a = lam - syy;
    b = sxy;
  } else {
    a = sxy;
    b = lam - sxx;
  }
  const double nv = std::sqrt(a * a + b * b);
  vx = vy = 0.0;
  if (!(nv > 0.0)) return false;
  vx = a / nv;
  vy = b / nv;
  return true;
}

// line = mx my vx vy.  corner k = line (k + 3) % 4 meets line k; it stays within AR_MAX_MOVE of the pixel corner
AR_HD bool ar_corners(const double* lines, const int32_t* q, double* c) {
  for (int k = 0; k < 4; ++k) {
    const double* a = lines + 4 * ((k + 3) & 3);
    const double* b = lines + 4 * k;
    const double den = a[2] * b[3] - a[3] * b[2];
    if (!(std::fabs(den) >= 1.0e-6)) return false;
    const double s = ((b[0] - a[0]) * b[3] - (b[1] - a[1]) * b[2]) / den;
    c[2 * k] = a[0] + s * a[2];
    c[2 * k + 1] = a[1] + s * a[3];
    if (!(std::fabs(c[2 * k] - (double)q[2 * k]) <= AR_MAX_MOVE &&
          std::fabs(c[2 * k + 1] - (double)q[2 * k + 1]) <= AR_MAX_MOVE))
      return false;
  }
  return true;
}

// unit square (0,0) (1,0) (1,1) (0,1) -> the quad: x = (H0 u + H1 v + H2) / (H6 u + H7 v + 1), y likewise with H3..5
AR_HD void ar_square_to_quad(const double* c, double* H) {
  const double dx1 = c[2] - c[4], dx2 = c[6] - c[4], sx = c[0] - c[2] + c[4] - c[6];
  const double dy1 = c[3] - c[5], dy2 = c[7] - c[5], sy = c[1] - c[3] + c[5] - c[7];
  const double den = dx1 * dy2 - dx2 * dy1;
  const double g = (sx * dy2 - dx2 * sy) / den;
  const double hh = (dx1 * sy - sx * dy1) / den;
  H[0] = c[2] - c[0] + g * c[2];
  H[1] = c[6] - c[0] + hh * c[6];
  H[2] = c[0];
  H[3] = c[3] - c[1] + g * c[3];
  H[4] = c[7] - c[1] + hh * c[7];
  H[5] = c[1];
  H[6] = g;
  H[7] = hh;
}

// sum of the 3 x 3 samples inside cell (row, col) of the 6 x 6 grid
AR_HD double ar_cell_sum(const uint8_t* img, int h, int w, const double* H, int cell) {
  const int r = cell / 6, cc = cell % 6;
  const double off[3] = {0.3, 0.5, 0.7};
  double s = 0.0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double u = ((double)cc + off[b]) / 6.0, v = ((double)r + off[a]) / 6.0;
      const double den = H[6] * u + H[7] * v + 1.0;
      s = s + ar_sample(img, h, w, (H[0] * u + H[1] * v + H[2]) / den, (H[3] * u + H[4] * v + H[5]) / den);
    }
  return s;
}

// 36 cell sums -> the code in the quad's own orientation; false without contrast or with a broken border
AR_HD bool ar_decode(const double* cells, int border_errors, int32_t& code) {
  double mn = cells[0], mx = cells[0];
  for (int k = 1; k < 36; ++k) {
    mn = cells[k] < mn ? cells[k] : mn;
    mx = cells[k] > mx ? cells[k] : mx;
  }
  code = 0;
  if (!(mx - mn >= 9.0 * AR_MIN_CONTRAST)) return false;
  const double thr = 0.5 * (mn + mx);
  int border = 0;
  for (int k = 0; k < 36; ++k) {
    const int r = k / 6, c = k % 6;
    const int bit = cells[k] > thr ? 1 : 0;
    if (r == 0 || r == 5 || c == 0 || c == 5)
      border += bit;
    else
      code |= bit << (15 - (4 * (r - 1) + (c - 1)));
  }
  return border <= border_errors;
}

// the code of the marker turned clockwise by 90 degrees: new[r][c] = old[3 - c][r]
AR_HD uint32_t ar_rot_code(uint32_t code) {
  uint32_t out = 0;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      const uint32_t bit = (code >> (15 - (4 * (3 - c) + r))) & 1u;
      out |= bit << (15 - (4 * r + c));
    }
  return out;
}

AR_HD int ar_popcount16(uint32_t v) {
  int n = 0;
  for (int k = 0; k < 16; ++k) n += (v >> k) & 1u;
  return n;
}

constexpr uint32_t AR_NO_MATCH = 0xffffffffu;

// smallest (distance << 16 | id << 2 | rot) over the codes first, first + stride, ...
AR_HD uint32_t ar_match_partial(uint32_t code, const uint16_t* dict, int n_codes, int first, int stride) {
  uint32_t best = AR_NO_MATCH;
  for (int i = first; i < n_codes; i += stride) {
    uint32_t d = dict[i];
    for (int r = 0; r < 4; ++r) {
      const uint32_t key = ((uint32_t)ar_popcount16(code ^ d) << 16) | ((uint32_t)i << 2) | (uint32_t)r;
      best = key < best ? key : best;
      d = ar_rot_code(d);
    }
  }
  return best;
}

// the result of one quad from its refined corners in geometric order, the decoded code and the best key
AR_HD void ar_finish(const double* c, int32_t code, bool have_dict, uint32_t key, int max_correction_bits, ArQuad& out) {
  out.ok = 0;
  out.id = -1;
  out.rot = 0;
  out.code = code;
  for (int k = 0; k < 8; ++k) out.c[k] = __builtin_nan("");
  int rot = 0;
  if (have_dict) {
    if (key == AR_NO_MATCH || (int)(key >> 16) > max_correction_bits) return;
    out.id = (int32_t)((key >> 2) & 0x3fffu);
    rot = (int)(key & 3u);
  }
  out.ok = 1;
  out.rot = rot;
  for (int k = 0; k < 4; ++k) {
    out.c[2 * k] = c[2 * ((k + rot) & 3)];
    out.c[2 * k + 1] = c[2 * ((k + rot) & 3) + 1];
  }
}

AR_HD void ar_reject(ArQuad& out) {
  out.ok = 0;
  out.id = -1;
  out.rot = 0;
  out.code = 0;
  for (int k = 0; k < 8; ++k) out.c[k] = __builtin_nan("");
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One quad on the host, lane by lane: what one wave of aruco_quads_kernel does.  dict may be null (every quad that
// passes the border test is accepted with id -1).
inline void ar_quad_host(const uint8_t* img, int h, int w, const int32_t* cand, const uint16_t* dict, int n_codes,
                         int max_correction_bits, int border_errors, ArQuad& out) {
  ar_reject(out);
  int32_t q[8];
  if (!ar_pick_quad(cand, h, w, q)) return;
  double ex[AR_LANES], ey[AR_LANES], part[AR_LANES][3];
  bool valid[AR_LANES];
  for (int l = 0; l < AR_LANES; ++l) {
    valid[l] = ar_profile(img, h, w, q, l, ex[l], ey[l]);
    part[l][0] = valid[l] ? 1.0 : 0.0;
    part[l][1] = valid[l] ? ex[l] : 0.0;
    part[l][2] = valid[l] ? ey[l] : 0.0;
  }
  auto butterfly = [&]() {  // within each group of 16 lanes
    for (int o = AR_N_PROF / 2; o > 0; o >>= 1) {
      double nxt[AR_LANES][3];
      for (int l = 0; l < AR_LANES; ++l)
        for (int k = 0; k < 3; ++k) nxt[l][k] = part[l][k] + part[l ^ o][k];
      for (int l = 0; l < AR_LANES; ++l)
        for (int k = 0; k < 3; ++k) part[l][k] = nxt[l][k];
    }
  };
  butterfly();
  double lines[16];
  double mean[4][2];
  for (int k = 0; k < 4; ++k) {
    const double* s = part[16 * k];
    if (!(s[0] >= (double)AR_MIN_PROFILES)) return;
    mean[k][0] = s[1] / s[0];
    mean[k][1] = s[2] / s[0];
  }
  for (int l = 0; l < AR_LANES; ++l) {
    const int k = l >> 4;
    const double dx = valid[l] ? ex[l] - mean[k][0] : 0.0, dy = valid[l] ? ey[l] - mean[k][1] : 0.0;
    part[l][0] = dx * dx;
    part[l][1] = dx * dy;
    part[l][2] = dy * dy;
  }
  butterfly();
  for (int k = 0; k < 4; ++k) {
    const double* s = part[16 * k];
    lines[4 * k] = mean[k][0];
    lines[4 * k + 1] = mean[k][1];
    if (!ar_line_dir(s[0], s[1], s[2], lines[4 * k + 2], lines[4 * k + 3])) return;
  }
  double c[8], H[8], cells[36];
  if (!ar_corners(lines, q, c)) return;
  ar_square_to_quad(c, H);
  for (int k = 0; k < 36; ++k) cells[k] = ar_cell_sum(img, h, w, H, k);
  int32_t code = 0;
  if (!ar_decode(cells, border_errors, code)) return;
  uint32_t key = AR_NO_MATCH;
  if (dict)
    for (int l = 0; l < AR_LANES; ++l) {
      const uint32_t kk = ar_match_partial((uint32_t)code, dict, n_codes, l, AR_LANES);
      key = kk < key ? kk : key;
    }
  ar_finish(c, code, dict != nullptr, key, max_correction_bits, out);
}
#endif

}  // namespace mq
