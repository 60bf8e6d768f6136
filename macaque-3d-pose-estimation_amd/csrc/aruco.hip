// ArUco-marker detector for gfx950: the reference's aruco.detectMarkers (multicam_toolbox.py:283, :356) as a
// detector of this project's own for 4 x 4 codes given by the caller.  tests/aruco_ref.py is the numpy restatement;
// stages 2-4 are integer and equal it exactly, stage 5 is float64 without FMA contraction.
//   2. aruco_threshold_kernel   box sum of a 23 x 23 window from one LDS tile (11-pixel halo), integer compare
//   3. aruco_label_init /       union-find over the dark pixels: a pixel starts at its row run's first pixel, the
//      _merge / _flatten        merge joins vertically adjacent runs with atomicMin on the larger root, the flatten
//                               writes every pixel's root.  Three launches; parent[] is read with agent-scope atomic
//                               loads.  No thread waits on another: a find walks strictly decreasing parents, a
//                               union retries only when its atomicMin found the root already lowered by another
//   4. aruco_area / _slots /    area per root; the roots above the area gate get a slot, in ascending order (a scan
//      _stats / _candidates     inside one workgroup per image); bounding box and the eight extremes per slot by
//                               integer atomics over the components' outline pixels (64-bit atomicMax over unique
//                               keys: no dependence on arrival order); the gates, again in ascending order
//   5. aruco_quads_kernel       one wave per candidate runs aruco_dev.hpp's core
//   6. aruco_collect_kernel     order by (id, label), frame pixels
#include <hip/hip_runtime.h>

#include "aruco.hpp"
#include "aruco_dev.hpp"

namespace mq {

namespace {

int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }

// ------------------------------------------------------------------ 2. threshold
constexpr int TT_W = 64, TT_H = 16;
constexpr int TT_GW = TT_W + 2 * AR_THR_R, TT_GH = TT_H + 2 * AR_THR_R;

__global__ __launch_bounds__(256) void aruco_threshold_kernel(const uint8_t* __restrict__ gray, int h, int w,
                                                              uint8_t* __restrict__ dark) {
  __shared__ uint8_t g[TT_GH][TT_GW + 2];
  __shared__ int32_t rs[TT_GH][TT_W];  // row sums over the window's 23 columns
  const int x0 = blockIdx.x * TT_W, y0 = blockIdx.y * TT_H;
  const uint8_t* img = gray + (int64_t)blockIdx.z * h * w;
  for (int e = threadIdx.x; e < TT_GH * TT_GW; e += 256) {
    const int r = e / TT_GW, c = e % TT_GW;
    int yy = y0 + r - AR_THR_R, xx = x0 + c - AR_THR_R;
    yy = yy < 0 ? 0 : (yy > h - 1 ? h - 1 : yy);  // replicated border
    xx = xx < 0 ? 0 : (xx > w - 1 ? w - 1 : xx);
    g[r][c] = img[(int64_t)yy * w + xx];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < TT_GH * TT_W; e += 256) {
    const int r = e / TT_W, c = e % TT_W;
    int s = 0;
#pragma unroll
    for (int k = 0; k <= 2 * AR_THR_R; ++k) s += g[r][c + k];
    rs[r][c] = s;
  }
  __syncthreads();
  const int tx = threadIdx.x % TT_W, ty = threadIdx.x / TT_W;
  const int x = x0 + tx;
  if (x >= w) return;
  constexpr int N = (2 * AR_THR_R + 1) * (2 * AR_THR_R + 1);
  for (int r = ty; r < TT_H; r += 256 / TT_W) {
    const int y = y0 + r;
    if (y >= h) break;
    int box = 0;
#pragma unroll
    for (int k = 0; k <= 2 * AR_THR_R; ++k) box += rs[r + k][tx];
    const int v = g[r + AR_THR_R][tx + AR_THR_R];
    dark[((int64_t)blockIdx.z * h + y) * w + x] = (v * N < box - AR_THR_C * N) ? 1 : 0;
  }
}

// ------------------------------------------------------------------ 3. label
__device__ __forceinline__ int32_t parent_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of a: parents are strictly smaller than their children, so the walk ends
__device__ __forceinline__ int32_t find_root(const int32_t* parent, int32_t a) {
  int32_t p = parent_load(parent + a);
  while (p != a) {
    a = p;
    p = parent_load(parent + a);
  }
  return a;
}

// a pixel starts at the first pixel of its run of dark pixels within the 256-pixel segment of its row; the first
// pixel of a segment whose left neighbour is dark starts at that neighbour
__global__ __launch_bounds__(256) void aruco_label_init_kernel(const uint8_t* __restrict__ dark, int h, int w,
                                                               int32_t* __restrict__ parent) {
  __shared__ int32_t sc[2][256];
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const uint8_t* d = dark + (int64_t)blockIdx.z * h * w;
  int32_t* par = parent + (int64_t)blockIdx.z * h * w;
  const bool in = x < w;
  const bool on = in && d[(int64_t)y * w + x] != 0;
  const bool left = in && x > 0 && d[(int64_t)y * w + x - 1] != 0;
  int32_t v = -1;
  if (on && (!left || threadIdx.x == 0)) v = left ? y * w + x - 1 : y * w + x;
  sc[0][threadIdx.x] = v;
  __syncthreads();
  int cur = 0;
  for (int o = 1; o < 256; o <<= 1) {  // inclusive max scan: the latest run start at or before x
    int32_t m = sc[cur][threadIdx.x];
    if ((int)threadIdx.x >= o) m = max(m, sc[cur][threadIdx.x - o]);
    sc[cur ^ 1][threadIdx.x] = m;
    cur ^= 1;
    __syncthreads();
  }
  if (in) par[(int64_t)y * w + x] = on ? sc[cur][threadIdx.x] : -1;
}

// joins pixel (x, y) to (x, y - 1) where both are dark, unless the pair to their left already joins the two runs
__global__ __launch_bounds__(256) void aruco_label_merge_kernel(const uint8_t* __restrict__ dark, int h, int w,
                                                                int32_t* __restrict__ parent) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y + 1;
  if (x >= w || y >= h) return;
  const uint8_t* d = dark + (int64_t)blockIdx.z * h * w;
  int32_t* par = parent + (int64_t)blockIdx.z * h * w;
  const int32_t i = y * w + x;
  if (!d[i] || !d[i - w]) return;
  if (x > 0 && d[i - 1] && d[i - w - 1]) return;
  int32_t a = i, b = i - w;
  for (;;) {
    a = find_root(par, a);
    b = find_root(par, b);
    if (a == b) break;
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    // a > b: hang root a below b.  When another thread lowered parent[a] first, `old` is where a pointed: the
    // minimum now stored keeps one of the two links, the next round restores the other.
    const int32_t old = atomicMin(par + a, b);
    if (old == a) break;
    a = old;
  }
}

__global__ __launch_bounds__(256) void aruco_label_flatten_kernel(int64_t hw, int32_t* __restrict__ parent) {
  int32_t* par = parent + (int64_t)blockIdx.y * hw;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  if (parent_load(par + i) < 0) return;
  const int32_t r = find_root(par, (int32_t)i);
  atomicMin(par + i, r);  // the root is the smallest index of the component: the final value whatever the order
}

// ------------------------------------------------------------------ 4. components
struct Slot {
  int32_t label, area, x0, y0, x1, y1, pad0, pad1;
  unsigned long long ext[8];
};

constexpr int EXT_BIAS = 1 << 17;  // projections are in (-2^16, 2^16)

__global__ __launch_bounds__(256) void aruco_area_kernel(const int32_t* __restrict__ labels, int64_t hw,
                                                         int32_t* __restrict__ area) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const int32_t l = labels[(int64_t)blockIdx.y * hw + i];
  if (l >= 0 && l < hw) atomicAdd(area + (int64_t)blockIdx.y * hw + l, 1);
}

// exclusive scan of one int per thread over the workgroup; *total receives the sum
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int32_t (*sc)[NT], int* total) {
  sc[0][threadIdx.x] = v;
  __syncthreads();
  int cur = 0;
  for (int o = 1; o < NT; o <<= 1) {
    int m = sc[cur][threadIdx.x];
    if ((int)threadIdx.x >= o) m += sc[cur][threadIdx.x - o];
    sc[cur ^ 1][threadIdx.x] = m;
    cur ^= 1;
    __syncthreads();
  }
  const int incl = sc[cur][threadIdx.x];
  *total = sc[cur][NT - 1];
  __syncthreads();
  return incl - v;
}

// One workgroup per image.  The roots with area >= AR_MIN_AREA get slots in ascending order; area[root] becomes the
// slot (-1 for the other roots).  At most hw / AR_MIN_AREA roots pass, which is what max_slots holds.
__global__ __launch_bounds__(1024) void aruco_slots_kernel(const int32_t* __restrict__ labels, int64_t hw,
                                                           int32_t* __restrict__ area, Slot* __restrict__ slots,
                                                           int max_slots, int32_t* __restrict__ n_slots) {
  __shared__ int32_t sc[2][1024];
  const int img = blockIdx.x;
  const int32_t* lab = labels + (int64_t)img * hw;
  int32_t* ar = area + (int64_t)img * hw;
  Slot* sl = slots + (int64_t)img * max_slots;
  const int64_t per = (hw + 1023) / 1024;
  const int64_t i0 = per * threadIdx.x, i1 = (i0 + per < hw) ? i0 + per : hw;
  int mine = 0;
  for (int64_t i = i0; i < i1; ++i) mine += (lab[i] == (int32_t)i && ar[i] >= AR_MIN_AREA) ? 1 : 0;
  int total;
  int at = block_excl_scan<1024>(mine, sc, &total);
  for (int64_t i = i0; i < i1; ++i) {
    if (lab[i] != (int32_t)i) continue;
    const int32_t a = ar[i];
    int32_t s = -1;
    if (a >= AR_MIN_AREA) {
      if (at < max_slots) {
        s = at;
        Slot& o = sl[s];
        o.label = (int32_t)i;
        o.area = a;
        o.x0 = o.y0 = INT32_MAX;
        o.x1 = o.y1 = -1;
        o.pad0 = o.pad1 = 0;
        for (int k = 0; k < 8; ++k) o.ext[k] = 0ull;
      }
      ++at;
    }
    ar[i] = s;
  }
  if (threadIdx.x == 0) n_slots[img] = total < max_slots ? total : max_slots;
}

// bounding box and extremes from the outline pixels: a pixel whose four neighbours are dark is beaten by one of them
// in every one of the eight directions
__global__ __launch_bounds__(256) void aruco_stats_kernel(const int32_t* __restrict__ labels, int h, int w,
                                                          const int32_t* __restrict__ area, Slot* __restrict__ slots,
                                                          int max_slots) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= w) return;
  const int64_t hw = (int64_t)h * w;
  const int32_t* lab = labels + (int64_t)blockIdx.z * hw;
  const int32_t i = y * w + x;
  const int32_t l = lab[i];
  if (l < 0 || l >= hw) return;
  const int32_t s = area[(int64_t)blockIdx.z * hw + l];
  if (s < 0 || s >= max_slots) return;
  if (x > 0 && x < w - 1 && y > 0 && y < h - 1 && lab[i - 1] >= 0 && lab[i + 1] >= 0 && lab[i - w] >= 0 &&
      lab[i + w] >= 0)
    return;
  Slot& o = slots[(int64_t)blockIdx.z * max_slots + s];
  atomicMin(&o.x0, x);
  atomicMin(&o.y0, y);
  atomicMax(&o.x1, x);
  atomicMax(&o.y1, y);
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    const int proj = ar_dir_x(d) * x + ar_dir_y(d) * y + EXT_BIAS;
    atomicMax(&o.ext[d], ((unsigned long long)(unsigned)proj << 32) | (unsigned)i);
  }
}

// One workgroup per image: the slots that pass the box gates, in slot (= label) order
__global__ __launch_bounds__(256) void aruco_candidates_kernel(const Slot* __restrict__ slots, int max_slots,
                                                               const int32_t* __restrict__ n_slots, int h, int w,
                                                               int max_quads, int32_t* __restrict__ count,
                                                               int32_t* __restrict__ cand) {
  __shared__ int32_t sc[2][256];
  const int img = blockIdx.x;
  const Slot* sl = slots + (int64_t)img * max_slots;
  int32_t* out = cand + (int64_t)img * max_quads * AR_CAND;
  for (int e = threadIdx.x; e < max_quads * AR_CAND; e += 256) out[e] = 0;
  int ns = n_slots[img];
  ns = ns < 0 ? 0 : (ns > max_slots ? max_slots : ns);
  const int per = (ns + 255) / 256;
  const int s0 = per * threadIdx.x, s1 = (s0 + per < ns) ? s0 + per : ns;
  auto pass = [&](const Slot& o) {
    return o.x1 - o.x0 + 1 >= AR_MIN_BOX && o.y1 - o.y0 + 1 >= AR_MIN_BOX && o.x0 >= 1 && o.y0 >= 1 &&
           o.x1 <= w - 2 && o.y1 <= h - 2;
  };
  int mine = 0;
  for (int s = s0; s < s1; ++s) mine += pass(sl[s]) ? 1 : 0;
  int total;
  int at = block_excl_scan<256>(mine, sc, &total);  // its barriers also order the zeroing above before the rows below
  for (int s = s0; s < s1; ++s) {
    const Slot& o = sl[s];
    if (!pass(o)) continue;
    if (at < max_quads) {
      int32_t* row = out + at * AR_CAND;
      row[0] = o.label;
      row[1] = o.area;
      row[2] = o.x0;
      row[3] = o.y0;
      row[4] = o.x1;
      row[5] = o.y1;
      for (int k = 0; k < 8; ++k) row[6 + k] = (int32_t)(o.ext[k] & 0xffffffffull);
    }
    ++at;
  }
  if (threadIdx.x == 0) count[img] = total;
}

// ------------------------------------------------------------------ 5. quads
__global__ __launch_bounds__(AR_LANES) void aruco_quads_kernel(const uint8_t* __restrict__ gray, int h, int w,
                                                               const int32_t* __restrict__ count,
                                                               const int32_t* __restrict__ cand, int max_quads,
                                                               const uint16_t* __restrict__ dict, int n_codes,
                                                               int max_correction_bits, int border_errors,
                                                               int32_t* __restrict__ ok, int32_t* __restrict__ ids,
                                                               int32_t* __restrict__ rot,
                                                               double* __restrict__ corners) {
  __shared__ double lines[16];
  __shared__ int32_t line_ok[4];
  __shared__ double cells[36];
  const int k = blockIdx.x, img = blockIdx.y, lane = threadIdx.x;
  const int64_t slot = (int64_t)img * max_quads + k;
  const uint8_t* im = gray + (int64_t)img * h * w;
  ArQuad res;
  ar_reject(res);
  int n = count[img];
  n = n < 0 ? 0 : (n > max_quads ? max_quads : n);
  int32_t q[8];
  // every branch below depends only on values all lanes share
  bool go = k < n && ar_pick_quad(cand + slot * AR_CAND, h, w, q);
  if (go) {
    double ex, ey;
    const bool valid = ar_profile(im, h, w, q, lane, ex, ey);
    double s0 = valid ? 1.0 : 0.0, s1 = valid ? ex : 0.0, s2 = valid ? ey : 0.0;
    for (int o = AR_N_PROF / 2; o > 0; o >>= 1) {
      s0 += __shfl_xor(s0, o, AR_LANES);
      s1 += __shfl_xor(s1, o, AR_LANES);
      s2 += __shfl_xor(s2, o, AR_LANES);
    }
    const bool side = s0 >= (double)AR_MIN_PROFILES;
    const double mx = side ? s1 / s0 : 0.0, my = side ? s2 / s0 : 0.0;
    const double dx = valid ? ex - mx : 0.0, dy = valid ? ey - my : 0.0;
    double sxx = dx * dx, sxy = dx * dy, syy = dy * dy;
    for (int o = AR_N_PROF / 2; o > 0; o >>= 1) {
      sxx += __shfl_xor(sxx, o, AR_LANES);
      sxy += __shfl_xor(sxy, o, AR_LANES);
      syy += __shfl_xor(syy, o, AR_LANES);
    }
    double vx, vy;
    const bool lok = ar_line_dir(sxx, sxy, syy, vx, vy) && side;
    if ((lane & 15) == 0) {
      const int sd = lane >> 4;
      lines[4 * sd] = mx;
      lines[4 * sd + 1] = my;
      lines[4 * sd + 2] = vx;
      lines[4 * sd + 3] = vy;
      line_ok[sd] = lok ? 1 : 0;
    }
    __syncthreads();
    go = line_ok[0] && line_ok[1] && line_ok[2] && line_ok[3];
  }
  double c[8], H[8];
  if (go) {
    go = ar_corners(lines, q, c);
  }
  if (go) {
    ar_square_to_quad(c, H);
    if (lane < 36) cells[lane] = ar_cell_sum(im, h, w, H, lane);
    __syncthreads();
    int32_t code = 0;
    if (ar_decode(cells, border_errors, code)) {
      uint32_t key = AR_NO_MATCH;
      if (dict) {
        key = ar_match_partial((uint32_t)code, dict, n_codes, lane, AR_LANES);
        for (int o = AR_LANES / 2; o > 0; o >>= 1) {
          const uint32_t t = (uint32_t)__shfl_xor((int)key, o, AR_LANES);
          key = t < key ? t : key;
        }
      }
      ar_finish(c, code, dict != nullptr, key, max_correction_bits, res);
    }
  }
  if (lane == 0) {
    ok[slot] = res.ok;
    ids[slot] = res.id;
    rot[slot] = res.rot;
  }
  if (lane < 8) corners[slot * 8 + lane] = res.c[lane];
}

// ------------------------------------------------------------------ 6. collect
__global__ __launch_bounds__(AR_LANES) void aruco_collect_kernel(const int32_t* __restrict__ cand_count,
                                                                 const int32_t* __restrict__ cand,
                                                                 const int32_t* __restrict__ ok,
                                                                 const int32_t* __restrict__ ids,
                                                                 const double* __restrict__ corners, int max_quads,
                                                                 int max_markers, double rx, double ry,
                                                                 int32_t* __restrict__ count_out,
                                                                 int32_t* __restrict__ ids_out,
                                                                 double* __restrict__ corners_out) {
  __shared__ int32_t order[AR_MAX_QUADS];
  __shared__ int32_t n_sh;
  const int img = blockIdx.x;
  int n = cand_count[img];
  n = n < 0 ? 0 : (n > max_quads ? max_quads : n);
  const int64_t base = (int64_t)img * max_quads;
  if (threadIdx.x == 0) {
    int m = 0;  // insertion sort by (id, label): the candidates come in ascending label order
    for (int k = 0; k < n; ++k) {
      if (!ok[base + k]) continue;
      int at = m;
      while (at > 0 && ids[base + order[at - 1]] > ids[base + k]) {
        order[at] = order[at - 1];
        --at;
      }
      order[at] = k;
      ++m;
    }
    n_sh = m < max_markers ? m : max_markers;
    count_out[img] = n_sh;
  }
  __syncthreads();
  const int m = n_sh;
  for (int j = threadIdx.x; j < max_markers; j += AR_LANES)
    ids_out[(int64_t)img * max_markers + j] = j < m ? ids[base + order[j]] : -1;
  for (int e = threadIdx.x; e < max_markers * 8; e += AR_LANES) {
    const int j = e >> 3, cpt = e & 7;
    double v = __builtin_nan("");
    if (j < m) {
      const double p = corners[(base + order[j]) * 8 + cpt];
      const double r = (cpt & 1) ? ry : rx;
      v = p * r + (r - 1.0) / 2.0;
    }
    corners_out[((int64_t)img * max_markers + j) * 8 + cpt] = v;
  }
}

int max_slots_of(int h, int w) { return (int)(((int64_t)h * w) / AR_MIN_AREA) + 1; }

}  // namespace

int aruco_threshold(const uint8_t* gray, int n, int h, int w, uint8_t* dark, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(aruco_threshold_kernel, dim3((w + TT_W - 1) / TT_W, (h + TT_H - 1) / TT_H, n), dim3(256), 0, s,
                     gray, h, w, dark);
  return launched();
}

int aruco_label(const uint8_t* dark, int n, int h, int w, int32_t* labels, hipStream_t s) {
  if (n <= 0) return 0;
  if ((int64_t)h * w >= ((int64_t)1 << 31) || h > 65535) return -1;
  const int64_t hw = (int64_t)h * w;
  hipLaunchKernelGGL(aruco_label_init_kernel, dim3((w + 255) / 256, h, n), dim3(256), 0, s, dark, h, w, labels);
  if (h > 1)
    hipLaunchKernelGGL(aruco_label_merge_kernel, dim3((w + 255) / 256, h - 1, n), dim3(256), 0, s, dark, h, w, labels);
  hipLaunchKernelGGL(aruco_label_flatten_kernel, dim3((unsigned)((hw + 255) / 256), n), dim3(256), 0, s, hw, labels);
  return launched();
}

ArucoCompBufs aruco_components_layout(Carver& c, int n, int h, int w) {
  const size_t nn = (size_t)(n > 0 ? n : 0);
  ArucoCompBufs b;
  b.n_area = nn * (size_t)h * (size_t)w;
  b.area = c.take<int32_t>(b.n_area);
  b.slots = c.take<Slot>(nn * (size_t)max_slots_of(h, w));
  b.n_slots = c.take<int32_t>(nn);
  return b;
}

size_t aruco_components_ws_bytes(int n, int h, int w) { return measure(aruco_components_layout, n, h, w); }

int aruco_components(const int32_t* labels, int n, int h, int w, int max_quads, int32_t* count, int32_t* cand,
                     const ArucoCompBufs& b, hipStream_t s) {
  if (n <= 0) return 0;
  if (max_quads < 1 || max_quads > AR_MAX_QUADS || (int64_t)h * w >= ((int64_t)1 << 31) || h > 65535) return -1;
  const int64_t hw = (int64_t)h * w;
  const int ms = max_slots_of(h, w);
  int32_t *area = b.area, *n_slots = b.n_slots;
  Slot* slots = static_cast<Slot*>(b.slots);
  if (hipMemsetAsync(area, 0, b.n_area * sizeof(int32_t), s) != hipSuccess) return -1;
  hipLaunchKernelGGL(aruco_area_kernel, dim3((unsigned)((hw + 255) / 256), n), dim3(256), 0, s, labels, hw, area);
  hipLaunchKernelGGL(aruco_slots_kernel, dim3(n), dim3(1024), 0, s, labels, hw, area, slots, ms, n_slots);
  hipLaunchKernelGGL(aruco_stats_kernel, dim3((w + 255) / 256, h, n), dim3(256), 0, s, labels, h, w, area, slots, ms);
  hipLaunchKernelGGL(aruco_candidates_kernel, dim3(n), dim3(256), 0, s, slots, ms, n_slots, h, w, max_quads, count,
                     cand);
  return launched();
}

int aruco_quads(const uint8_t* gray, int n, int h, int w, const int32_t* count, const int32_t* cand, int max_quads,
                const uint16_t* dict, int n_codes, int max_correction_bits, int border_errors, int32_t* ok,
                int32_t* ids, int32_t* rot, double* corners, hipStream_t s) {
  if (n <= 0) return 0;
  if (max_quads < 1 || max_quads > AR_MAX_QUADS || n_codes < 0 || n_codes > AR_MAX_CODES) return -1;
  hipLaunchKernelGGL(aruco_quads_kernel, dim3(max_quads, n), dim3(AR_LANES), 0, s, gray, h, w, count, cand, max_quads,
                     dict, n_codes, max_correction_bits, border_errors, ok, ids, rot, corners);
  return launched();
}

int aruco_collect(const int32_t* cand_count, const int32_t* cand, const int32_t* ok, const int32_t* ids,
                  const double* corners, int n, int max_quads, int max_markers, double ratio_x, double ratio_y,
                  int32_t* count_out, int32_t* ids_out, double* corners_out, hipStream_t s) {
  if (n <= 0) return 0;
  if (max_quads < 1 || max_quads > AR_MAX_QUADS || max_markers < 1 || max_markers > AR_MAX_QUADS) return -1;
  hipLaunchKernelGGL(aruco_collect_kernel, dim3(n), dim3(AR_LANES), 0, s, cand_count, cand, ok, ids, corners,
                     max_quads, max_markers, ratio_x, ratio_y, count_out, ids_out, corners_out);
  return launched();
}

}  // namespace mq
