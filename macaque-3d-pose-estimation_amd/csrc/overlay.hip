// Pose overlay (visualize_result.py proc :220-242, clean_kp :30-62 with show_as_possible, draw_kps :71-110,
// ellipse_line :19-28; visualize_result_2.py's skeleton): reproject kp3d into a camera, turn each animal's
// joints into discs and limbs, and draw them over a copy of the frame.  Compiled with -ffp-contract=off.
//
// overlay_prims_kernel  one wave per (output image, animal); lanes are the joints (lane J is the neck), then the
//                       limbs.  Writes a fixed-size primitive table per (image, animal).
// overlay_draw_kernel   fused copy + draw; one workgroup per (image, tile).  Wave 0 culls the image's primitives
//                       against the tile into LDS (ascending order), then every thread produces 16-byte chunks
//                       of the output rows: one read of the source, one write of the output, no read of `out`.
//
// Coverage rules (the project's own, exact, shared with tests/overlay_ref.py; cv2's fixed-point circle /
// ellipse2Poly / FillConvexPoly rasterisers and its whole-degree limb angle are not restated):
//   disc (cx, cy, r), integers:   (X - cx)^2 + (Y - cy)^2 <= r^2 + r
//   limb (x1, y1)-(x2, y2), minor axis m, fp64 in this order:
//     ex = x2 - x1, ey = y2 - y1, d2 = ex*ex + ey*ey, cx = (x1 + x2)/2, cy = (y1 + y2)/2, px = X - cx, py = Y - cy,
//     u = px*ex + py*ey, v = py*ex - px*ey, a2 = d2/4, b2 = m*m/4;  inside iff d2 > 0 and u*u*b2 + v*v*a2 <= a2*b2*d2
// The pixel takes the colour of the highest animal index with a covering primitive (the reference's painter's
// order: one colour per animal, animals drawn in index order), else the source pixel.
//
// Labelled variant (step3_crossframematching.py visualize :1642-1670: the tracklet's voted collar ID picks the
// colour, cv2.putText writes its key at the skeleton's upper left): the LBL instantiations of both kernels.  Each
// animal gets one more slot, the last, holding its label: a list of stroke segments relative to an origin.
//   label segment p0 -> p1 (origin added), thickness t, integers (int64): e = p1 - p0, w = X - p0;
//     w.e <= 0: 4|w|^2 <= t^2;  w.e >= |e|^2: 4|X - p1|^2 <= t^2;  else 4 (w x e)^2 <= t^2 |e|^2
// The label is the animal's highest slot, so it lies over that animal's skeleton and under every higher animal.
// A colour table (B, A) replaces "colour = animal index": entry 0..3 as animal_colour, anything else black.
#include "common.hpp"
#include "camera.hpp"
#include "dlt_dev.hpp"
#include "overlay.hpp"

namespace mq {

// ------------------------------------------------------------------------------------------- primitives
template <bool LBL>
__global__ __launch_bounds__(64) void overlay_prims_kernel(
    const double* __restrict__ cams, int C, const int32_t* __restrict__ cam_of_img, const double* __restrict__ kp3d,
    const double* __restrict__ score, int A, int J, OverlaySkeleton sk, int mrksize, int32_t* __restrict__ prim_i,
    double* __restrict__ prim_d, OverlayLabels lb) {
  __shared__ double px[OVL_MAX_PRIMS], py[OVL_MAX_PRIMS];
  __shared__ int ok[OVL_MAX_PRIMS];
  const int b = blockIdx.x / A, a = blockIdx.x % A;
  const int lane = threadIdx.x;
  const int P = sk.n_pairs, NP = J + 1 + P + (LBL ? 1 : 0);
  const int cam = cam_of_img[b];
  const double* x3 = kp3d + ((size_t)b * A + a) * J * 3;
  const double* sc = score + ((size_t)b * A + a) * J;

  // lanes 0..J: the joint (lane J: the neck, the mean of joints 5 and 6 in 3D and of their scores)
  double X = 0, Y = 0, Z = 0, s = 0, u = NAN, v = NAN;
  bool flag = false;
  if (lane <= J) {
    if (lane < J) {
      X = x3[3 * lane];
      Y = x3[3 * lane + 1];
      Z = x3[3 * lane + 2];
      s = sc[lane];
    } else {
      X = (x3[15] + x3[18]) / 2;
      Y = (x3[16] + x3[19]) / 2;
      Z = (x3[17] + x3[20]) / 2;
      s = (sc[5] + sc[6]) / 2;
    }
    if (cam >= 0 && cam < C) cam_project(cam_at(cams, cam), X, Y, Z, u, v);
    flag = !(X == 0) && (s > 0.0);  // proc :231-232
  }
  const int cnt = __popcll(__ballot(flag));  // clean_kp :32-35 on the 0/1 flag
  if (lane <= J) {
    bool keep = !(sk.flags[lane] & OVL_JOINT_NULLED) && cnt != 0 && !(u != u);
    if (keep && (u > 3000 || u < -1000 || v > 3000 || v < -1000)) keep = false;
    if (v != v) keep = false;  // int(nan) raises in the reference; nothing is drawn here
    px[lane] = u;
    py[lane] = v;
    ok[lane] = keep;
    int32_t* o = prim_i + (((size_t)b * A + a) * NP + lane) * 8;
    const bool disc = keep && (sk.flags[lane] & OVL_JOINT_DISC);
    const int cx = disc ? (int)u : 0, cy = disc ? (int)v : 0, r = disc ? (int)sk.radius[lane] : 0;
    o[0] = disc;
    o[1] = cx;
    o[2] = cy;
    o[3] = r;
    o[4] = cx - r;
    o[5] = cy - r;
    o[6] = cx + r;
    o[7] = cy + r;
  }
  __syncthreads();
  if (lane < P) {
    const int i1 = sk.pair_a[lane], i2 = sk.pair_b[lane];
    const bool valid = ok[i1] && ok[i2];
    const double x1 = valid ? px[i1] : 0.0, y1 = valid ? py[i1] : 0.0;
    const double x2 = valid ? px[i2] : 0.0, y2 = valid ? py[i2] : 0.0;
    const double hm = (double)mrksize / 2;
    int32_t* o = prim_i + (((size_t)b * A + a) * NP + J + 1 + lane) * 8;
    o[0] = valid;
    o[1] = 0;
    o[2] = 0;
    o[3] = 0;
    o[4] = valid ? (int)floor(fmin(x1, x2) - hm) : 0;
    o[5] = valid ? (int)floor(fmin(y1, y2) - hm) : 0;
    o[6] = valid ? (int)ceil(fmax(x1, x2) + hm) : 0;
    o[7] = valid ? (int)ceil(fmax(y1, y2) + hm) : 0;
    double* d = prim_d + (((size_t)b * A + a) * P + lane) * 4;
    d[0] = x1;
    d[1] = y1;
    d[2] = x2;
    d[3] = y2;
  }
  if constexpr (LBL) {
    // the label slot (visualize :1658-1670): origin = the NaN-ignoring minima of u and v over all J + 1 slots,
    // before clean_kp; box = the segments' extent around it, padded by ceil(t / 2)
    int n = lb.seg ? lb.n[(size_t)b * A + a] : 0;
    n = n < 0 ? 0 : (n > lb.S ? lb.S : n);
    int x0 = INT32_MAX, y0 = INT32_MAX, x1 = INT32_MIN, y1 = INT32_MIN;
    for (int i = lane; i < n; i += 64) {
      const int32_t* g = lb.seg + (((size_t)b * A + a) * lb.S + i) * 4;
      x0 = min(x0, min(g[0], g[2]));
      y0 = min(y0, min(g[1], g[3]));
      x1 = max(x1, max(g[0], g[2]));
      y1 = max(y1, max(g[1], g[3]));
    }
    for (int o = 32; o > 0; o >>= 1) {
      x0 = min(x0, __shfl_xor(x0, o));
      y0 = min(y0, __shfl_xor(y0, o));
      x1 = max(x1, __shfl_xor(x1, o));
      y1 = max(y1, __shfl_xor(y1, o));
    }
    if (lane == 0) {
      double xm = NAN, ym = NAN;
      for (int j = 0; j <= J; ++j) {
        const double uj = px[j], vj = py[j];
        if (uj == uj && !(xm <= uj)) xm = uj;
        if (vj == vj && !(ym <= vj)) ym = vj;
      }
      bool valid = n > 0 && xm == xm && ym == ym;
      if (valid && (xm > 3000 || xm < -1000 || ym > 3000 || ym < -1000)) valid = false;
      // beyond +-OVL_MAX_LABEL_COORD, 4 (w x e)^2 could leave int64: such a label is not drawn
      if (valid && (x0 < -OVL_MAX_LABEL_COORD || y0 < -OVL_MAX_LABEL_COORD || x1 > OVL_MAX_LABEL_COORD ||
                    y1 > OVL_MAX_LABEL_COORD))
        valid = false;
      const int ox = valid ? (int)xm : 0, oy = valid ? (int)ym : 0, pad = (lb.t + 1) / 2;
      int32_t* o = prim_i + (((size_t)b * A + a) * NP + NP - 1) * 8;
      o[0] = valid;
      o[1] = ox;
      o[2] = oy;
      o[3] = 0;
      o[4] = valid ? ox + x0 - pad : 0;
      o[5] = valid ? oy + y0 - pad : 0;
      o[6] = valid ? ox + x1 + pad : 0;
      o[7] = valid ? oy + y1 + pad : 0;
    }
  }
}

// ------------------------------------------------------------------------------------------------- draw
constexpr int OVL_TILE_CHUNKS = 16;  // 16-byte chunks per tile row: 256 bytes, 85.3 pixels
constexpr int OVL_TILE_ROWS = 32;
constexpr int OVL_THREADS = 256;
constexpr int OVL_CHUNK_PIX = 6;     // a 16-byte chunk touches at most 6 BGR pixels

// BGR colours (255,0,0), (0,255,0), (0,0,255), (255,255,255); animals >= 4 are black
__device__ __forceinline__ uint32_t animal_colour(int a, int ch) {
  return a < 3 ? (a == ch ? 255u : 0u) : (a == 3 ? 255u : 0u);
}

// One chunk of one row.  S = (first byte of the chunk) % 3: byte i of the chunk is channel (i + S) % 3 of the
// chunk's pixel (i + S) / 3, whose column is X0 + (i + S) / 3.
template <int S, bool VEC, bool LBL>
__device__ __forceinline__ void draw_chunk(const uint8_t* __restrict__ srow, uint8_t* __restrict__ orow, int byte0,
                                           int row_bytes, int X0, int Y, int W, const uint16_t* list, int n_list,
                                           const int32_t* __restrict__ pi, const double* __restrict__ pd, int NP,
                                           int J, int P, double b2, const int32_t* __restrict__ lseg,
                                           const int32_t* __restrict__ ln, int LS, int lt,
                                           const int32_t* __restrict__ clr) {
  uint32_t w[4] = {0, 0, 0, 0};
  if (srow) {
    if (VEC) {
      const uint4 q = *reinterpret_cast<const uint4*>(srow + byte0);
      w[0] = q.x;
      w[1] = q.y;
      w[2] = q.z;
      w[3] = q.w;
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (byte0 + i < row_bytes) w[i >> 2] |= (uint32_t)srow[byte0 + i] << (8 * (i & 3));
    }
  }
  if (n_list > 0) {
    int col[OVL_CHUNK_PIX];
#pragma unroll
    for (int k = 0; k < OVL_CHUNK_PIX; ++k) col[k] = -1;
    // descending: the list is ascending in (animal, slot), so the first hit of a pixel is its highest animal
    for (int e = n_list - 1; e >= 0; --e) {
      const int idx = list[e];
      const int32_t* q = pi + (size_t)idx * 8;
      const int x0 = q[4], y0 = q[5], x1 = q[6], y1 = q[7];
      if (Y < y0 || Y > y1 || X0 + OVL_CHUNK_PIX - 1 < x0 || X0 > x1) continue;
      const int animal = idx / NP, slot = idx - animal * NP;
      if (LBL && slot == NP - 1) {
        int n = ln[animal];
        n = n < 0 ? 0 : (n > LS ? LS : n);
        const int ox = q[1], oy = q[2], pad = (lt + 1) / 2;
        const int64_t t2 = (int64_t)lt * lt;
        const int4* g = reinterpret_cast<const int4*>(lseg) + (size_t)animal * LS;
        for (int i = 0; i < n; ++i) {
          const int4 sg = g[i];
          const int ax = ox + sg.x, ay = oy + sg.y, bx = ox + sg.z, by = oy + sg.w;
          if (Y < min(ay, by) - pad || Y > max(ay, by) + pad || X0 + OVL_CHUNK_PIX - 1 < min(ax, bx) - pad ||
              X0 > max(ax, bx) + pad)
            continue;
          const int64_t ex = bx - ax, ey = by - ay, ee = ex * ex + ey * ey;
          const int64_t wy = Y - ay, vy = Y - by;
#pragma unroll
          for (int k = 0; k < OVL_CHUNK_PIX; ++k) {
            if (col[k] >= 0) continue;
            const int64_t wx = X0 + k - ax, we = wx * ex + wy * ey;
            bool in;
            if (we <= 0) {
              in = 4 * (wx * wx + wy * wy) <= t2;
            } else if (we >= ee) {
              const int64_t vx = X0 + k - bx;
              in = 4 * (vx * vx + vy * vy) <= t2;
            } else {
              const int64_t cr = wx * ey - wy * ex;
              in = 4 * cr * cr <= t2 * ee;
            }
            if (in) col[k] = animal;
          }
        }
      } else if (slot <= J) {
        const int cx = q[1], cy = q[2], r = q[3];
        const int dy = Y - cy, lim = r * r + r - dy * dy;
#pragma unroll
        for (int k = 0; k < OVL_CHUNK_PIX; ++k) {
          const int dx = X0 + k - cx;
          if (col[k] < 0 && dx * dx <= lim) col[k] = animal;
        }
      } else {
        const double* d = pd + ((size_t)animal * P + (slot - J - 1)) * 4;
        const double lx1 = d[0], ly1 = d[1], lx2 = d[2], ly2 = d[3];
        const double ex = lx2 - lx1, ey = ly2 - ly1;
        const double d2 = ex * ex + ey * ey;
        if (!(d2 > 0)) continue;
        const double cx = (lx1 + lx2) / 2, cy = (ly1 + ly2) / 2;
        const double a2 = d2 / 4;
        const double rhs = a2 * b2 * d2;
        const double py = (double)Y - cy;
#pragma unroll
        for (int k = 0; k < OVL_CHUNK_PIX; ++k) {
          const int X = X0 + k;
          const double px = (double)X - cx;
          const double u = px * ex + py * ey, v = py * ex - px * ey;
          if (col[k] < 0 && X >= x0 && X <= x1 && u * u * b2 + v * v * a2 <= rhs) col[k] = animal;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int k = (i + S) / 3, ch = (i + S) % 3;
      if (col[k] >= 0 && X0 + k < W) {
        const int c = (LBL && clr) ? clr[col[k]] : col[k];
        w[i >> 2] = (w[i >> 2] & ~(0xffu << (8 * (i & 3)))) | (animal_colour(c, ch) << (8 * (i & 3)));
      }
    }
  }
  if (VEC) {
    *reinterpret_cast<uint4*>(orow + byte0) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (byte0 + i < row_bytes) orow[byte0 + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  }
}

template <bool VEC, bool LBL>
__global__ __launch_bounds__(OVL_THREADS) void overlay_draw_kernel(
    const uint8_t* __restrict__ frames, int64_t frame_stride, int n_src, const int32_t* __restrict__ src_index, int H,
    int W, int A, int J, int P, int mrksize, const int32_t* __restrict__ prim_i, const double* __restrict__ prim_d,
    uint8_t* __restrict__ out, int tiles_x, OverlayLabels lb) {
  __shared__ uint16_t list[OVL_MAX_ANIMALS * OVL_MAX_PRIMS];
  __shared__ int n_shared;
  const int b = blockIdx.y;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int row_bytes = 3 * W;
  const int NP = J + 1 + P + (LBL ? 1 : 0), N = A * NP;
  const int32_t* lseg = nullptr;
  const int32_t* ln = nullptr;
  const int32_t* clr = nullptr;
  if constexpr (LBL) {
    lseg = lb.seg ? lb.seg + (size_t)b * A * lb.S * 4 : nullptr;
    ln = lb.seg ? lb.n + (size_t)b * A : nullptr;
    clr = lb.colour ? lb.colour + (size_t)b * A : nullptr;
  }
  const int32_t* pi = prim_i + (size_t)b * N * 8;
  const double* pd = prim_d + (size_t)b * A * P * 4;
  const int chunk0 = tx * OVL_TILE_CHUNKS, row0 = ty * OVL_TILE_ROWS;

  // wave 0: the image's valid primitives whose box meets the tile, in ascending order
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const int tx0 = (16 * chunk0) / 3, tx1 = min(W - 1, (16 * (chunk0 + OVL_TILE_CHUNKS) - 1) / 3);
    const int ty0 = row0, ty1 = min(H - 1, row0 + OVL_TILE_ROWS - 1);
    int n = 0;
    for (int base = 0; base < N; base += 64) {
      const int idx = base + lane;
      bool hit = false;
      if (idx < N) {
        const int32_t* q = pi + (size_t)idx * 8;
        hit = q[0] != 0 && q[4] <= tx1 && q[6] >= tx0 && q[5] <= ty1 && q[7] >= ty0;
      }
      const unsigned long long m = __ballot(hit);
      if (hit) list[n + __popcll(m & ((1ull << lane) - 1))] = (uint16_t)idx;
      n += __popcll(m);
    }
    if (lane == 0) n_shared = n;
  }
  __syncthreads();
  const int n_list = n_shared;

  const int src = src_index[b];
  const uint8_t* simg = (src >= 0 && src < n_src) ? frames + (size_t)src * (size_t)frame_stride : nullptr;
  uint8_t* oimg = out + (size_t)b * H * row_bytes;
  const int chunk = chunk0 + (threadIdx.x % OVL_TILE_CHUNKS);
  const int byte0 = 16 * chunk;
  if (byte0 >= row_bytes) return;
  const int X0 = byte0 / 3, S = byte0 % 3;
  const double b2 = (double)mrksize * (double)mrksize / 4;
  for (int r = threadIdx.x / OVL_TILE_CHUNKS; r < OVL_TILE_ROWS; r += OVL_THREADS / OVL_TILE_CHUNKS) {
    const int Y = row0 + r;
    if (Y >= H) break;
    const uint8_t* srow = simg ? simg + (size_t)Y * row_bytes : nullptr;
    uint8_t* orow = oimg + (size_t)Y * row_bytes;
    if (S == 0)
      draw_chunk<0, VEC, LBL>(srow, orow, byte0, row_bytes, X0, Y, W, list, n_list, pi, pd, NP, J, P, b2, lseg, ln,
                               lb.S, lb.t, clr);
    else if (S == 1)
      draw_chunk<1, VEC, LBL>(srow, orow, byte0, row_bytes, X0, Y, W, list, n_list, pi, pd, NP, J, P, b2, lseg, ln,
                               lb.S, lb.t, clr);
    else
      draw_chunk<2, VEC, LBL>(srow, orow, byte0, row_bytes, X0, Y, W, list, n_list, pi, pd, NP, J, P, b2, lseg, ln,
                               lb.S, lb.t, clr);
  }
}

// ------------------------------------------------------------------------------------------- launchers
int overlay_primitives(const double* cams, int C, const int32_t* cam_of_img, const double* kp3d, const double* score,
                       int B, int A, int J, const OverlaySkeleton& sk, int mrksize, int32_t* prim_i, double* prim_d,
                       hipStream_t s) {
  if (B <= 0 || A <= 0) return 0;
  if (A > OVL_MAX_ANIMALS || J < 7 || sk.n_pairs < 0 || J + 1 + sk.n_pairs > OVL_MAX_PRIMS) return -2;
  hipLaunchKernelGGL(overlay_prims_kernel<false>, dim3(B * A), dim3(64), 0, s, cams, C, cam_of_img, kp3d, score, A, J,
                     sk, mrksize, prim_i, prim_d, OverlayLabels{});
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int overlay_primitives_labelled(const double* cams, int C, const int32_t* cam_of_img, const double* kp3d,
                                const double* score, int B, int A, int J, const OverlaySkeleton& sk, int mrksize,
                                const OverlayLabels& lb, int32_t* prim_i, double* prim_d, hipStream_t s) {
  if (B <= 0 || A <= 0) return 0;
  if (A > OVL_MAX_ANIMALS || J < 7 || sk.n_pairs < 0 || J + 2 + sk.n_pairs > OVL_MAX_PRIMS) return -2;
  if (lb.S < 0 || lb.S > OVL_MAX_LABEL_SEGS || lb.t < 1 || lb.t > 32 || (lb.seg && !lb.n)) return -2;
  hipLaunchKernelGGL(overlay_prims_kernel<true>, dim3(B * A), dim3(64), 0, s, cams, C, cam_of_img, kp3d, score, A, J,
                     sk, mrksize, prim_i, prim_d, lb);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int overlay_draw(const uint8_t* frames, int64_t frame_stride, int n_src, const int32_t* src_index, int B, int H, int W,
                 int A, int J, int P, int mrksize, const int32_t* prim_i, const double* prim_d, uint8_t* out,
                 hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  if (A < 0 || A > OVL_MAX_ANIMALS || J + 1 + P > OVL_MAX_PRIMS || B > 65535) return -2;
  const int row_bytes = 3 * W;
  const int tiles_x = (row_bytes + 16 * OVL_TILE_CHUNKS - 1) / (16 * OVL_TILE_CHUNKS);
  const int tiles_y = (H + OVL_TILE_ROWS - 1) / OVL_TILE_ROWS;
  // 16-byte accesses when every row of every image starts on a 16-byte boundary
  const bool vec = row_bytes % 16 == 0 && frame_stride % 16 == 0 && (uintptr_t)frames % 16 == 0 &&
                   (uintptr_t)out % 16 == 0;
  const dim3 grid(tiles_x * tiles_y, B);
  if (vec)
    hipLaunchKernelGGL((overlay_draw_kernel<true, false>), grid, dim3(OVL_THREADS), 0, s, frames, frame_stride, n_src,
                       src_index, H, W, A, J, P, mrksize, prim_i, prim_d, out, tiles_x, OverlayLabels{});
  else
    hipLaunchKernelGGL((overlay_draw_kernel<false, false>), grid, dim3(OVL_THREADS), 0, s, frames, frame_stride, n_src,
                       src_index, H, W, A, J, P, mrksize, prim_i, prim_d, out, tiles_x, OverlayLabels{});
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int overlay_draw_labelled(const uint8_t* frames, int64_t frame_stride, int n_src, const int32_t* src_index, int B,
                          int H, int W, int A, int J, int P, int mrksize, const OverlayLabels& lb,
                          const int32_t* prim_i, const double* prim_d, uint8_t* out, hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  if (A < 0 || A > OVL_MAX_ANIMALS || J + 2 + P > OVL_MAX_PRIMS || B > 65535) return -2;
  if (lb.S < 0 || lb.S > OVL_MAX_LABEL_SEGS || lb.t < 1 || lb.t > 32 || (lb.seg && !lb.n)) return -2;
  const int row_bytes = 3 * W;
  const int tiles_x = (row_bytes + 16 * OVL_TILE_CHUNKS - 1) / (16 * OVL_TILE_CHUNKS);
  const int tiles_y = (H + OVL_TILE_ROWS - 1) / OVL_TILE_ROWS;
  const bool vec = row_bytes % 16 == 0 && frame_stride % 16 == 0 && (uintptr_t)frames % 16 == 0 &&
                   (uintptr_t)out % 16 == 0;
  const dim3 grid(tiles_x * tiles_y, B);
  if (vec)
    hipLaunchKernelGGL((overlay_draw_kernel<true, true>), grid, dim3(OVL_THREADS), 0, s, frames, frame_stride, n_src,
                       src_index, H, W, A, J, P, mrksize, prim_i, prim_d, out, tiles_x, lb);
  else
    hipLaunchKernelGGL((overlay_draw_kernel<false, true>), grid, dim3(OVL_THREADS), 0, s, frames, frame_stride, n_src,
                       src_index, H, W, A, J, P, mrksize, prim_i, prim_d, out, tiles_x, lb);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mq
