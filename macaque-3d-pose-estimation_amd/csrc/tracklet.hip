// Step-3 tracklet lift (step3_crossframematching.py calc_3dtrace :274-302, get_graph's calc_p3d
// :1115-1130, count_id_detections :839-870): per (tracklet, frame) cell, gather each camera's row that
// carries the tracklet's box id, undistort and pinv-DLT the joints, and reduce the joints to the
// per-axis nanmedian / nanmean the host stages compare.  Compiled with -ffp-contract=off.
//
// One wave per cell.  Lanes 0..C-1 scan their camera's rows of the frame (CSR) for the last row with
// the cell's box id; lanes 0..J-1 then lift one joint each from the selected rows (17 joints x 8
// cameras x 24 B read per cell); lanes 0..2 reduce one axis each over the joints in LDS.
#include "common.hpp"
#include "camera.hpp"
#include "dlt_dev.hpp"
#include "geometry.hpp"

namespace mq {

constexpr int TRK_MAXJ = 32;

template <int MAXC>
__global__ __launch_bounds__(64) void tracklet_traces_kernel(
    const double* __restrict__ cams, int C, const int32_t* __restrict__ row_start,
    const int32_t* __restrict__ row_tid, const double* __restrict__ row_kp, int R, int F, int J,
    const int32_t* __restrict__ trk, int K, const int32_t* __restrict__ cells, int N, double thr_kp,
    double* __restrict__ p3d, double* __restrict__ median, double* __restrict__ mean) {
  __shared__ int sel[MAXC];
  __shared__ double pj[TRK_MAXJ][3];
  __shared__ double srt[3][TRK_MAXJ];
  const int n = blockIdx.x;
  const int lane = threadIdx.x;
  if (n >= N) return;
  const int k = cells[2 * n], f = cells[2 * n + 1];
  const bool cell_ok = k >= 0 && k < K && f >= 0 && f < F;

  // lanes 0..C-1: the last row of (camera, frame) whose id is the cell's box id; negative ids never match
  int mine = -1;
  bool present = false;
  if (cell_ok && lane < C) {
    const int want = trk[((size_t)k * F + f) * C + lane];
    present = want >= 0;
    if (present) {
      int lo = row_start[(size_t)lane * (F + 1) + f], hi = row_start[(size_t)lane * (F + 1) + f + 1];
      lo = lo < 0 ? 0 : lo;
      hi = hi > R ? R : hi;
      for (int r = lo; r < hi; ++r)
        if (row_tid[r] == want) mine = r;
    }
  }
  if (lane < MAXC) sel[lane] = mine;
  const int n_present = __popcll(__ballot(present));
  __syncthreads();

  // lanes 0..J-1: one joint each
  double p[3] = {NAN, NAN, NAN};
  if (lane < J) {
    double ux[MAXC], uy[MAXC];
    unsigned use = 0;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      ux[c] = uy[c] = 0;
      const int r = (c < C) ? sel[c] : -1;
      if (r >= 0) {
        const double* q = row_kp + ((size_t)r * J + lane) * 3;
        const double x = q[0], y = q[1], s = q[2];
        if (!(x != x) && !(s < thr_kp)) {  // calc_3dpose :262-268: x not NaN and not (score < thr)
          omni_undistort(cam_at(cams, c), x, y, ux[c], uy[c]);
          use |= 1u << c;
        }
      }
    }
    pinv_dlt_solve<MAXC>(cams, C, ux, uy, use, p);
    pj[lane][0] = p[0];
    pj[lane][1] = p[1];
    pj[lane][2] = p[2];
  }
  __syncthreads();
  const bool skip = n_present < 2;  // calc_3dtrace :283 leaves the frame NaN; calc_p3d has no such skip
  if (p3d && lane < J) {
    double* o = p3d + ((size_t)n * J + lane) * 3;
    o[0] = skip ? NAN : p[0];
    o[1] = skip ? NAN : p[1];
    o[2] = skip ? NAN : p[2];
  }
  if (lane < 3) {
    // np.nanmean: sum of the finite joints in joint order / their count; np.nanmedian: insertion sort
    double* v = srt[lane];
    int m = 0;
    double sum = 0.0;
    for (int j = 0; j < J; ++j) {
      const double x = pj[j][lane];
      if (x != x) continue;
      sum = sum + x;
      int i = m++;
      while (i > 0 && v[i - 1] > x) {
        v[i] = v[i - 1];
        --i;
      }
      v[i] = x;
    }
    double med = NAN, avg = NAN;
    if (m > 0) {
      avg = sum / (double)m;
      med = (m & 1) ? v[m / 2] : (v[m / 2 - 1] + v[m / 2]) / 2.0;
    }
    median[(size_t)n * 3 + lane] = skip ? NAN : med;
    mean[(size_t)n * 3 + lane] = avg;
  }
}

// count_id_detections (:839-870): one thread per cell; every row of every camera carrying the cell's box
// id and an ID score above conf_thr adds one vote to its class.
constexpr int TRK_MAXCLS = 16;

__global__ void tracklet_votes_kernel(int C, const int32_t* __restrict__ row_start,
                                      const int32_t* __restrict__ row_tid, const int32_t* __restrict__ row_cls,
                                      const double* __restrict__ row_score, int R, int F,
                                      const int32_t* __restrict__ trk, int K, const int32_t* __restrict__ cells,
                                      int N, double conf_thr, int n_class, int32_t* __restrict__ votes) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int cnt[TRK_MAXCLS];
#pragma unroll
  for (int i = 0; i < TRK_MAXCLS; ++i) cnt[i] = 0;
  const int k = cells[2 * n], f = cells[2 * n + 1];
  if (k >= 0 && k < K && f >= 0 && f < F) {
    for (int c = 0; c < C; ++c) {
      const int want = trk[((size_t)k * F + f) * C + c];
      if (want < 0) continue;
      int lo = row_start[(size_t)c * (F + 1) + f], hi = row_start[(size_t)c * (F + 1) + f + 1];
      lo = lo < 0 ? 0 : lo;
      hi = hi > R ? R : hi;
      for (int r = lo; r < hi; ++r) {
        if (row_tid[r] != want || !(row_score[r] > conf_thr)) continue;
        const int cls = row_cls[r];
#pragma unroll
        for (int i = 0; i < TRK_MAXCLS; ++i)
          if (i == cls) ++cnt[i];
      }
    }
  }
  for (int i = 0; i < n_class; ++i) votes[(size_t)n * n_class + i] = cnt[i];
}

int tracklet_traces(const double* cams, int C, const int32_t* row_start, const int32_t* row_tid,
                    const double* row_kp, int R, int F, int J, const int32_t* trk, int K, const int32_t* cells,
                    int N, double thr_kp, double* p3d, double* median, double* mean, hipStream_t s) {
  if (N <= 0) return 0;
  if (J < 1 || J > TRK_MAXJ) return -2;
  if (C <= 8)
    hipLaunchKernelGGL(tracklet_traces_kernel<8>, dim3(N), dim3(64), 0, s, cams, C, row_start, row_tid, row_kp, R, F,
                       J, trk, K, cells, N, thr_kp, p3d, median, mean);
  else if (C <= 16)
    hipLaunchKernelGGL(tracklet_traces_kernel<16>, dim3(N), dim3(64), 0, s, cams, C, row_start, row_tid, row_kp, R,
                       F, J, trk, K, cells, N, thr_kp, p3d, median, mean);
  else
    return -2;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int tracklet_id_votes(int C, const int32_t* row_start, const int32_t* row_tid, const int32_t* row_cls,
                      const double* row_score, int R, int F, const int32_t* trk, int K, const int32_t* cells, int N,
                      double conf_thr, int n_class, int32_t* votes, hipStream_t s) {
  if (N <= 0) return 0;
  if (n_class < 1 || n_class > TRK_MAXCLS) return -2;
  hipLaunchKernelGGL(tracklet_votes_kernel, dim3((N + 127) / 128), dim3(128), 0, s, C, row_start, row_tid, row_cls,
                     row_score, R, F, trk, K, cells, N, conf_thr, n_class, votes);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mq
