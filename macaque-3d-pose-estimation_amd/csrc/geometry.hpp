// Internal launchers of the float64 geometry kernels (geometry.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mq {
int omnidir_undistort(const double* cams, int C, const double* pts, double* out, int N, hipStream_t s);
int omnidir_project(const double* cams, int C, const double* p3d, double* out, int N, hipStream_t s);
int triangulate_dlt(const double* cams, int C, const double* pts, int N, int undistort, double* out, hipStream_t s);
int reprojection_error(const double* cams, int C, const double* p3d, const double* p2d, int N, int mean, double* out,
                       hipStream_t s);
int triangulate_pinv(const double* cams, int C, const double* und, const uint8_t* use, int N, double* out,
                     hipStream_t s);
int geometry_affinity(const double* cams, int C, const double* pts, const int32_t* cam_of_det, int B, int M, int J,
                      double thr_kp, void* ws, size_t ws_bytes, double* out, hipStream_t s);
size_t affinity_workspace_bytes(int B, int M, int J);
int viterbi_filter(const double* kp, int A, int F, int C, int J, double score_thr, int n_back, double thres_dist,
                   void* scratch, size_t scratch_bytes, double* out, hipStream_t s);
size_t viterbi_scratch_bytes(int A, int F, int C, int J, int n_back);
int match_svt(const double* S, const int32_t* n_det, const int32_t* cam_of_det, int B, int Nmax, double alpha,
              double lambda, double mu, double tol, int max_iter, int pselect, void* ws, size_t ws_bytes,
              uint8_t* match, double* x_out, int32_t* iters, hipStream_t s);
size_t match_svt_workspace_bytes(int B, int Nmax);
// step-3 tracklet lift (tracklet.hip)
int tracklet_traces(const double* cams, int C, const int32_t* row_start, const int32_t* row_tid,
                    const double* row_kp, int R, int F, int J, const int32_t* trk, int K, const int32_t* cells,
                    int N, double thr_kp, double* p3d, double* median, double* mean, hipStream_t s);
int tracklet_id_votes(int C, const int32_t* row_start, const int32_t* row_tid, const int32_t* row_cls,
                      const double* row_score, int R, int F, const int32_t* trk, int K, const int32_t* cells, int N,
                      double conf_thr, int n_class, int32_t* votes, hipStream_t s);
}  // namespace mq
