// Internal launchers of the candidate kernels (candidates.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mq {
constexpr int CAND_MAX = 4;  // candidates per (instance, joint) and per (camera, point); also imgproc.hip's top-K
int viterbi_filter_multi(const double* kp, int A, int F, int C, int J, int K, double score_thr, int n_back,
                         double thres_dist, void* scratch, size_t scratch_bytes, double* out, hipStream_t s);
size_t viterbi_multi_scratch_bytes(int A, int F, int C, int J, int K, int n_back);
int triangulate_possible(const double* cams, int C, const double* pts, int N, int P, int min_cams, double threshold,
                         double* p3d, uint8_t* picked, double* p2d, double* err, hipStream_t s);
// one candidate per camera (CameraGroup.triangulate_ransac): triangulate_possible at P = 1, picked [C][N]
int triangulate_ransac(const double* cams, int C, const double* pts, int N, int min_cams, double threshold,
                       double* p3d, uint8_t* picked, double* p2d, double* err, hipStream_t s);
}  // namespace mq
