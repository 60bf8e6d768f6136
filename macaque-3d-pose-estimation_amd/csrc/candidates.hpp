// Internal launchers of the candidate kernels (candidates.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mq {
int udp_decode_topk(const float* avg, int n, int joints, int h, int w, const float* center, const float* scale,
                    int in_w, int in_h, int n_cand, int min_sep, float min_score, float* work, double* kp_img,
                    float* score, int32_t* peak, float* kp_hm, hipStream_t s);
int viterbi_filter_multi(const double* kp, int A, int F, int C, int J, int K, double score_thr, int n_back,
                         double thres_dist, void* scratch, double* out, hipStream_t s);
size_t viterbi_multi_scratch_bytes(int A, int F, int C, int J, int K, int n_back);
int triangulate_possible(const double* cams, int C, const double* pts, int N, int P, int min_cams, double threshold,
                         double* p3d, uint8_t* picked, double* p2d, double* err, hipStream_t s);
}  // namespace mq
