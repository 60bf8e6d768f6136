// Camera-motion compensation (cmc.hip): SIFT + 2-NN match + partial-affine RANSAC, restating boxmot 12.0.7
// cmc/sift.py SIFT.apply stage by stage (tests/cmc_ref.py is the numpy restatement the kernels mirror).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mq {

constexpr int CMC_KCAND = 4096;   // DoG extrema refined per image (scan order octave, layer, row, column)
constexpr int CMC_MAXPEAK = 4;    // orientation peaks kept per extremum (lowest bins first)
constexpr int CMC_MAX_OCT = 8;
constexpr int CMC_KP = 7;         // floats per keypoint: x, y, size, angle, octave, layer, response
constexpr int CMC_KMAX = 2048;    // largest max_kp any entry point accepts
constexpr int CMC_MAX_HYP = 2000;

// Pyramid layout of one image (the same for every image of a batch): octave o holds 6 Gaussian and 5 DoG
// layers of h[o] x w[o] floats at g_off[o] / d_off[o] of the per-image arena, and 3 layers of extremum
// flags (bytes) at f_off[o].
struct SiftGeom {
  int n_oct, first_octave, img_h, img_w;
  int h[CMC_MAX_OCT], w[CMC_MAX_OCT];
  int g_off[CMC_MAX_OCT], d_off[CMC_MAX_OCT], f_off[CMC_MAX_OCT + 1];
  int arena;  // floats per image
};

struct SiftWs;  // pyramid + candidate workspace, grown on demand
SiftWs* sift_ws_create();
void sift_ws_destroy(SiftWs* ws);

int sift_geometry(int h, int w, int first_octave, SiftGeom* g);
int64_t sift_dog_floats(const SiftGeom& g);

// uint8 BGR frames (n, H, W, 3) -> uint8 gray (n, h, w), h = rint(H scale), w = rint(W scale)
int cmc_preprocess(const uint8_t* frames, int64_t frame_stride, int n, int H, int W, double scale, uint8_t* gray,
                   hipStream_t s);
// 255 inside the 2 % border, 0 inside every scaled box; boxes (n, max_boxes, 4) f64 x1 y1 x2 y2 full resolution
int cmc_mask(const double* boxes, const int32_t* box_counts, int max_boxes, int n, int h, int w, double scale,
             uint8_t* mask, hipStream_t s);
// builds the pyramid of every image and writes the sorted keypoints (n, max_kp, 7) and counts (n)
int sift_detect(SiftWs* ws, const uint8_t* gray, int n, int h, int w, int first_octave, const uint8_t* mask, int max_kp,
                float* kps, int32_t* counts, float* dog_out, hipStream_t s);
// gray == nullptr: the pyramid of the last sift_detect / sift_describe call on ws is reused
int sift_describe(SiftWs* ws, const uint8_t* gray, int n, int h, int w, int first_octave, const float* kps,
                  const int32_t* counts, int max_kp, uint8_t* desc, hipStream_t s);
// query image i is q_index[i] (null: i) of the query arrays; idx / dist (n, max_kp, 2) int32
int desc_match_knn2(const uint8_t* query, const int32_t* n_query, const int32_t* q_index, const uint8_t* train,
                    const int32_t* n_train, int n, int max_kp, int32_t* idx, int32_t* dist, hipStream_t s);
// ratio test, spatial gate, boxmot's one-sided 2.5 sigma rule -> good (n, max_kp, 4) f64 [px, py, cx, cy]
int cmc_match_filter(const int32_t* idx, const int32_t* dist, const float* prev_kps, const int32_t* n_prev,
                     const int32_t* q_index, const float* cur_kps, const int32_t* n_cur, int n, int max_kp, int h, int w,
                     double* tmp, double* good, int32_t* n_knn, int32_t* n_good, hipStream_t s);
// pts (n, max_pts, 4) f64 [sx, sy, dx, dy]; warps (n, 6) f64; info (n, 2) int32 [hypothesis, inliers]
int affine_partial_ransac(const double* pts, const int32_t* counts, int n, int max_pts, double thresh, double* warps,
                          int32_t* info, uint8_t* mask, hipStream_t s);
// previous-frame state of slot slots[i] := image i
int cmc_store_prev(const float* kps, const uint8_t* desc, const int32_t* counts, const int32_t* slots, int n, int max_kp,
                   float* prev_kps, uint8_t* prev_desc, int32_t* prev_counts, hipStream_t s);

}  // namespace mq
