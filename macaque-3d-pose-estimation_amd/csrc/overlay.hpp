// Internal launchers of the pose-overlay kernels (overlay.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mq {

constexpr int OVL_MAX_ANIMALS = 8;   // animals per image
constexpr int OVL_MAX_PRIMS = 64;    // disc slots + limb slots per animal

// joint flags of a skeleton table
constexpr int OVL_JOINT_DISC = 1;    // draw_kps draws a disc at the joint
constexpr int OVL_JOINT_NULLED = 2;  // clean_kp sets the joint to None before anything is drawn

// The skeleton, passed to the kernel by value.  Slots 0..J are the joints and the neck (slot J).
struct OverlaySkeleton {
  uint8_t pair_a[OVL_MAX_PRIMS], pair_b[OVL_MAX_PRIMS];  // limb p joins slots pair_a[p], pair_b[p]
  uint8_t radius[OVL_MAX_PRIMS];                         // disc radius per slot
  uint8_t flags[OVL_MAX_PRIMS];                          // OVL_JOINT_* per slot
  int n_pairs;
};

// prim_i int32 (B, A, J + 1 + P, 8): valid, cx, cy, r, x0, y0, x1, y1;  prim_d float64 (B, A, P, 4): x1, y1, x2, y2
int overlay_primitives(const double* cams, int C, const int32_t* cam_of_img, const double* kp3d, const double* score,
                       int B, int A, int J, const OverlaySkeleton& sk, int mrksize, int32_t* prim_i, double* prim_d,
                       hipStream_t s);
int overlay_draw(const uint8_t* frames, int64_t frame_stride, int n_src, const int32_t* src_index, int B, int H, int W,
                 int A, int J, int P, int mrksize, const int32_t* prim_i, const double* prim_d, uint8_t* out,
                 hipStream_t s);

}  // namespace mq
