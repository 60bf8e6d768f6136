// Internal launchers of the pose-overlay kernels (overlay.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mq {

constexpr int OVL_MAX_ANIMALS = 8;   // animals per image
constexpr int OVL_MAX_PRIMS = 64;    // disc slots + limb slots (+ the label slot) per animal
constexpr int OVL_MAX_LABEL_SEGS = 96;      // stroke segments of one label
constexpr int OVL_MAX_LABEL_COORD = 8192;   // |segment coordinate| relative to the label origin

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

// The labelled variant's device tables.  colour int32 (B, A) or null (colour = animal index); seg int32
// (B, A, S, 4) x0, y0, x1, y1 relative to the label origin, 16-byte aligned, or null (no labels); n int32 (B, A)
// segments in use; t the stroke thickness.
struct OverlayLabels {
  const int32_t* colour;
  const int32_t* seg;
  const int32_t* n;
  int S, t;
};

// prim_i int32 (B, A, J + 1 + P, 8): valid, cx, cy, r, x0, y0, x1, y1;  prim_d float64 (B, A, P, 4): x1, y1, x2, y2
int overlay_primitives(const double* cams, int C, const int32_t* cam_of_img, const double* kp3d, const double* score,
                       int B, int A, int J, const OverlaySkeleton& sk, int mrksize, int32_t* prim_i, double* prim_d,
                       hipStream_t s);
int overlay_draw(const uint8_t* frames, int64_t frame_stride, int n_src, const int32_t* src_index, int B, int H, int W,
                 int A, int J, int P, int mrksize, const int32_t* prim_i, const double* prim_d, uint8_t* out,
                 hipStream_t s);

// The same with one more slot per animal, the last: prim_i int32 (B, A, J + 2 + P, 8), the label slot holding
// valid, origin x, origin y, 0 and the box of its segments padded by ceil(t / 2).
int overlay_primitives_labelled(const double* cams, int C, const int32_t* cam_of_img, const double* kp3d,
                                const double* score, int B, int A, int J, const OverlaySkeleton& sk, int mrksize,
                                const OverlayLabels& lb, int32_t* prim_i, double* prim_d, hipStream_t s);
int overlay_draw_labelled(const uint8_t* frames, int64_t frame_stride, int n_src, const int32_t* src_index, int B,
                          int H, int W, int A, int J, int P, int mrksize, const OverlayLabels& lb,
                          const int32_t* prim_i, const double* prim_d, uint8_t* out, hipStream_t s);

}  // namespace mq
