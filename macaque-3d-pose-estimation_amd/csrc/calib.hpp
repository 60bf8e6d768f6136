// Internal launchers of the view calibration (calib.hip): camera intrinsics and one pose per view from detected
// points (the reference's calibrate_intrinsic, multicam_toolbox.py:74-116) and the pose-only case (solvePnP in
// get_extrinsic_from_cagekeypoints, :213-242).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mq {

constexpr int CAL_NI_API = 10;  // intrinsic slots per problem (calib_dev.hpp CAL_NI)

// what calib_init reports beyond HIP errors (positive: the input cannot be initialised)
constexpr int CAL_INIT_NONPLANAR = 1;  // a non-planar view without given intrinsics (Zhang's init needs planes)
constexpr int CAL_INIT_SINGULAR = 2;   // Zhang's focal-length system is singular or gives no finite length
constexpr int CAL_INIT_FEW = 3;        // a non-planar view with fewer than 6 points
constexpr int CAL_INIT_POSE = 4;       // a pose came out non-finite (degenerate points)

size_t calib_workspace_bytes(int n_prob, int n_views, int n_pts);

// Host: view_prefix (n_prob + 1), pt_prefix (n_views + 1), intr (n_prob, 10) in / out, poses (n_views, 6) out.
// Device: obj (n_pts, 3), img (n_pts, 2).  On a positive return intr and poses are untouched and *where is the
// index of the first view (or problem, for CAL_INIT_SINGULAR) that failed.
int calib_init(int model, int n_prob, int n_views, int n_pts, const int* view_prefix, const int* pt_prefix,
               const double* obj, const double* img, int width, int height, int use_intrinsics, double* intr,
               double* poses, int* where, void* ws, hipStream_t s);

// As above, plus host free_mask (n_prob, 10), device resid (n_pts, 2) or null, host info (n_prob, 8) in
// bundle.hpp's layout (info[7]: unknowns of the problem, free intrinsic slots + 6 per view).
int calibrate_views(int model, int n_prob, int n_views, int n_pts, const int* view_prefix, const int* pt_prefix,
                    const double* obj, const double* img, const uint8_t* free_mask, double ftol, double xtol,
                    int max_iter, double* intr, double* poses, double* resid, double* info, void* ws, hipStream_t s);

}  // namespace mq
