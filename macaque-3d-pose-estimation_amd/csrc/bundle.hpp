// Internal launcher of the rig bundle adjustment (bundle.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mq {

constexpr int BA_MAXC_API = 16;  // cameras (OPT_MAXC)
constexpr int BA_GP_API = 9;     // mode 2: parameter slots per camera
constexpr int BA_GFIX_API = 11;  // mode 2: fixed doubles per camera (model first)

// stop reasons written to info[3]
constexpr int BA_STOP_MAX_ITER = 1;  // max_iter trial steps taken
constexpr int BA_STOP_FTOL = 2;      // accepted relative cost decrease below ftol (gain ratio above 1/4)
constexpr int BA_STOP_XTOL = 3;      // step norm below xtol * (xtol + |x|)
constexpr int BA_STOP_LAMBDA = 4;    // damping above 1e16 without an acceptable step (or nothing to solve)

size_t bundle_workspace_bytes(int mode, int C, int N);

// cam: host (C, P) in / out; X: device (N, 3) in / out; obs: device (C, N, 2); use: device (N, C);
// resid: device (N, C, 2) or null, the residuals at the returned parameters (0 where unobserved);
// info: host, 8 doubles: initial cost, final cost, trial steps, stop reason, accepted steps, final lambda,
// linearisations, free camera parameters.  Returns 0, or a negative HIP / argument error.
int bundle_adjust(int mode, int C, int N, double* cam, double* X, const double* obs, const uint8_t* use,
                  int fix_cam0, double ftol, double xtol, int max_iter, double* resid, double* info, void* ws,
                  hipStream_t s);

// Mode 2, aniposelib's CameraGroup.bundle_adjust (cameras.py:894-980): cam is HOST (C, 9) in / out -- rvec, tvec,
// f, k1, k2; cam_fixed is HOST (C, 11) -- the model (camera.hpp's ids), then cx, cy (pinhole, fisheye) or K00,
// K01, K02, K11, K12, xi, D[4] (omnidir); free_mask is HOST (C * 9): the columns the solve may move (a column
// whose camera nobody observes is removed as well).  The rest as bundle_adjust; workspace of mode 2.
int bundle_adjust_group(int C, int N, double* cam, const double* cam_fixed, const uint8_t* free_mask, double* X,
                        const double* obs, const uint8_t* use, double ftol, double xtol, int max_iter,
                        double* resid, double* info, void* ws, hipStream_t s);

}  // namespace mq
