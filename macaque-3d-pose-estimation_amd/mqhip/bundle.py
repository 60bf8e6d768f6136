"""Bundle adjustment of the camera rig on the GPU: the solve inside the reference's
``multicam_toolbox.optimize_extrinsic`` (:523-612) and ``optimize_all_camera_params`` (:696-777), through
``mq_bundle_adjust`` (csrc/bundle.hip).  A Schur-complement Levenberg-Marquardt with Marquardt scaling stands
in for scipy's trust-region-reflective solver.  No CPU fallback.
"""
from __future__ import annotations

import numpy as np

MAX_CAMS = 16                      # csrc/bundle_dev.hpp BA_MAXC
N_PARAMS = {0: 6, 1: 16}           # rvec, tvec [, K00, K01, K02, K11, K12, xi, D[4]] (multicam_toolbox.py:692-694)
STOP_REASONS = {1: "max_iter", 2: "ftol", 3: "xtol", 4: "damping exhausted"}
DEFAULT_FTOL = {0: 1e-5, 1: 1e-3}  # the reference's values (:611, :639)


def select_points(use):
    """Indices of the points the reference keeps (:523, :696): seen by at least 2 cameras."""
    use = np.asarray(use, dtype=bool)
    return np.argwhere(np.sum(use, axis=1) >= 2).ravel()


def free_columns(mode, use, fix_cam0=True):
    """Indices into the raveled (C, P) camera parameters that the solve may move: every parameter of a camera
    that some point in use observes, minus camera 0's rvec and tvec under ``fix_cam0`` (:585-586, :746-747).
    The library removes the other columns from the reduced system (``info['n_free']`` counts what is left)."""
    use = np.asarray(use, dtype=bool)
    P = N_PARAMS[mode]
    seen = use[select_points(use)].any(axis=0)
    return np.array([c * P + p for c in range(use.shape[1]) for p in range(P)
                     if seen[c] and not (fix_cam0 and c == 0 and p < 6)], dtype=np.int64)


def bundle_adjust(cam_params, points3d, obs, use, mode, fix_cam0=True, ftol=None, max_iter=200, xtol=1e-8,
                  return_residuals=False, device: int = 0):
    """Refine ``cam_params`` (C, 6) [mode 0] or (C, 16) [mode 1] and ``points3d`` (N, 3) on observations
    ``obs`` (C, N, 2) marked by ``use`` (N, C).

    Mode 0 observations are undistorted (normalised) points, mode 1 observations are pixels.  Points seen by
    fewer than 2 cameras are left out of the solve and come back unchanged; a camera nobody observes keeps its
    parameters; ``fix_cam0`` freezes camera 0's rvec and tvec (its intrinsics stay free in mode 1).
    ``max_iter`` counts trial steps, accepted or not; 0 only evaluates.

    Returns ``(cam_params, points3d, info)``; info holds ``cost0``, ``cost`` (1/2 sum r^2), ``iterations``,
    ``accepted``, ``stop`` (a STOP_REASONS value), ``lambda``, ``linearisations``, ``n_free``, ``n_points`` and,
    with ``return_residuals``, ``residuals`` (N, C, 2) at the returned parameters (0 where unused).
    """
    import torch

    from . import _lib
    if mode not in N_PARAMS:
        raise ValueError(f"mode must be 0 or 1, got {mode}")
    P = N_PARAMS[mode]
    cam = np.array(cam_params, dtype=np.float64)
    pts = np.array(points3d, dtype=np.float64)
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    use = np.asarray(use, dtype=bool)
    if cam.ndim != 2 or cam.shape[1] != P or not 1 <= cam.shape[0] <= MAX_CAMS:
        raise ValueError(f"cam_params must be (C <= {MAX_CAMS}, {P}) in mode {mode}, got {cam.shape}")
    C = cam.shape[0]
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"points3d must be (N, 3), got {pts.shape}")
    N = pts.shape[0]
    if obs.shape != (C, N, 2) or use.shape != (N, C):
        raise ValueError(f"obs must be {(C, N, 2)} and use {(N, C)}, got {obs.shape} and {use.shape}")
    if ftol is None:
        ftol = DEFAULT_FTOL[mode]
    keep = select_points(use)
    if keep.size == 0:
        raise ValueError("no point is seen by at least 2 cameras")
    if not (np.isfinite(pts[keep]).all() and np.isfinite(obs.transpose(1, 0, 2)[keep][use[keep]]).all()):
        raise ValueError("non-finite point or observation among the points in use")
    dev = torch.device("cuda", device)
    ctx = _lib.Context.get(device)
    n = int(keep.size)
    # unused observations may hold anything (NaN, -1): the kernels never read them, zero them anyway
    obs_k = np.where(use[keep].T[:, :, None], obs[:, keep, :], 0.0)
    x_d = torch.from_numpy(np.ascontiguousarray(pts[keep])).to(dev)
    obs_d = torch.from_numpy(np.ascontiguousarray(obs_k)).to(dev)
    use_d = torch.from_numpy(np.ascontiguousarray(use[keep], dtype=np.uint8)).to(dev)
    res_d = torch.zeros((n, C, 2), dtype=torch.float64, device=dev) if return_residuals else None
    cam_h = np.ascontiguousarray(cam)
    info_h = np.zeros(8, dtype=np.float64)
    _lib.check(ctx.lib.mq_bundle_adjust(ctx.handle, int(mode), C, n, cam_h.ctypes.data, _lib.ptr(x_d),
                                        _lib.ptr(obs_d), _lib.ptr(use_d), int(bool(fix_cam0)), float(ftol),
                                        float(xtol), int(max_iter), _lib.ptr(res_d), info_h.ctypes.data,
                                        _lib.stream_ptr(dev)), "mq_bundle_adjust")
    pts[keep] = x_d.cpu().numpy()
    info = {"cost0": float(info_h[0]), "cost": float(info_h[1]), "iterations": int(info_h[2]),
            "stop": STOP_REASONS[int(info_h[3])], "accepted": int(info_h[4]), "lambda": float(info_h[5]),
            "linearisations": int(info_h[6]), "n_free": int(info_h[7]), "n_points": n}
    if return_residuals:
        r = np.zeros((N, C, 2))
        r[keep] = res_d.cpu().numpy()
        info["residuals"] = r
    return cam_h, pts, info


# ----------------------------------------------------------------------------- aniposelib's CameraGroup.bundle_adjust
N_GROUP_PARAMS = 9                 # csrc/bundle_dev.hpp BA_GP: rvec, tvec, f, k1, k2 (cameras.py:279-299)
N_GROUP_FIXED = 11                 # BA_GFIX: model, then cx, cy or K00, K01, K02, K11, K12, xi, D[4]
MODEL_OMNIDIR = 0                  # csrc/camera.hpp CamModel


def group_free_mask(models, extra_dist):
    """(C, 9) bool: the slots aniposelib's parametrisation moves.  rvec, tvec, f, k1 of every camera, k2 only
    with ``extra_dist`` (cameras.py:279-299); an omnidir camera projects with K, xi, D, which set_params does not
    touch (:509-529), so only its rvec and tvec are free."""
    models = np.asarray(models).ravel()
    mask = np.ones((models.size, N_GROUP_PARAMS), dtype=bool)
    mask[:, 8] = bool(extra_dist)
    mask[models == MODEL_OMNIDIR, 6:] = False
    return mask


def bundle_adjust_group(cam_fixed, cam_params, free_mask, points3d, obs, use, ftol=1e-4, max_iter=1000, xtol=1e-8,
                        return_residuals=False, device: int = 0):
    """The solve inside aniposelib's ``CameraGroup.bundle_adjust`` (cameras.py:894-980, ``extra=None``,
    ``loss='linear'``) through ``mq_bundle_adjust_group``: refine ``cam_params`` (C, 9) -- rvec, tvec, f, k1, k2 --
    and ``points3d`` (N, 3) on pixel observations ``obs`` (C, N, 2) marked by ``use`` (N, C).

    ``cam_fixed`` (C, 11) holds each camera's model and what the solve does not move (include/mq_hip.h);
    ``free_mask`` (C, 9) the columns it may move (``group_free_mask``).  Unlike ``bundle_adjust`` every point
    stays in the solve, as in the reference: a point one camera sees moves through the damping alone, a point
    nobody sees keeps its value.  No camera is fixed; the 7 gauge freedoms are left to the damping.

    Returns ``(cam_params, points3d, info)`` with ``bundle_adjust``'s info; ``residuals`` are projection - pixel.
    """
    import torch

    from . import _lib
    fixed = np.ascontiguousarray(cam_fixed, dtype=np.float64)
    cam = np.array(cam_params, dtype=np.float64)
    mask = np.ascontiguousarray(free_mask, dtype=np.uint8)
    pts = np.array(points3d, dtype=np.float64)
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    use = np.asarray(use, dtype=bool)
    if cam.ndim != 2 or cam.shape[1] != N_GROUP_PARAMS or not 1 <= cam.shape[0] <= MAX_CAMS:
        raise ValueError(f"cam_params must be (C <= {MAX_CAMS}, {N_GROUP_PARAMS}), got {cam.shape}")
    C = cam.shape[0]
    if fixed.shape != (C, N_GROUP_FIXED) or mask.shape != (C, N_GROUP_PARAMS):
        raise ValueError(f"cam_fixed must be {(C, N_GROUP_FIXED)} and free_mask {(C, N_GROUP_PARAMS)}, got "
                         f"{fixed.shape} and {mask.shape}")
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError(f"points3d must be (N >= 1, 3), got {pts.shape}")
    N = pts.shape[0]
    if obs.shape != (C, N, 2) or use.shape != (N, C):
        raise ValueError(f"obs must be {(C, N, 2)} and use {(N, C)}, got {obs.shape} and {use.shape}")
    if not (np.isfinite(pts).all() and np.isfinite(obs.transpose(1, 0, 2)[use]).all()):
        raise ValueError("non-finite point or observation in use")
    dev = torch.device("cuda", device)
    ctx = _lib.Context.get(device)
    obs_k = np.where(use.T[:, :, None], obs, 0.0)      # what nobody uses is never read: zero it anyway
    x_d = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
    obs_d = torch.from_numpy(np.ascontiguousarray(obs_k)).to(dev)
    use_d = torch.from_numpy(np.ascontiguousarray(use, dtype=np.uint8)).to(dev)
    res_d = torch.zeros((N, C, 2), dtype=torch.float64, device=dev) if return_residuals else None
    cam_h = np.ascontiguousarray(cam)
    info_h = np.zeros(8, dtype=np.float64)
    rc = ctx.lib.mq_bundle_adjust_group(ctx.handle, C, N, fixed.ctypes.data, cam_h.ctypes.data, mask.ctypes.data,
                                        _lib.ptr(x_d), _lib.ptr(obs_d), _lib.ptr(use_d), float(ftol), float(xtol),
                                        int(max_iter), _lib.ptr(res_d), info_h.ctypes.data, _lib.stream_ptr(dev))
    if rc == -2:
        raise ValueError(ctx.lib.mq_last_error().decode())
    _lib.check(rc, "mq_bundle_adjust_group")
    info = {"cost0": float(info_h[0]), "cost": float(info_h[1]), "iterations": int(info_h[2]),
            "stop": STOP_REASONS[int(info_h[3])], "accepted": int(info_h[4]), "lambda": float(info_h[5]),
            "linearisations": int(info_h[6]), "n_free": int(info_h[7]), "n_points": N}
    if return_residuals:
        info["residuals"] = res_d.cpu().numpy()
    return cam_h, x_d.cpu().numpy(), info
