"""Camera calibration from detected points on the GPU: the fits the reference takes from OpenCV in
``multicam_toolbox.calibrate_intrinsic`` (:74-116, ``cv2.calibrateCamera`` and ``cv2.omnidir.calibrate``) and in
``get_extrinsic_from_cagekeypoints`` (:213-242, ``cv2.solvePnP``), through ``mq_calib_init`` and
``mq_calibrate_views`` (csrc/calib.hip).  One problem is one camera: 10 intrinsic slots and a pose per view; any
number of independent problems goes through one call.  A Levenberg-Marquardt on the Schur complement of the view
poses stands in for OpenCV's solvers; parity with OpenCV itself is not pinned.  No CPU
fallback.
"""
from __future__ import annotations

import numpy as np

MODEL_OMNIDIR, MODEL_PINHOLE = 0, 1          # csrc/camera.hpp CamModel
N_SLOTS = 10                                 # csrc/calib_dev.hpp CAL_NI
SLOTS = {MODEL_PINHOLE: ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "unused"),
         MODEL_OMNIDIR: ("fx", "fy", "s", "cx", "cy", "xi", "k1", "k2", "p1", "p2")}
# what the reference's calls leave free: cv2.calibrateCamera with flags 0 moves all nine (:88); the omnidir flags
# CALIB_FIX_SKEW + CALIB_FIX_CENTER (:100) freeze s, cx, cy
DEFAULT_FREE = {MODEL_PINHOLE: (1, 1, 1, 1, 1, 1, 1, 1, 1, 0), MODEL_OMNIDIR: (1, 1, 0, 0, 0, 1, 1, 1, 1, 1)}
# (max_iter, xtol): cv2.calibrateCamera's default criteria (30, DBL_EPSILON); the reference's omnidir criteria (:111)
DEFAULT_CRITERIA = {MODEL_PINHOLE: (30, float(np.finfo(np.float64).eps)), MODEL_OMNIDIR: (200, 1e-8)}
STOP_REASONS = {1: "max_iter", 2: "ftol", 3: "xtol", 4: "damping exhausted"}


def pinhole_slots(mtx, dist):
    """``mtx`` (3, 3) and ``dist`` (up to 5: k1, k2, p1, p2, k3) as the pinhole model's 10 slots."""
    mtx = np.asarray(mtx, dtype=np.float64)
    d = np.zeros(5)
    dist = np.ravel(np.asarray(dist, dtype=np.float64))
    if dist.size > 5:
        raise ValueError(f"at most 5 distortion coefficients (k1, k2, p1, p2, k3), got {dist.size}")
    d[:dist.size] = dist
    return np.array([mtx[0, 0], mtx[1, 1], mtx[0, 2], mtx[1, 2], d[0], d[1], d[2], d[3], d[4], 0.0])


def pinhole_from_slots(k):
    """The pinhole slots as ``mtx`` (3, 3), ``dist`` (1, 5) (cv2.calibrateCamera's shapes)."""
    k = np.asarray(k, dtype=np.float64)
    return np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]]), k[4:9][np.newaxis, :].copy()


def omnidir_from_slots(k):
    """The omnidir slots as ``K`` (3, 3), ``xi`` (1, 1), ``D`` (1, 4) (cv2.omnidir.calibrate's shapes)."""
    k = np.asarray(k, dtype=np.float64)
    return np.array([[k[0], k[2], k[3]], [0, k[1], k[4]], [0, 0, 1]]), np.array([[k[5]]]), k[6:10][np.newaxis, :].copy()


def _pack(obj, img, views_per_problem):
    obj = [np.asarray(o, dtype=np.float64).reshape(-1, 3) for o in obj]
    img = [np.asarray(i, dtype=np.float64).reshape(-1, 2) for i in img]
    vpp = [int(v) for v in views_per_problem]
    if len(obj) != len(img) or sum(vpp) != len(obj) or min(vpp, default=0) < 0 or not vpp:
        raise ValueError(f"{len(obj)} object and {len(img)} image point sets for views_per_problem {vpp}")
    for v, (o, i) in enumerate(zip(obj, img)):
        if o.shape[0] != i.shape[0]:
            raise ValueError(f"view {v}: {o.shape[0]} object points and {i.shape[0]} image points")
        if o.shape[0] < 4:
            raise ValueError(f"view {v} has fewer than 4 points")
        if not (np.isfinite(o).all() and np.isfinite(i).all()):
            raise ValueError(f"view {v}: non-finite point")
    view_prefix = np.concatenate([[0], np.cumsum(vpp)]).astype(np.int32)
    pt_prefix = np.concatenate([[0], np.cumsum([o.shape[0] for o in obj])]).astype(np.int32)
    obj_all = np.concatenate(obj) if obj else np.zeros((0, 3))
    img_all = np.concatenate(img) if img else np.zeros((0, 2))
    return np.ascontiguousarray(obj_all), np.ascontiguousarray(img_all), view_prefix, pt_prefix


def calibrate_views(model, obj, img, views_per_problem, image_size, free_mask=None, intrinsics0=None, poses0=None,
                    ftol=0.0, xtol=None, max_iter=None, return_residuals=False, device: int = 0):
    """Fit intrinsics and one pose per view to detected points, for any number of independent cameras at once.

    ``obj`` / ``img``: per view (n, 3) object points and (n, 2) pixels, the views of problem 0 first, then problem
    1's, ...; ``views_per_problem`` their counts (0 is legal: that problem keeps its slots).  ``image_size`` =
    (width, height).  ``free_mask`` (n_prob, 10) or (10,): the slots that move (``DEFAULT_FREE``; all zero is the
    pose-only problem).

    The start: without ``intrinsics0`` the closed-form one (homography per view, Zhang's focal length with the
    centre at ((w - 1) / 2, (h - 1) / 2), zero distortion; omnidir: fx, fy doubled and xi = 1).  With
    ``intrinsics0`` (n_prob, 10) only the poses are started, on pixels normalised through it (a non-planar view
    then needs 6 points).  With ``poses0`` (n_views, 6) as well nothing is started.

    ``max_iter`` trial steps and ``xtol`` default to ``DEFAULT_CRITERIA``; ``ftol`` = 0 leaves the cost rule off, as
    OpenCV has none.  Returns ``(intrinsics (n_prob, 10), poses (n_views, 6), rms (n_prob,), infos)``: rms is
    sqrt(sum |r|^2 / points) in pixels as cv2 reports it (0 for a problem without views), infos a dict per problem
    with mq_bundle_adjust's fields (``residuals`` (n, 2) per view with ``return_residuals``).  Input that cannot be
    started (fewer than 4 points, a non-planar view without intrinsics or with fewer than 6 points, every view
    fronto-parallel) raises ``ValueError``.
    """
    import torch

    from . import _lib
    if model not in SLOTS:
        raise ValueError(f"model must be {MODEL_OMNIDIR} (omnidir) or {MODEL_PINHOLE} (pinhole), got {model}")
    obj_all, img_all, view_prefix, pt_prefix = _pack(obj, img, views_per_problem)
    n_prob, n_views = len(view_prefix) - 1, len(pt_prefix) - 1
    mask = np.asarray(DEFAULT_FREE[model] if free_mask is None else free_mask).astype(bool)
    mask = np.ascontiguousarray(np.broadcast_to(mask, (n_prob, N_SLOTS)), dtype=np.uint8)
    d_iter, d_xtol = DEFAULT_CRITERIA[model]
    max_iter = d_iter if max_iter is None else int(max_iter)
    xtol = d_xtol if xtol is None else float(xtol)
    intr = np.zeros((n_prob, N_SLOTS))
    if intrinsics0 is not None:
        intr = np.array(intrinsics0, dtype=np.float64).reshape(n_prob, N_SLOTS)
    poses = np.zeros((n_views, 6))
    if poses0 is not None:
        if intrinsics0 is None:
            raise ValueError("poses0 needs intrinsics0")
        poses = np.array(poses0, dtype=np.float64).reshape(n_views, 6)
    dev = torch.device("cuda", device)
    ctx = _lib.Context.get(device)
    obj_d = torch.from_numpy(obj_all).to(dev)
    img_d = torch.from_numpy(img_all).to(dev)
    if obj_all.shape[0] == 0:                       # no views at all: keep a valid pointer
        obj_d = torch.zeros((1, 3), dtype=torch.float64, device=dev)
        img_d = torch.zeros((1, 2), dtype=torch.float64, device=dev)

    def call(rc, what):
        if rc == -2:
            raise ValueError(ctx.lib.mq_last_error().decode())
        _lib.check(rc, what)

    if poses0 is None:
        call(ctx.lib.mq_calib_init(ctx.handle, int(model), n_prob, view_prefix.ctypes.data, pt_prefix.ctypes.data,
                                   _lib.ptr(obj_d), _lib.ptr(img_d), int(image_size[0]), int(image_size[1]),
                                   int(intrinsics0 is not None), intr.ctypes.data, poses.ctypes.data,
                                   _lib.stream_ptr(dev)), "mq_calib_init")
    start = (intr.copy(), poses.copy())
    res_d = torch.zeros((max(obj_all.shape[0], 1), 2), dtype=torch.float64, device=dev) if return_residuals else None
    info_h = np.zeros((n_prob, 8))
    call(ctx.lib.mq_calibrate_views(ctx.handle, int(model), n_prob, view_prefix.ctypes.data, pt_prefix.ctypes.data,
                                    _lib.ptr(obj_d), _lib.ptr(img_d), mask.ctypes.data, float(ftol), float(xtol),
                                    max_iter, intr.ctypes.data, poses.ctypes.data, _lib.ptr(res_d),
                                    info_h.ctypes.data, _lib.stream_ptr(dev)), "mq_calibrate_views")
    res = res_d.cpu().numpy() if return_residuals else None
    rms = np.zeros(n_prob)
    infos = []
    for p in range(n_prob):
        v0, v1 = int(view_prefix[p]), int(view_prefix[p + 1])
        n = int(pt_prefix[v1] - pt_prefix[v0])
        row = info_h[p]
        rms[p] = np.sqrt(2.0 * row[1] / n) if n else 0.0
        info = {"cost0": float(row[0]), "cost": float(row[1]), "iterations": int(row[2]),
                "stop": STOP_REASONS[int(row[3])], "accepted": int(row[4]), "lambda": float(row[5]),
                "linearisations": int(row[6]), "n_free": int(row[7]), "n_views": v1 - v0, "n_points": n,
                "intrinsics0": start[0][p], "poses0": start[1][v0:v1]}
        if return_residuals:
            info["residuals"] = [res[pt_prefix[v]:pt_prefix[v + 1]] for v in range(v0, v1)]
        infos.append(info)
    return intr, poses, rms, infos


def solve_pnp(obj, img, mtx, dist, max_iter=100, xtol=1e-12, device: int = 0, return_info=False):
    """The pose of one pinhole camera (``mtx`` (3, 3), ``dist`` up to 5 coefficients) from n object points and
    their pixels: ``cv2.solvePnP(obj, img, mtx, dist)`` (multicam_toolbox.py:234) as the pose-only case of
    ``calibrate_views``.  A planar target needs 4 points, any other 6.  Returns ``rvec (3, 1), tvec (3, 1)``."""
    k = pinhole_slots(mtx, dist)
    _, poses, _, infos = calibrate_views(MODEL_PINHOLE, [obj], [img], [1], (1, 1), free_mask=np.zeros(N_SLOTS),
                                         intrinsics0=k[np.newaxis], max_iter=max_iter, xtol=xtol, device=device)
    out = poses[0, :3].reshape(3, 1).copy(), poses[0, 3:].reshape(3, 1).copy()
    return out + (infos[0],) if return_info else out
