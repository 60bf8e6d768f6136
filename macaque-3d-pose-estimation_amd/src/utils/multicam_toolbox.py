"""multicam_toolbox point functions used by steps 2-3 (row a17) and the rig calibration refinement
(``optimize_extrinsic``, ``optimize_all_camera_params``), backed by libmq_hip.

``undistortPoints(config_path, pos_2d, omnidir, camparam)`` and
``triangulatePoints(config_path, pos_2d_undist, frame_use, use_optim_extrin, camparam)``
keep the reference signatures (multicam_toolbox.py:393-486).  The ``camparam``
dict path is supported (``camera_id``, ``K``, ``xi``, ``D`` and ``pmat`` = [R|t]
per camera); the h5 path needs h5py, which this image lacks, and raises.
Only omnidir undistortion is on the path (step2/3 call it with omnidir=True).

``optimize_extrinsic`` / ``optimize_all_camera_params`` (:488-824) produce the refined calibration the steps read
(``cam_extrinsic_optim.h5``); their solve runs in ``mqhip.bundle`` (csrc/bundle.hip).  ``fix_extrinsic_optim``
(:942-974) is not provided: it edits ``cam_extrinsic_optim.h5`` in place through h5py's append mode and
``applytransform``, which is file surgery rather than array work.
"""
import os

import numpy as np

from mqhip.geometry import CameraGroup, OmnidirCamera, triangulate_pinv


def _group_from_camparam(camparam, with_extrinsics=False, device: int = 0):
    cams = []
    for i, cid in enumerate(camparam['camera_id']):
        rvec = np.zeros(3)
        tvec = np.zeros(3)
        cams.append(OmnidirCamera(K=np.asarray(camparam['K'][i], dtype=np.float64),
                                  xi=float(np.ravel(camparam['xi'][i])[0]),
                                  D=np.asarray(camparam['D'][i], dtype=np.float64).ravel(),
                                  rvec=rvec, tvec=tvec, name=str(cid), size=[2048, 1536]))
    return CameraGroup(cams, device=device)


def _require_camparam(camparam):
    if camparam is None:
        raise NotImplementedError("the h5 calibration path needs h5py (absent); pass camparam")


def undistortPoints(config_path, pos_2d, omnidir=False, camparam=None, device: int = 0):
    """list/array of per-camera (N,2) pixels -> list of per-camera (N,2) normalized points."""
    _require_camparam(camparam)
    if not omnidir:
        raise NotImplementedError("pinhole cv2.undistortPoints is not on the omnidir pipeline's path")
    g = _group_from_camparam(camparam, device=device)
    pts = np.stack([np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in pos_2d])
    und = g.undistort_points(pts)
    return [np.squeeze(u) for u in und]


def triangulatePoints(config_path, pos_2d_undist, frame_use, use_optim_extrin=True, camparam=None,
                      device: int = 0):
    """(C, N, 2) undistorted + frame_use (N, C) -> (N, 3), NaN where < 2 cameras are used."""
    _require_camparam(camparam)
    C = len(camparam['camera_id'])
    cams = []
    for i, cid in enumerate(camparam['camera_id']):
        P = np.asarray(camparam['pmat'][i], dtype=np.float64)
        cams.append(OmnidirCamera.from_projection(P, name=str(cid)))
    g = CameraGroup(cams, device=device)
    und = np.stack([np.asarray(u, dtype=np.float64).reshape(-1, 2) for u in pos_2d_undist[:C]])
    return triangulate_pinv(g, und, np.asarray(frame_use, dtype=bool))


# ----------------------------------------------------------------------------- rig calibration refinement
def ba_frame_use(pos_2d):
    """:501-507 (and :653-659): the last 5 rows of the trace are not used; a camera sees the marker in a frame
    when its x is >= 0.  Returns (n_frame, frame_use (n_frame, n_cam) bool)."""
    n_frame = np.asarray(pos_2d[0]).shape[0] - 5
    if n_frame <= 0:
        raise ValueError("the marker trace needs more than 5 frames")
    frame_use = np.stack([np.asarray(p, dtype=np.float64)[:n_frame, 0] >= 0.0 for p in pos_2d], axis=1)
    return n_frame, frame_use


def _calib_arrays(config_path, camparam, marker_trace, file_intrin=None, file_extrin=None):
    """The inputs as arrays: (camparam dict, per-camera traces, came_from_h5)."""
    if camparam is not None and marker_trace is not None:
        return camparam, [np.asarray(p, dtype=np.float64) for p in marker_trace], False
    try:
        import h5py  # absent in this image; the reference's files are read only when it imports
    except ImportError:
        _require_camparam(None)
    import yaml
    base = os.path.dirname(config_path)
    with open(config_path, 'r') as f:
        ID = yaml.safe_load(f)['camera_id']
    if marker_trace is None:
        with h5py.File(base + '/marker_trace.h5', mode='r') as f:
            marker_trace = [f[str(i)][()] for i in ID]
    if camparam is None:
        camparam = {'camera_id': list(ID), 'K': [], 'xi': [], 'D': [], 'mtx': [], 'dist': [], 'rvecs': [], 'tvecs': []}
        with h5py.File(file_extrin or base + '/cam_extrinsic.h5', mode='r') as f:
            for i in ID:
                rvec = np.asarray(f[str(i)]['rvec'][()], dtype=np.float64)
                camparam['rvecs'].append(rvec.reshape(3, 1))           # (3,) or (3, 1) (:684-685)
                camparam['tvecs'].append(np.asarray(f[str(i)]['tvec'][()], dtype=np.float64).reshape(3, 1))
        with h5py.File(file_intrin or base + '/cam_intrinsic.h5', mode='r') as f:
            for i in ID:
                for key, name in (('K', 'K'), ('xi', 'xi'), ('D', 'D'), ('mtx', 'mtx'), ('dist', 'dist')):
                    camparam[key].append(np.asarray(f[str(i)][name][()], dtype=np.float64))
    return camparam, [np.asarray(p, dtype=np.float64) for p in marker_trace], True


def _with_pmat(camparam):
    from mqhip.geometry import rodrigues
    cp = dict(camparam)
    cp['pmat'] = [np.hstack([rodrigues(np.ravel(r)), np.asarray(t, dtype=np.float64).reshape(3, 1)])
                  for r, t in zip(camparam['rvecs'], camparam['tvecs'])]
    return cp


def _ba_undistort(config_path, pos_2d, omnidir, camparam, device):
    if omnidir:
        return undistortPoints(config_path, pos_2d, True, camparam, device=device)
    if 'mtx' not in camparam or 'dist' not in camparam:
        raise NotImplementedError("omnidir=False undistorts with cam_intrinsic.h5's mtx / dist (:423-427): "
                                  "pass them in camparam['mtx'] / camparam['dist'], or use omnidir=True")
    from mqhip.geometry import Camera
    cams = [Camera(matrix=m, dist=np.ravel(d), name=str(i))
            for i, m, d in zip(camparam['camera_id'], camparam['mtx'], camparam['dist'])]
    pts = np.stack([np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in pos_2d])
    return list(CameraGroup(cams, device=device).undistort_points(pts))


def _ba_setup(config_path, omnidir, camparam, pos_2d, frame_use, device):
    """:509-528: undistort, triangulate with the initial extrinsics, keep the frames at least 2 cameras see."""
    from mqhip.bundle import select_points
    und = _ba_undistort(config_path, pos_2d, omnidir, camparam, device)
    und = [np.asarray(u, dtype=np.float64).reshape(-1, 2) for u in und]
    P3 = triangulatePoints(config_path, und, frame_use, False, _with_pmat(camparam), device=device)
    keep = select_points(frame_use)
    return und, P3, keep


def _write_extrinsic_h5(path, ID, cam):
    import h5py
    with h5py.File(path, mode='w') as f:       # :615-621, :780-786: rvec (3,), tvec (3, 1)
        for i, cid in enumerate(ID):
            f.create_dataset('/' + str(cid) + '/rvec', data=cam[i, :3].ravel())
            f.create_dataset('/' + str(cid) + '/tvec', data=cam[i, 3:6].ravel()[:, np.newaxis])


def _result_camparam(camparam, cam):
    """The refined parameters in the camparam layout (rvecs / tvecs (3, 1), K (3, 3), xi (1, 1), D (1, 4), pmat)."""
    out = {k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in camparam.items()}
    C = cam.shape[0]
    out['rvecs'] = [cam[i, :3].reshape(3, 1).copy() for i in range(C)]
    out['tvecs'] = [cam[i, 3:6].reshape(3, 1).copy() for i in range(C)]
    if cam.shape[1] == 16:
        out['K'] = [np.array([[k[6], k[7], k[8]], [0, k[9], k[10]], [0, 0, 1]]) for k in cam]
        out['xi'] = [np.array([[k[11]]]) for k in cam]
        out['D'] = [k[12:16][np.newaxis, :].copy() for k in cam]
    return _with_pmat(out)


def _write_toml(path, cp):
    """calibration.toml in the layout step 4 writes and steps 2-4 read (step4:101-138): matrix = mtx with its
    first two rows halved and distortions = dist when the inputs carry them, zeros otherwise."""
    from mqhip.io import dump_toml
    calib = {}
    for i, cid in enumerate(cp['camera_id']):
        mtx, dist = np.zeros((3, 3)), np.zeros(4)
        if 'mtx' in cp and 'dist' in cp:
            mtx = np.array(cp['mtx'][i], dtype=np.float64)
            mtx[:2, :] /= 2
            dist = np.ravel(cp['dist'][i])
        calib[f'cam_{i}'] = {
            'name': str(cid), 'size': [2048, 1536], 'matrix': mtx.tolist(), 'distortions': dist.tolist(),
            'rotation': np.ravel(cp['rvecs'][i]).tolist(), 'translation': np.ravel(cp['tvecs'][i]).tolist(),
            'fisheye': False, 'omnidir': True, 'xi': np.ravel(cp['xi'][i]).tolist(),
            'K': np.asarray(cp['K'][i]).tolist(), 'D': np.ravel(cp['D'][i]).tolist()}
    dump_toml(calib, path)


def optimize_extrinsic(config_path, show_estimated_campos=True, omnidir=False, fixcam0=True, *, camparam=None,
                       marker_trace=None, write_calibration_toml=None, max_iter=200, return_info=False,
                       device: int = 0):
    """multicam_toolbox.optimize_extrinsic (:488-621) on the GPU: frame mask over ``n_frame - 5`` frames, undistort,
    pinv triangulation with the initial extrinsics, then the 6-parameter-per-camera bundle adjustment
    (``mqhip.bundle.bundle_adjust`` mode 0, ftol 1e-5 as :611).  Returns the refined ``(rvec (3,), tvec (3, 1))``
    per camera (with ``return_info`` also the solver's info dict).

    ``camparam`` (``camera_id``, ``K``, ``xi``, ``D``, ``rvecs``, ``tvecs``; ``mtx`` / ``dist`` for
    ``omnidir=False``) and ``marker_trace`` (per camera (n, 2) pixels, x < 0 = not seen) keep h5 out of it.
    Otherwise h5py must import: ``marker_trace.h5``, ``cam_extrinsic.h5`` and ``cam_intrinsic.h5`` next to
    ``config_path`` are read and ``cam_extrinsic_optim.h5`` is written (:615-621).  ``write_calibration_toml``
    names a calibration.toml to write in the layout steps 2-4 read.  ``show_estimated_campos`` prints the camera
    positions (:623-631).  The reference's debug tail (two more triangulations saved by
    ``scipy.io.savemat('test.mat')``, :633-636) is not reproduced."""
    from mqhip.bundle import bundle_adjust
    camparam, pos_2d, from_h5 = _calib_arrays(config_path, camparam, marker_trace)
    ID = camparam['camera_id']
    n_frame, frame_use = ba_frame_use(pos_2d)
    pos_2d = [p[:n_frame, :2] for p in pos_2d]
    und, P3, keep = _ba_setup(config_path, omnidir, camparam, pos_2d, frame_use, device)
    cam0 = np.stack([np.concatenate([np.ravel(r)[:3], np.ravel(t)[:3]])
                     for r, t in zip(camparam['rvecs'], camparam['tvecs'])])
    cam, _, info = bundle_adjust(cam0, P3[keep], np.stack(und)[:, keep, :], frame_use[keep], mode=0,
                                 fix_cam0=fixcam0, ftol=1e-5, max_iter=max_iter, device=device)
    res = _result_camparam(camparam, cam)
    if from_h5:
        _write_extrinsic_h5(os.path.dirname(config_path) + '/cam_extrinsic_optim.h5', ID, cam)
    if write_calibration_toml:
        _write_toml(write_calibration_toml, res)
    if show_estimated_campos:
        for i, cid in enumerate(ID):
            print(cid, ':', -res['pmat'][i][:, :3].T @ cam[i, 3:6])
    out = [(cam[i, :3].copy(), cam[i, 3:6].reshape(3, 1).copy()) for i in range(len(ID))]
    return (out, info) if return_info else out


def optimize_all_camera_params(config_path, show_estimated_campos=True, omnidir=False, fixcam0=True,
                               n_random_sample=-1, ftol=1e-3, max_nfev=None, mode_eval=False, file_intrin=None,
                               file_extrin=None, verbose=2, *, camparam=None, marker_trace=None, seed=None,
                               write_calibration_toml=None, return_info=False, device: int = 0):
    """multicam_toolbox.optimize_all_camera_params (:638-803) on the GPU: as ``optimize_extrinsic`` up to the
    triangulation, then the 16-parameter-per-camera bundle adjustment on the raw pixels (rvec, tvec, K00, K01,
    K02, K11, K12, xi, D[4]; ``mqhip.bundle.bundle_adjust`` mode 1).  Returns the refined parameters in the
    camparam layout (``rvecs``, ``tvecs``, ``K``, ``xi``, ``D``, ``pmat``).

    ``n_random_sample`` > 0 samples that many frames (:662-666) -- with ``seed`` from ``random.Random(seed)``,
    without from the global ``random`` state as the reference.  ``max_nfev`` bounds the trial steps (200 when
    None).  ``mode_eval`` returns the initial residual vector f0 in the reference's camera-major order (:772-773).
    ``camparam`` / ``marker_trace`` / ``write_calibration_toml`` as in ``optimize_extrinsic``; on the h5 path
    ``cam_extrinsic_optim.h5`` and ``cam_intrinsic_optim.h5`` (K, xi, D refined; mtx, dist copied) are written
    next to ``file_extrin`` / ``file_intrin`` (:780-803).  ``verbose`` is accepted and unused; the debug tail
    (:821-824, ``test.mat``) is not reproduced."""
    import random

    from mqhip.bundle import bundle_adjust
    camparam, pos_2d, from_h5 = _calib_arrays(config_path, camparam, marker_trace, file_intrin, file_extrin)
    ID = camparam['camera_id']
    n_frame, frame_use = ba_frame_use(pos_2d)
    pos_2d = [p[:n_frame, :2] for p in pos_2d]
    if n_random_sample > 0:
        rng = random if seed is None else random.Random(seed)
        I = rng.sample(list(range(n_frame)), n_random_sample)
        pos_2d = [p[I, :] for p in pos_2d]
        frame_use = frame_use[I, :]
    und, P3, keep = _ba_setup(config_path, omnidir, camparam, pos_2d, frame_use, device)
    cam0 = np.zeros((len(ID), 16))
    for i in range(len(ID)):
        K = np.asarray(camparam['K'][i], dtype=np.float64)
        cam0[i, :3] = np.ravel(camparam['rvecs'][i])[:3]
        cam0[i, 3:6] = np.ravel(camparam['tvecs'][i])[:3]
        cam0[i, 6:11] = [K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]]
        cam0[i, 11] = np.ravel(camparam['xi'][i])[0]
        cam0[i, 12:16] = np.ravel(camparam['D'][i])[:4]
    use = frame_use[keep]
    obs = np.stack(pos_2d)[:, keep, :]
    if mode_eval:
        _, _, info = bundle_adjust(cam0, P3[keep], obs, use, mode=1, fix_cam0=fixcam0, ftol=ftol, max_iter=0,
                                   return_residuals=True, device=device)
        r = info['residuals']
        return np.concatenate([r[use[:, c], c, :] for c in range(len(ID))]).ravel()
    cam, _, info = bundle_adjust(cam0, P3[keep], obs, use, mode=1, fix_cam0=fixcam0, ftol=ftol,
                                 max_iter=200 if max_nfev is None else int(max_nfev), device=device)
    res = _result_camparam(camparam, cam)
    if from_h5:
        import h5py
        base = os.path.dirname(config_path)
        file_extrin = file_extrin or base + '/cam_extrinsic.h5'
        file_intrin = file_intrin or base + '/cam_intrinsic.h5'
        _write_extrinsic_h5(os.path.dirname(file_extrin) + '/cam_extrinsic_optim.h5', ID, cam)
        with h5py.File(os.path.dirname(file_intrin) + '/cam_intrinsic_optim.h5', mode='w') as f:
            for i, cid in enumerate(ID):
                f.create_dataset('/' + str(cid) + '/K', data=res['K'][i])
                f.create_dataset('/' + str(cid) + '/xi', data=res['xi'][i])
                f.create_dataset('/' + str(cid) + '/D', data=res['D'][i])
                f.create_dataset('/' + str(cid) + '/mtx', data=np.asarray(camparam['mtx'][i]))
                f.create_dataset('/' + str(cid) + '/dist', data=np.asarray(camparam['dist'][i]))
    if write_calibration_toml:
        _write_toml(write_calibration_toml, res)
    if show_estimated_campos:
        for i, cid in enumerate(ID):
            print(cid)
            print(res['K'][i])
            print(res['xi'][i])
            print(res['D'][i])
        for i, cid in enumerate(ID):
            print(cid, ':', -res['pmat'][i][:, :3].T @ cam[i, 3:6])
    return (res, info) if return_info else res
