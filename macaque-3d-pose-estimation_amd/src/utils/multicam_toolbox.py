"""multicam_toolbox point functions used by steps 2-3 (row a17) and the rig calibration, backed by libmq_hip.

``undistortPoints(config_path, pos_2d, omnidir, camparam)`` and
``triangulatePoints(config_path, pos_2d_undist, frame_use, use_optim_extrin, camparam)``
keep the reference signatures (multicam_toolbox.py:393-486).  The ``camparam``
dict path is supported (``camera_id``, ``K``, ``xi``, ``D`` and ``pmat`` = [R|t]
per camera); the h5 path needs h5py, which this image lacks, and raises.
Only omnidir undistortion is on the path (step2/3 call it with omnidir=True).

The calibration chain: ``analyze_chessboardvid`` (:22-72, calibration video -> chessboard corners, detected in
``mqhip.chessboard``, csrc/chessboard.hip; frame stores instead of mp4), ``calibrate_intrinsic`` (:74-116, chessboard corners ->
``cam_intrinsic.h5``'s ``mtx``, ``dist``, ``K``, ``xi``, ``D``) and ``get_extrinsic_from_cagekeypoints`` (:213-242,
cage annotations -> ``cam_extrinsic.h5``'s ``rvec``, ``tvec``) fit cameras to points in ``mqhip.calib``
(csrc/calib.hip); ``optimize_extrinsic`` / ``optimize_all_camera_params`` (:488-824) refine the rig on a marker
trace in ``mqhip.bundle`` (csrc/bundle.hip) and produce the calibration the steps read.  That trace comes from
``analyze_aruco_marker_vid`` / ``analyze_aruco_cube_vid`` (:244-391, marker video -> the marker's centre per frame,
detected in ``mqhip.aruco``, csrc/aruco.hip; the caller passes the 4 x 4 dictionary), which live in the sibling
module ``src.utils.multicam_aruco``: this module's own surface stays as it was.  What else needs images
stays out: the labelling GUI (:118-211), ``saveimg`` (``cv2.drawChessboardCorners``), ``disp_result``
and mp4 input.  ``fix_extrinsic_optim``
(:942-974) is not provided either: it edits ``cam_extrinsic_optim.h5`` in place through h5py's append mode and
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


# ----------------------------------------------------------------------------- calibration from detected points
def _camera_ids(config_path):
    import yaml
    with open(config_path, 'r') as f:
        return yaml.safe_load(f)


def chessboard_objp(square_size):
    """:34-35: the board coordinates of the 54 inner corners, x fastest over 9, y over 6."""
    objp = np.zeros((6 * 9, 3), np.float64)
    objp[:, :2] = np.mgrid[0:9, 0:6].T.reshape(-1, 2) * square_size
    return objp


def analyze_chessboardvid(config_path, saveimg=False, frame_intv=5, *, stores=None, device: int = 0, batch: int = 8,
                          win: int = 11, scale=None, square_size=None):
    """multicam_toolbox.analyze_chessboardvid (:22-72) on the GPU.  Per camera id, frames ``range(10, n, frame_intv)``
    (:50) of its calibration video go through ``mqhip.chessboard.find_chessboard_corners`` (BGR2GRAY, the 9 x 6
    detector, ``cornerSubPix`` with window (win, win), zero zone (-1, -1), criteria (30, 0.001), :57-61) in batches
    of ``batch``; the views where the board was found are kept.

    ``stores`` = {camera id: frames}, uint8 (n, H, W, 3) BGR or (n, H, W) gray (a numpy array, an
    ``mqhip.io.MjpegFrames`` or anything indexable by frame), keeps files out of it; ``square_size`` is then needed
    unless ``config_path`` names a config with ``chessboard_square_size``.  Otherwise ``camera_id``,
    ``chessboard_square_size`` and ``chessboard_vid_folder`` come from ``config_path`` and camera ``id`` reads the
    frame store ``<chessboard_vid_folder>/<id>*`` (an ``mqhip.io.FrameStore`` directory, ``npy`` or ``mjpeg``; the
    reference's ``<id>*.mp4`` is out of scope).

    Returns {id: {'imp': (V, 54, 1, 2) float32, 'objp': (V, 54, 3) float64}}, what
    ``calibrate_intrinsic(chessboard_points=...)`` takes, and writes ``chessboard_points.h5`` next to the config
    (:40, :71-72) only when h5py imports and the frames came from the config's stores.  ``saveimg`` raises
    ``NotImplementedError`` (``cv2.drawChessboardCorners``).  The default ``win`` is the reference's 11, which needs
    corners more than about 24 px apart (mqhip.chessboard)."""
    if saveimg:
        raise NotImplementedError("saveimg draws with cv2.drawChessboardCorners, which this build does not have")
    import glob

    from mqhip import chessboard
    from_cfg = stores is None
    cfg = None
    if from_cfg or square_size is None:
        cfg = _camera_ids(config_path)
        square_size = cfg['chessboard_square_size'] if square_size is None else square_size
    if from_cfg:
        from mqhip.io import FrameStore
        vid_dir = os.path.dirname(config_path) + '/' + cfg['chessboard_vid_folder']
        stores = {}
        for i in cfg['camera_id']:
            found = sorted(d for d in glob.glob(vid_dir + '/' + str(i) + '*') if os.path.isdir(d))
            if not found:
                raise FileNotFoundError(f"no frame store {vid_dir}/{i}* (mp4 input is out of scope)")
            stores[i] = FrameStore(found[0], device=device)
    objp = chessboard_objp(square_size)
    out = {}
    for i, frames in stores.items():
        index = None
        if hasattr(frames, 'frame_index'):          # a FrameStore: stored frame k is frames[frame_index[k]]
            index, frames = frames.frame_index, frames.frames
        n = len(frames) if index is None else len(index)
        pick = list(range(10, n, frame_intv))
        imgpoints = []
        print(i)
        for at in range(0, len(pick), max(1, int(batch))):
            ks = pick[at:at + max(1, int(batch))]
            ks = ks if index is None else [int(index[k]) for k in ks]
            if hasattr(frames, 'device_frames'):
                block = frames.device_frames(ks, device=device)
            else:
                block = np.stack([np.asarray(frames[k]) for k in ks])
            ok, corners = chessboard.find_chessboard_corners(block, scale=scale, win=win, criteria=(30, 0.001),
                                                             device=device)
            imgpoints.extend(corners[v].astype(np.float32)[:, np.newaxis, :] for v in range(len(ks)) if ok[v])
        V = len(imgpoints)
        out[i] = {'imp': np.stack(imgpoints) if V else np.zeros((0, 54, 1, 2), np.float32),
                  'objp': np.tile(objp[np.newaxis], (V, 1, 1))}
    if from_cfg:
        try:
            import h5py
        except ImportError:
            h5py = None
        if h5py is not None:
            with h5py.File(os.path.dirname(config_path) + '/chessboard_points.h5', mode='w') as f:
                for i, d in out.items():
                    f.create_dataset('/' + str(i) + '/imp', data=d['imp'])
                    f.create_dataset('/' + str(i) + '/objp', data=d['objp'])
    return out


def _h5_or_raise():
    try:
        import h5py  # absent in this image; the reference's files are read and written only when it imports
    except ImportError:
        _require_camparam(None)
    return h5py


def calibrate_intrinsic(config_path, mtx_init=None, dist_init=None, *, chessboard_points=None, img_size=None,
                        device: int = 0, return_info=False):
    """multicam_toolbox.calibrate_intrinsic (:74-116) on the GPU.  Per camera id, from the detected chessboard
    corners ``imp`` (V, 54, 1, 2) and their board coordinates ``objp`` (V, 54, 3): one pinhole fit gives ``mtx``
    (3, 3) and ``dist`` (1, 5) (``cv2.calibrateCamera``, flags 0, :88) and one omnidir fit gives ``K`` (3, 3), ``xi``
    (1, 1), ``D`` (1, 4) (``cv2.omnidir.calibrate`` with CALIB_USE_GUESS + CALIB_FIX_SKEW + CALIB_FIX_CENTER and
    criteria (200, 1e-8), :100-111).  All cameras go through one ``mqhip.calib.calibrate_views`` call per model.

    ``chessboard_points`` = {camera id: {'imp': ..., 'objp': ...}} and ``img_size`` = (width, height) keep files out
    of it.  Otherwise h5py must import: ``camera_id`` and ``img_size`` come from ``config_path``,
    ``chessboard_points.h5`` next to it is read and ``cam_intrinsic.h5`` is written (:80-116).

    Returns a camparam-style dict that ``get_extrinsic_from_cagekeypoints``, ``optimize_extrinsic`` and the
    calibration.toml writer take as it is: ``camera_id``, ``mtx``, ``dist``, ``K``, ``xi``, ``D`` per camera, plus
    ``rms`` (the omnidir fit's, px) and ``rms_pinhole``, the omnidir fit's per-view poses ``view_rvecs`` /
    ``view_tvecs`` (V arrays (3, 1) per camera; ``rvecs`` / ``tvecs`` stay free for the rig's extrinsics) and
    ``idx``, every view (this fit drops none).  With ``return_info`` also the solver's info dicts.

    Not pinned against OpenCV, which is not a dependency: the start (Zhang's closed form
    with the centre at ((w - 1) / 2, (h - 1) / 2); the omnidir start doubles fx, fy and sets xi = 1), the frozen
    omnidir centre (w / 2 - 0.5, h / 2 - 0.5), and ``mtx_init`` / ``dist_init``: here they replace the closed-form
    focal length and the zero distortion as the pinhole start; whether cv2 with flags 0 honours them is not
    known."""
    from mqhip import calib
    from_h5 = chessboard_points is None
    if from_h5:
        h5py = _h5_or_raise()
        cfg = _camera_ids(config_path)
        ID = list(cfg['camera_id'])
        img_size = img_size or cfg['img_size']
        base = os.path.dirname(config_path)
        chessboard_points = {}
        with h5py.File(base + '/chessboard_points.h5', mode='r') as f:
            for i in ID:
                chessboard_points[i] = {'imp': f[str(i)]['imp'][()], 'objp': f[str(i)]['objp'][()]}
    else:
        ID = list(chessboard_points.keys())
        if img_size is None:
            raise ValueError("img_size = (width, height) is needed with chessboard_points")
    if not ID:
        raise ValueError("no camera to calibrate")
    obj, img, vpp = [], [], []
    for i in ID:
        imp = np.asarray(chessboard_points[i]['imp'], dtype=np.float64)
        objp = np.asarray(chessboard_points[i]['objp'], dtype=np.float64)
        if imp.ndim < 3 or imp.shape[-1] != 2 or objp.ndim != 3 or objp.shape[-1] != 3:
            raise ValueError(f"camera {i}: imp must be (V, n, 1, 2) and objp (V, n, 3), got {imp.shape} and {objp.shape}")
        imp = imp.reshape(imp.shape[0], -1, 2)
        if imp.shape[:2] != objp.shape[:2]:
            raise ValueError(f"camera {i}: {imp.shape[:2]} image points for {objp.shape[:2]} object points")
        vpp.append(imp.shape[0])
        obj.extend(objp)
        img.extend(imp)
    size = (int(img_size[0]), int(img_size[1]))
    k_init = None
    if mtx_init is not None:
        k_init = np.tile(calib.pinhole_slots(mtx_init, np.zeros(5) if dist_init is None else dist_init), (len(ID), 1))
    elif dist_init is not None:
        raise ValueError("dist_init needs mtx_init")
    kp, _, rms_p, info_p = calib.calibrate_views(calib.MODEL_PINHOLE, obj, img, vpp, size, intrinsics0=k_init,
                                                device=device)
    ko, poses, rms_o, info_o = calib.calibrate_views(calib.MODEL_OMNIDIR, obj, img, vpp, size, device=device)
    out = {'camera_id': ID, 'mtx': [], 'dist': [], 'K': [], 'xi': [], 'D': [], 'rms': [float(r) for r in rms_o],
           'rms_pinhole': [float(r) for r in rms_p], 'view_rvecs': [], 'view_tvecs': [], 'idx': []}
    at = 0
    for c, V in enumerate(vpp):
        mtx, dist = calib.pinhole_from_slots(kp[c])
        K, xi, D = calib.omnidir_from_slots(ko[c])
        for key, val in (('mtx', mtx), ('dist', dist), ('K', K), ('xi', xi), ('D', D)):
            out[key].append(val)
        out['view_rvecs'].append([poses[v, :3].reshape(3, 1).copy() for v in range(at, at + V)])
        out['view_tvecs'].append([poses[v, 3:].reshape(3, 1).copy() for v in range(at, at + V)])
        out['idx'].append(np.arange(V, dtype=np.int32)[np.newaxis, :])
        at += V
    if from_h5:
        with h5py.File(base + '/cam_intrinsic.h5', mode='w') as f:
            for c, i in enumerate(ID):
                for key in ('mtx', 'dist', 'K', 'xi', 'D'):
                    f.create_dataset('/' + str(i) + '/' + key, data=out[key][c])
    return (out, {'pinhole': info_p, 'omnidir': info_o}) if return_info else out


def get_extrinsic_from_cagekeypoints(config_path, *, cagepoints=None, camparam=None, device: int = 0):
    """multicam_toolbox.get_extrinsic_from_cagekeypoints (:213-242) on the GPU: each camera's pose in the cage's
    frame from its annotated cage keypoints, ``cv2.solvePnP(objp, imgp, mtx, dist)`` (:234) as the pose-only case of
    ``mqhip.calib.calibrate_views``, all cameras in one call.

    ``cagepoints`` = {camera id: (n, 6) rows of flag, u, v, X, Y, Z}: rows with flag > 0 are used, the pixels are
    annotated on the 640-wide preview and scaled by 2048 / 640 (:229-232).  ``camparam`` carries ``camera_id``,
    ``mtx`` and ``dist`` (``calibrate_intrinsic``'s result).  Otherwise h5py must import:
    ``cagepoints_annotation.h5`` and ``cam_intrinsic.h5`` next to ``config_path`` are read and ``cam_extrinsic.h5``
    is written with ``rvec`` (3, 1), ``tvec`` (3, 1) (:236-237).  Prints the camera positions as :239-242 does and
    returns the camparam with ``rvecs`` / ``tvecs`` (3, 1) per camera added.

    A planar set of keypoints needs 4 points, any other 6 (``ValueError`` otherwise); the planarity rule is
    cv2.solvePnP's as recalled, not pinned."""
    from mqhip import calib
    from mqhip.geometry import rodrigues
    from_h5 = cagepoints is None or camparam is None
    if from_h5:
        h5py = _h5_or_raise()
        base = os.path.dirname(config_path)
        if camparam is None:
            ID = list(_camera_ids(config_path)['camera_id'])
            camparam = {'camera_id': ID, 'mtx': [], 'dist': []}
            with h5py.File(base + '/cam_intrinsic.h5', mode='r') as f:
                for i in ID:
                    camparam['mtx'].append(np.asarray(f[str(i)]['mtx'][()], dtype=np.float64))
                    camparam['dist'].append(np.asarray(f[str(i)]['dist'][()], dtype=np.float64))
        if cagepoints is None:
            with h5py.File(base + '/cagepoints_annotation.h5', mode='r') as f:
                cagepoints = {i: f[str(i)][()] for i in camparam['camera_id']}
    ID = list(camparam['camera_id'])
    if 'mtx' not in camparam or 'dist' not in camparam:
        raise ValueError("camparam needs mtx and dist (calibrate_intrinsic's result)")
    obj, img, k = [], [], []
    for c, i in enumerate(ID):
        cp = np.asarray(cagepoints[i], dtype=np.float64)
        if cp.ndim != 2 or cp.shape[1] != 6:
            raise ValueError(f"camera {i}: cage points must be (n, 6) rows of flag, u, v, X, Y, Z, got {cp.shape}")
        cp = cp[cp[:, 0] > 0, 1:]
        img.append(cp[:, 0:2] * 2048 / 640)
        obj.append(cp[:, 2:])
        k.append(calib.pinhole_slots(camparam['mtx'][c], camparam['dist'][c]))
    _, poses, _, _ = calib.calibrate_views(calib.MODEL_PINHOLE, obj, img, [1] * len(ID), (2048, 1536),
                                           free_mask=np.zeros(calib.N_SLOTS), intrinsics0=np.stack(k),
                                           max_iter=100, xtol=1e-12, device=device)
    out = {key: (list(v) if isinstance(v, (list, tuple)) else v) for key, v in camparam.items()}
    out['rvecs'] = [poses[c, :3].reshape(3, 1).copy() for c in range(len(ID))]
    out['tvecs'] = [poses[c, 3:].reshape(3, 1).copy() for c in range(len(ID))]
    if from_h5:
        with h5py.File(base + '/cam_extrinsic.h5', mode='w') as f:
            for c, i in enumerate(ID):
                f.create_dataset('/' + str(i) + '/rvec', data=out['rvecs'][c])
                f.create_dataset('/' + str(i) + '/tvec', data=out['tvecs'][c])
    for c, i in enumerate(ID):
        print('3D pos of camera ' + str(i))
        print(-rodrigues(poses[c, :3]).T @ out['tvecs'][c])
    return out


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
