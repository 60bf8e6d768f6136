"""The marker trace of the rig calibration: ``analyze_aruco_marker_vid`` and ``analyze_aruco_cube_vid`` of the
reference's multicam_toolbox (:244-391) on the GPU.  Marker frames go through ``mqhip.aruco.find_markers``
(csrc/aruco.hip, a detector of this project's own for 4 x 4 codes the caller passes), each
marker's pose is the pose-only case of ``mqhip.calib.calibrate_views`` and the projection is ``mq_camera_project``.
The result is the ``marker_trace`` that ``multicam_toolbox.optimize_extrinsic`` reads.

The two functions keep the reference's names and leading arguments but live here, not in ``multicam_toolbox``:
that module's tests pin its surface (``analyze_aruco_marker_vid`` is on their list of names it does not have).
Frame stores instead of mp4; ``disp_result`` is not provided."""
import os

import numpy as np

from mqhip.geometry import CameraGroup

from .multicam_toolbox import _camera_ids, _h5_or_raise


# ----------------------------------------------------------------------------- marker trace
def marker_objp(marker_len):
    """The marker's corners in its own frame, cv2's order (estimatePoseSingleMarkers): top-left, top-right,
    bottom-right, bottom-left = (-+L/2, +-L/2, 0)."""
    L = float(marker_len)
    return np.array([[-L / 2, L / 2, 0], [L / 2, L / 2, 0], [L / 2, -L / 2, 0], [-L / 2, -L / 2, 0]], np.float64)


def _marker_setup(config_path, stores, camparam, folder_key, device):
    """(cfg or {}, stores, camparam with camera_id / mtx / dist, frames_came_from_the_config)."""
    import glob
    from_cfg = stores is None
    cfg = {}
    if config_path is not None and os.path.exists(config_path):
        cfg = _camera_ids(config_path)
    elif from_cfg:
        raise FileNotFoundError(f"no config {config_path!r} and no stores")
    if camparam is None:
        h5py = _h5_or_raise()
        ID = list(cfg['camera_id'])
        camparam = {'camera_id': ID, 'mtx': [], 'dist': []}
        with h5py.File(os.path.dirname(config_path) + '/cam_intrinsic.h5', mode='r') as f:
            for i in ID:
                camparam['mtx'].append(np.asarray(f[str(i)]['mtx'][()], dtype=np.float64))
                camparam['dist'].append(np.asarray(f[str(i)]['dist'][()], dtype=np.float64))
    if 'mtx' not in camparam or 'dist' not in camparam:
        raise ValueError("camparam needs camera_id, mtx and dist (calibrate_intrinsic's result)")
    if from_cfg:
        from mqhip.io import FrameStore
        vid_dir = os.path.dirname(config_path) + '/' + cfg[folder_key]
        stores = {}
        for i in camparam['camera_id']:
            found = sorted(d for d in glob.glob(vid_dir + '/' + str(i) + '*') if os.path.isdir(d))
            if not found:
                raise FileNotFoundError(f"no frame store {vid_dir}/{i}* (mp4 input is out of scope)")
            stores[i] = FrameStore(found[0], device=device)
    return cfg, stores, camparam, from_cfg


def _frame_blocks(frames, pick, batch, device):
    """Blocks of at most ``batch`` frames at the stored positions ``pick``."""
    index = None
    if hasattr(frames, 'frame_index'):          # a FrameStore: stored frame k is frames[frame_index[k]]
        index, frames = frames.frame_index, frames.frames
    for at in range(0, len(pick), max(1, int(batch))):
        ks = pick[at:at + max(1, int(batch))]
        ks = ks if index is None else [int(index[k]) for k in ks]
        if hasattr(frames, 'device_frames'):
            yield frames.device_frames(ks, device=device)
        else:
            yield np.stack([np.asarray(frames[k]) for k in ks])


def _n_frames(frames):
    return len(frames.frame_index) if hasattr(frames, 'frame_index') else len(frames)


def _marker_poses(corner_sets, cam_of_set, camparam, marker_len, device):
    """The pose of every detected marker, ``aruco.estimatePoseSingleMarkers(corners, L, mtx, dist)`` (:289, :365):
    the pose-only case of ``mqhip.calib.calibrate_views``, every marker of a camera a view of that camera's problem,
    all cameras in one call.  Returns poses (n_sets, 6), in the order of ``corner_sets`` sorted by camera."""
    from mqhip import calib
    C = len(camparam['camera_id'])
    k = np.stack([calib.pinhole_slots(camparam['mtx'][c], camparam['dist'][c]) for c in range(C)])
    order = sorted(range(len(corner_sets)), key=lambda j: cam_of_set[j])
    vpp = [sum(1 for j in order if cam_of_set[j] == c) for c in range(C)]
    objp = marker_objp(marker_len)
    poses = np.zeros((len(corner_sets), 6))
    if order:
        _, p, _, _ = calib.calibrate_views(calib.MODEL_PINHOLE, [objp] * len(order), [corner_sets[j] for j in order],
                                           vpp, (1, 1), free_mask=np.zeros(calib.N_SLOTS), intrinsics0=k,
                                           max_iter=100, xtol=1e-12, device=device)
        poses[order] = p
    return poses


def _project_marker_points(poses, cam_of_set, offset, camparam, device):
    """``cv2.projectPoints(offset, rvec, tvec, mtx, dist)`` (:290, :366) for every pose: the point R offset + t in the
    camera's frame through the pinhole projection on the device."""
    from mqhip.geometry import Camera, rodrigues
    out = np.full((len(poses), 2), -1.0)
    offset = np.asarray(offset, dtype=np.float64).reshape(3)
    for c in range(len(camparam['camera_id'])):
        sel = [j for j in range(len(poses)) if cam_of_set[j] == c]
        if not sel:
            continue
        pts = np.stack([rodrigues(poses[j, :3]) @ offset + poses[j, 3:] for j in sel])
        dist = np.zeros(5)
        d = np.ravel(np.asarray(camparam['dist'][c], dtype=np.float64))
        dist[:d.size] = d
        cam = Camera(matrix=np.asarray(camparam['mtx'][c], dtype=np.float64), dist=dist, rvec=np.zeros(3),
                     tvec=np.zeros(3), name=str(camparam['camera_id'][c]))
        out[sel] = CameraGroup([cam], device=device).project(pts)[0]
    return out


def _write_marker_trace(config_path, trace):
    try:
        import h5py
    except ImportError:
        return
    with h5py.File(os.path.dirname(config_path) + '/marker_trace.h5', mode='w') as f:
        for i, C in trace.items():
            f.create_dataset('/' + str(i), data=C)


def _find_markers(block, dictionary, det_size, max_markers, device, cam_id, first_row):
    """``mqhip.aruco.find_markers`` on one block, with its per-axis ratios.  The detector fits quads to the first
    ``mqhip.aruco.MAX_QUADS`` candidate components of a frame in ascending label order, that is from the top of the
    image down; a frame with more candidates (a finely textured scene) is named in a ``RuntimeWarning``, since a
    marker low in such a frame can go unseen and its row would read [-1, -1] like any frame without a marker."""
    import warnings

    from mqhip import aruco
    count, ids, corners, info = aruco.find_markers(block, dictionary, det_size=det_size, max_markers=max_markers,
                                                   device=device, return_info=True)
    over = [(first_row + v, int(n)) for v, n in enumerate(info["candidates"]) if n > aruco.MAX_QUADS]
    if over:
        warnings.warn(f"camera {cam_id}: {len(over)} frame(s) hold more than {aruco.MAX_QUADS} marker candidates and "
                      f"only the first {aruco.MAX_QUADS} from the top were examined (row: candidates) "
                      + ", ".join(f"{r}: {n}" for r, n in over), RuntimeWarning, stacklevel=3)
    return count, corners, info["ratio"]


def analyze_aruco_marker_vid(config_path, disp_result=False, *, stores=None, camparam=None, dictionary=None,
                             det_size=(640, 480), device: int = 0, batch: int = 8):
    """multicam_toolbox.analyze_aruco_marker_vid (:244-305) on the GPU.  Per camera id every frame of its marker
    video goes through ``mqhip.aruco.find_markers`` (resize to ``det_size``, the marker detector; :281-283) in
    batches of ``batch``; where a marker is found the first one's pose is fitted to its four corners (:289) and the
    marker's centre is projected through ``mtx``, ``dist`` (:290); ``[-1, -1]`` elsewhere (:295).

    ``dictionary``: the 4 x 4 codes as 16-bit integers (``mqhip.aruco``); None accepts every dark-bordered quad, which
    is enough here: the trace never uses the id, and the centre is the same point for all four turns.
    ``stores`` = {camera id: frames}, uint8 (n, H, W, 3) BGR or (n, H, W) gray, keeps files out of it; otherwise
    camera ``id`` reads the frame store ``<marker_vid_folder>/<id>*`` (``npy`` or ``mjpeg``; the reference's mp4 is
    out of scope).  ``camparam`` carries ``camera_id``, ``mtx``, ``dist`` (and ``marker_size`` when there is no
    config); otherwise h5py must import and ``cam_intrinsic.h5`` is read (:261-263).

    Returns {id: (n_frames, 2) float64} and writes ``marker_trace.h5`` (:251, :303) only when h5py imports and the
    frames came from the config's stores.  Corners map back to the frame as p ratio + (ratio - 1) / 2, where the
    reference has ``corner * rsize_ratio``.  A frame with more candidate components than the detector examines (64,
    from the top of the image down) raises a ``RuntimeWarning`` that names it.  ``disp_result`` raises ``NotImplementedError`` (``cv2.imshow``)."""
    if disp_result:
        raise NotImplementedError("disp_result draws with cv2.imshow / aruco.drawDetectedMarkers, which this build "
                                  "does not have")
    cfg, stores, camparam, from_cfg = _marker_setup(config_path, stores, camparam, 'marker_vid_folder', device)
    marker_len = cfg.get('marker_size', camparam.get('marker_size', 1.0))
    ID = list(camparam['camera_id'])
    sets, cam_of, where = [], [], []
    n_of = {}
    for c, i in enumerate(ID):
        print(i)
        frames = stores[i]
        n_of[i] = _n_frames(frames)
        at = 0
        for block in _frame_blocks(frames, list(range(n_of[i])), batch, device):
            count, corners, _ = _find_markers(block, dictionary, det_size, 1, device, i, at)
            for v in range(len(count)):
                if count[v] > 0:
                    sets.append(corners[v, 0])
                    cam_of.append(c)
                    where.append((i, at + v))
            at += len(count)
    poses = _marker_poses(sets, cam_of, camparam, marker_len, device)
    centre = _project_marker_points(poses, cam_of, np.zeros(3), camparam, device)
    out = {i: np.full((n_of[i], 2), -1.0) for i in ID}
    for (i, k), p in zip(where, centre):
        out[i][k] = p
    if from_cfg:
        _write_marker_trace(config_path, out)
    return out


def analyze_aruco_cube_vid(config_path, frame_intv=5, disp_result=False, fps=24, *, stores=None, camparam=None,
                           dictionary=None, det_size=(640, 480), device: int = 0, batch: int = 8):
    """multicam_toolbox.analyze_aruco_cube_vid (:307-391) on the GPU: a cube with a marker on each face.  Frames
    ``range(5 fps, n - 5 fps, frame_intv)`` by index (:329; the reference looks each up by time stamp) go through
    the detector; every marker's pose is fitted (:365) and the cube's centre ``(0, 0, -cube_size / 2)`` in the
    marker's frame is projected (:366).  A projection is kept when it lies within ``det_width / 32`` detection pixels
    of the marker's mean corner (:368-369; frame pixels go back to detection pixels with the per-axis ratios, which
    are the reference's single ``rsize_ratio`` for frames of the detection image's shape); the row is the mean of
    the kept projections, ``[-1, -1]`` without one.
    The reference computes and draws that mean (:375-376) but appends the last marker's projection (:377); the mean
    is what this returns.  Arguments and files as ``analyze_aruco_marker_vid``; ``cube_size`` comes from the config
    or from ``camparam['cube_size']``."""
    if disp_result:
        raise NotImplementedError("disp_result draws with cv2.imshow / aruco.drawDetectedMarkers, which this build "
                                  "does not have")
    cfg, stores, camparam, from_cfg = _marker_setup(config_path, stores, camparam, 'marker_vid_folder', device)
    marker_len = cfg.get('marker_size', camparam.get('marker_size', 1.0))
    cube_len = cfg['cube_size'] if 'cube_size' in cfg else camparam['cube_size']
    ID = list(camparam['camera_id'])
    fps = int(fps)
    sets, cam_of, where, anchor = [], [], [], []
    rows = {}
    for c, i in enumerate(ID):
        print(i)
        frames = stores[i]
        pick = list(range(fps * 5, _n_frames(frames) - fps * 5, frame_intv))
        rows[i] = len(pick)
        at = 0
        for block in _frame_blocks(frames, pick, batch, device):
            count, corners, ratio = _find_markers(block, dictionary, det_size, 8, device, i, at)
            ratio = np.asarray(ratio, dtype=np.float64)         # per axis, as mq_find_markers maps the corners
            for v in range(len(count)):
                for m in range(int(count[v])):
                    sets.append(corners[v, m])
                    cam_of.append(c)
                    where.append((i, at + v))
                    anchor.append(((corners[v, m].mean(axis=0) - (ratio - 1.0) / 2.0) / ratio, ratio))
            at += len(count)
    poses = _marker_poses(sets, cam_of, camparam, marker_len, device)
    centre = _project_marker_points(poses, cam_of, np.array([0.0, 0.0, -cube_len / 2.0]), camparam, device)
    kept = {}
    for (i, k), p, (mean_det, ratio) in zip(where, centre, anchor):
        if np.linalg.norm((p - (ratio - 1.0) / 2.0) / ratio - mean_det) < det_size[0] / 32:
            kept.setdefault((i, k), []).append(p)
        else:
            print('warning: cube center estimation ignored; too far from square center')
    out = {i: np.full((rows[i], 2), -1.0) for i in ID}
    for (i, k), P in kept.items():
        out[i][k] = np.mean(np.vstack(P), axis=0)
    if from_cfg:
        _write_marker_trace(config_path, out)
    return out
