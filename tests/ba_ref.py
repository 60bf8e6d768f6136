"""CPU reference of the rig bundle adjustment (mqhip.bundle / csrc/bundle.hip): our restatement of what
multicam_toolbox.optimize_extrinsic (:523-612, mode 0) and optimize_all_camera_params (:696-777, mode 1) hand
to scipy -- the residual function, the Jacobian sparsity and the least_squares call with the reference's
arguments -- plus a synthetic scene builder and a gauge-invariant comparison.

Mode 1's projection is the vectorised numpy omnidir formula (mqhip.synth.project_numpy's, with per-row
parameters); the reference calls cv2.omnidir.projectPoints once per observation, which is the same map.
"""
import numpy as np
from scipy.optimize import least_squares
from scipy.sparse import lil_matrix

from mqhip import synth

N_PARAMS = {0: 6, 1: 16}


# ----------------------------------------------------------------------------- the reference's pieces
def rotate(points, rot_vecs):
    """Rodrigues' formula per row, with the reference's 0 / 0 -> 0 rule at a zero vector (:551-564)."""
    theta = np.linalg.norm(rot_vecs, axis=1)[:, np.newaxis]
    with np.errstate(invalid='ignore', divide='ignore'):
        v = np.nan_to_num(rot_vecs / theta)
    dot = np.sum(points * v, axis=1)[:, np.newaxis]
    c, s = np.cos(theta), np.sin(theta)
    return c * points + s * np.cross(v, points) + dot * (1 - c) * v


def project(mode, points, cam_rows):
    """One projection per row: points (M, 3), cam_rows (M, P)."""
    pc = rotate(points, cam_rows[:, :3]) + cam_rows[:, 3:6]
    if mode == 0:
        return pc[:, :2] / pc[:, 2, np.newaxis]
    xs = pc / np.sqrt(np.sum(pc * pc, axis=1))[:, np.newaxis]
    xi = cam_rows[:, 11]
    xu, yu = xs[:, 0] / (xs[:, 2] + xi), xs[:, 1] / (xs[:, 2] + xi)
    k1, k2, p1, p2 = cam_rows[:, 12], cam_rows[:, 13], cam_rows[:, 14], cam_rows[:, 15]
    r2 = xu * xu + yu * yu
    r4 = r2 * r2
    rad = 1 + k1 * r2 + k2 * r4
    xd = xu * rad + 2 * p1 * xu * yu + p2 * (r2 + 2 * xu * xu)
    yd = yu * rad + p1 * (r2 + 2 * yu * yu) + 2 * p2 * xu * yu
    u = cam_rows[:, 6] * xd + cam_rows[:, 7] * yd + cam_rows[:, 8]
    v = cam_rows[:, 9] * yd + cam_rows[:, 10]
    return np.stack([u, v], axis=1)


def observation_lists(obs, use):
    """The reference's camera-major lists (:530-543): camera_indices, point_indices, points_2d."""
    use = np.asarray(use, dtype=bool)
    cam_idx, pt_idx, p2 = [], [], []
    for c in range(use.shape[1]):
        for i in range(use.shape[0]):
            if use[i, c]:
                cam_idx.append(c)
                pt_idx.append(i)
                p2.append(obs[c][i, :])
    return np.array(cam_idx), np.array(pt_idx), np.vstack(p2)


def make_fun(mode, cam0, fix_cam0):
    P = N_PARAMS[mode]
    cam0 = np.array(cam0, dtype=np.float64)

    def fun(params, n_cameras, n_points, camera_indices, point_indices, points_2d):
        cp = params[:n_cameras * P].reshape((n_cameras, P))
        if fix_cam0:
            cp[0, :6] = cam0[0, :6]       # written into params, as the reference does (:585-586, :746-747)
        p3 = params[n_cameras * P:].reshape((n_points, 3))
        return (project(mode, p3[point_indices], cp[camera_indices]) - points_2d).ravel()

    return fun


def bundle_adjustment_sparsity(P, n_cameras, n_points, camera_indices, point_indices):
    m = camera_indices.size * 2
    A = lil_matrix((m, n_cameras * P + n_points * 3), dtype=int)
    i = np.arange(camera_indices.size)
    for s in range(P):
        A[2 * i, camera_indices * P + s] = 1
        A[2 * i + 1, camera_indices * P + s] = 1
    for s in range(3):
        A[2 * i, n_cameras * P + point_indices * 3 + s] = 1
        A[2 * i + 1, n_cameras * P + point_indices * 3 + s] = 1
    return A


def residuals(mode, cam, pts, obs, use):
    ci, pi, p2 = observation_lists(obs, use)
    return (project(mode, np.asarray(pts)[pi], np.asarray(cam)[ci]) - p2).ravel()


def cost(mode, cam, pts, obs, use):
    r = residuals(mode, cam, pts, obs, use)
    return 0.5 * float(r @ r)


def solve_scipy(mode, cam, pts, obs, use, fix_cam0=True, ftol=None, max_nfev=None):
    """The reference's call: least_squares(fun, x0, jac_sparsity=A, x_scale='jac', ftol=1e-5 (:611) or the
    argument's 1e-3 default with loss='linear' and max_nfev (:776), method='trf').  Returns (cam, pts, result)."""
    P = N_PARAMS[mode]
    cam = np.array(cam, dtype=np.float64)
    pts = np.array(pts, dtype=np.float64)
    if ftol is None:
        ftol = 1e-5 if mode == 0 else 1e-3
    ci, pi, p2 = observation_lists(obs, use)
    C, N = cam.shape[0], pts.shape[0]
    x0 = np.hstack((cam.ravel(), pts.ravel()))
    A = bundle_adjustment_sparsity(P, C, N, ci, pi)
    kw = dict(loss='linear', max_nfev=max_nfev) if mode == 1 else {}
    res = least_squares(make_fun(mode, cam, fix_cam0), x0, jac_sparsity=A, verbose=0, x_scale='jac', ftol=ftol,
                        method='trf', args=(C, N, ci, pi, p2), **kw)
    return res.x[:C * P].reshape(C, P).copy(), res.x[C * P:].reshape(N, 3).copy(), res


# ----------------------------------------------------------------------------- scenes
def cam_rows(cams, mode):
    """(C, P) rows in the reference's order: rvec, tvec [, K00, K01, K02, K11, K12, xi, D[4]] (:692-694)."""
    out = np.zeros((len(cams), N_PARAMS[mode]))
    for i, c in enumerate(cams):
        out[i, :3] = np.ravel(c["rvec"])
        out[i, 3:6] = np.ravel(c["tvec"])
        if mode == 1:
            K = np.asarray(c["K"])
            out[i, 6:11] = [K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]]
            out[i, 11] = float(np.ravel(c["xi"])[0])
            out[i, 12:16] = np.ravel(c["D"])[:4]
    return out


def make_scene(C, N, seed=0, mode=0, noise=None, drop=0.15):
    """N points uniform in +-600 x +-600 x +-300 mm seen by synth.make_cameras(C); ``drop`` of the observations
    removed, every point keeping at least 2 cameras; noise 5e-4 (normalised units, mode 0) or 0.5 px (mode 1);
    start = truth with cameras 1.. moved by N(0, 0.01) rad and N(0, 10) mm and the points by N(0, 15) mm."""
    rng = np.random.default_rng(seed)
    truth = cam_rows(synth.make_cameras(C), mode)
    pts = rng.uniform(-1.0, 1.0, (N, 3)) * np.array([600.0, 600.0, 300.0])
    use = rng.uniform(size=(N, C)) >= drop
    for i in range(N):
        while use[i].sum() < 2:
            use[i, rng.integers(C)] = True
    if noise is None:
        noise = 5e-4 if mode == 0 else 0.5
    obs = np.zeros((C, N, 2))
    for c in range(C):
        obs[c] = project(mode, pts, np.repeat(truth[c][None], N, axis=0))
    obs += rng.normal(0.0, 1.0, obs.shape) * noise
    cam_start = truth.copy()
    cam_start[1:, :3] += rng.normal(0.0, 0.01, (C - 1, 3))
    cam_start[1:, 3:6] += rng.normal(0.0, 10.0, (C - 1, 3))
    pts_start = pts + rng.normal(0.0, 15.0, (N, 3))
    return dict(mode=mode, C=C, N=N, cam_true=truth, pts_true=pts, cam=cam_start, pts=pts_start, obs=obs, use=use)


# ----------------------------------------------------------------------------- gauge-invariant comparison
def gauge_invariants(cam):
    """Relative rotations R_c R_0^T (C, 3, 3) and baselines (centre_c - centre_0) / |centre_1 - centre_0| (C, 3):
    what a similarity of the world frame leaves alone (with camera 0 fixed the scale is still free, so raw tvec
    and points are not comparable between two solvers)."""
    cam = np.asarray(cam, dtype=np.float64)
    R = np.stack([synth.rodrigues_to_mat(c[:3]) for c in cam])
    centre = np.stack([-R[i].T @ cam[i, 3:6] for i in range(len(cam))])
    rel = np.stack([R[i] @ R[0].T for i in range(len(cam))])
    base = (centre - centre[0]) @ R[0].T            # in camera 0's axes
    return rel, base / np.linalg.norm(base[1])


def gauge_distance(cam_a, cam_b):
    """(largest rotation-matrix entry difference, largest baseline entry difference)."""
    ra, ba = gauge_invariants(cam_a)
    rb, bb = gauge_invariants(cam_b)
    return float(np.abs(ra - rb).max()), float(np.abs(ba - bb).max())
