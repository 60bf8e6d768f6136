"""CPU reference of ``CameraGroup.bundle_adjust`` / ``bundle_adjust_iter`` (mqhip.geometry, csrc/bundle.hip mode 2):
our restatement of what aniposelib's cameras.py hands to scipy -- ``_error_fun_bundle`` (:949-980),
``_jac_sparsity_bundle`` (:983-1057) and ``_initialize_params_bundle`` (:1059-1117) with ``extra=None``, the
``least_squares`` call with the reference's arguments (:926-937) and the loop of ``bundle_adjust_iter`` (:806-892)
with its helpers (:35-127) -- plus a scene builder in the style of ``ba_ref.make_scene``.  The gauge-invariant
comparison is ``ba_ref``'s.

A camera is a row: ``models`` (C,) with camera.hpp's ids, ``params`` (C, 9) [rvec, tvec, f, k1, k2] and ``fixed``
(C, 11) [model, cx, cy, ...] or [model, K00, K01, K02, K11, K12, xi, D[4]] (include/mq_hip.h).  The error function
projects with the model ``set_params`` leaves: fx = fy = f and every distortion but k1(, k2) zero; an omnidir camera
projects with its K, xi, D, which ``set_params`` does not touch.
"""
import numpy as np
from scipy.optimize import least_squares
from scipy.sparse import dok_matrix

import ba_ref
from ba_ref import gauge_distance  # noqa: F401  (the comparison is ba_ref's)
from mqhip import synth

OMNIDIR, PINHOLE, FISHEYE = 0, 1, 2
MODEL_IDS = {"omnidir": OMNIDIR, "pinhole": PINHOLE, "fisheye": FISHEYE}


# ----------------------------------------------------------------------------- the three reduced projections
def project(models, fixed, params, points):
    """One projection per row: models (M,), fixed (M, 11), params (M, 9), points (M, 3) -> (M, 2)."""
    pc = ba_ref.rotate(points, params[:, :3]) + params[:, 3:6]
    out = np.empty((len(points), 2))
    o = models == OMNIDIR
    if o.any():
        g = fixed[o, 1:]
        xs = pc[o] / np.sqrt(np.sum(pc[o] * pc[o], axis=1))[:, np.newaxis]
        xi = g[:, 5]
        xu, yu = xs[:, 0] / (xs[:, 2] + xi), xs[:, 1] / (xs[:, 2] + xi)
        k1, k2, p1, p2 = g[:, 6], g[:, 7], g[:, 8], g[:, 9]
        r2 = xu * xu + yu * yu
        r4 = r2 * r2
        rad = 1 + k1 * r2 + k2 * r4
        xd = xu * rad + 2 * p1 * xu * yu + p2 * (r2 + 2 * xu * xu)
        yd = yu * rad + p1 * (r2 + 2 * yu * yu) + 2 * p2 * xu * yu
        out[o, 0] = g[:, 0] * xd + g[:, 1] * yd + g[:, 2]
        out[o, 1] = g[:, 3] * yd + g[:, 4]
    for model in (PINHOLE, FISHEYE):
        m = models == model
        if not m.any():
            continue
        x, y = pc[m, 0] / pc[m, 2], pc[m, 1] / pc[m, 2]
        f, k1, k2 = params[m, 6], params[m, 7], params[m, 8]
        cx, cy = fixed[m, 1], fixed[m, 2]
        r2 = x * x + y * y
        if model == PINHOLE:
            cdist = 1 + k1 * r2 + k2 * (r2 * r2)
        else:
            r = np.sqrt(r2)
            th = np.arctan(r)
            th2 = th * th
            th3, th4 = th2 * th, th2 * th2
            theta_d = th + k1 * th3 + k2 * (th4 * th)
            with np.errstate(divide='ignore', invalid='ignore'):
                cdist = np.where(r > 1e-8, theta_d * (1.0 / r), 1.0)
        out[m, 0] = (x * cdist) * f + cx
        out[m, 1] = (y * cdist) * f + cy
    return out


def project_all(models, fixed, params, points):
    """Every camera on every point: (C, N, 2)."""
    N = len(points)
    return np.stack([project(np.full(N, models[c]), np.repeat(fixed[c][None], N, 0), np.repeat(params[c][None], N, 0),
                             points) for c in range(len(models))])


# ----------------------------------------------------------------------------- the reference's pieces
class RefGroup:
    """The state the reference's CameraGroup carries through a bundle adjustment, as arrays."""

    def __init__(self, models, fixed, params, extra_dist=False):
        self.models = np.array(models)
        self.fixed = np.array(fixed, dtype=np.float64)
        self.params = np.array(params, dtype=np.float64)       # (C, 9); slot 8 is read only with extra_dist
        self.extra_dist = bool(extra_dist)
        self.n_cam_params = 8 + self.extra_dist

    def get_params(self):
        return self.params[:, :self.n_cam_params].ravel().copy()

    def set_params(self, flat):
        """Camera.set_params per camera: k2 = 0 without extra_dist (the distortions are rebuilt from zeros)."""
        self.params[:, 8] = 0.0
        self.params[:, :self.n_cam_params] = np.asarray(flat).reshape(len(self.models), self.n_cam_params)

    def reprojection_error(self, p3ds, p2ds):
        """p2d - projection, NaN where the point is not seen (cameras.py:746-783)."""
        return p2ds - project_all(self.models, self.fixed, self.params, p3ds)

    def error_fun(self, x, p2ds):
        good = ~np.isnan(p2ds)
        sub = self.n_cam_params * len(self.models)
        self.set_params(x[:sub])
        p3ds = x[sub:sub + p2ds.shape[1] * 3].reshape(-1, 3)
        return self.reprojection_error(p3ds, p2ds)[good]

    def jac_sparsity(self, p2ds):
        C, N, _ = p2ds.shape
        P = self.n_cam_params
        good = ~np.isnan(p2ds)
        cam_ix = np.broadcast_to(np.arange(C)[:, None, None], p2ds.shape)[good]
        pt_ix = np.broadcast_to(np.arange(N)[None, :, None], p2ds.shape)[good]
        A = dok_matrix((int(good.sum()), C * P + N * 3), dtype='int16')
        ix = np.arange(int(good.sum()))
        for i in range(P):
            A[ix, cam_ix * P + i] = 1
        for i in range(3):
            A[ix, C * P + pt_ix * 3 + i] = 1
        return A

    def bundle_adjust(self, p2ds, p3ds0=None, start_params=None, ftol=1e-4, max_nfev=1000, threshold=50,
                      loss='linear'):
        """The reference's call.  x0 = every camera's get_params, then the triangulated points ``p3ds0``;
        ``start_params`` replaces it.  Returns scipy's result; the cameras are left at the optimum."""
        x0 = start_params if start_params is not None else np.hstack([self.get_params(), np.ravel(p3ds0)])
        res = least_squares(self.error_fun, np.array(x0, dtype=np.float64), jac_sparsity=self.jac_sparsity(p2ds),
                            f_scale=threshold, x_scale='jac', loss=loss, ftol=ftol, method='trf',
                            tr_solver='lsmr', verbose=0, max_nfev=max_nfev, args=(p2ds,))
        self.set_params(res.x[:self.n_cam_params * len(self.models)])
        return res


def get_error_dict(errors_full, min_points=10):
    n_cams = errors_full.shape[0]
    errors_norm = np.linalg.norm(errors_full, axis=2)
    good = ~np.isnan(errors_full[:, :, 0])
    out = {}
    for i in range(n_cams):
        for j in range(i + 1, n_cams):
            both = good[i] & good[j]
            pair_mean = np.mean(errors_norm[:, both][[i, j]], axis=0)
            if np.sum(both) > min_points:
                out[(i, j)] = (int(both.sum()), np.percentile(pair_mean, [15, 75]))
    return out


def resample_points(imgp, n_samp=25):
    n_cams = imgp.shape[0]
    good = ~np.isnan(imgp[:, :, 0])
    ixs = np.arange(imgp.shape[1])
    num_cams = np.sum(good, axis=0)
    include = set()
    for i in range(n_cams):
        for j in range(i + 1, n_cams):
            both = good[i] & good[j]
            if np.sum(both) > 0:
                arr = num_cams[both].astype('float64')
                arr += np.random.random(size=arr.shape)
                include.update(ixs[both][np.argsort(-arr)[:n_samp]])
    return imgp[:, sorted(include)]


def _mu_terms(errors_full):
    max_error = min_error = 0
    for _, percents in get_error_dict(errors_full).values():
        max_error = max(percents[-1], max_error)
        min_error = max(percents[0], min_error)
    return max_error, min_error


def bundle_adjust_iter(ref, backend, p2ds_full, n_iters=10, start_mu=15, end_mu=1, max_nfev=200, ftol=1e-4,
                       n_samp_iter=100, n_samp_full=1000, error_threshold=0.3):
    """The loop of cameras.py:806-892 around ``ref.bundle_adjust`` (scipy).  ``backend`` supplies what the
    reference takes from its own cameras: ``triangulate(p2ds)``, ``reprojection_error(p3ds, p2ds, mean)`` and
    ``set_params(rows)``, called with ``ref``'s (C, n_cam_params) rows after every solve.  Returns
    (median error, number of solves)."""
    def average_error(p2ds):
        return np.median(backend.reprojection_error(backend.triangulate(p2ds), p2ds, mean=True))

    def solve(p2ds, nfev):
        ref.bundle_adjust(p2ds, backend.triangulate(p2ds), ftol=ftol, max_nfev=nfev)
        backend.set_params(ref.params[:, :ref.n_cam_params])

    solves = 0
    p2ds = resample_points(p2ds_full, n_samp_full)
    average_error(p2ds)
    mus = np.exp(np.linspace(np.log(start_mu), np.log(end_mu), num=n_iters))
    for i in range(n_iters):
        p2ds = resample_points(p2ds_full, n_samp_full)
        p3ds = backend.triangulate(p2ds)
        errors_full = backend.reprojection_error(p3ds, p2ds, mean=False)
        errors_norm = backend.reprojection_error(p3ds, p2ds, mean=True)
        max_error, min_error = _mu_terms(errors_full)
        mu = max(min(max_error, mus[i]), min_error)
        good = errors_norm < mu
        p2ds_samp = resample_points(p2ds[:, good], n_samp_iter)
        if np.median(errors_norm) < error_threshold:
            break
        solve(p2ds_samp, max_nfev)
        solves += 1
    p2ds = resample_points(p2ds_full, n_samp_full)
    p3ds = backend.triangulate(p2ds)
    errors_full = backend.reprojection_error(p3ds, p2ds, mean=False)
    errors_norm = backend.reprojection_error(p3ds, p2ds, mean=True)
    max_error, min_error = _mu_terms(errors_full)
    mu = max(max(max_error, end_mu), min_error)
    solve(p2ds[:, errors_norm < mu], max(200, max_nfev))
    return average_error(p2ds), solves + 1


# ----------------------------------------------------------------------------- scenes
def make_scene(models, N, seed=0, extra_dist=False, noise=0.5, drop=0.15, outliers=0.0, min_cams=2):
    """N points uniform in +-600 x +-600 x +-300 mm seen by cameras on synth.make_cameras' extrinsics, one model
    name per camera ('pinhole', 'fisheye', 'omnidir'); the true cameras are reduced models (fx = fy = f, k1 and,
    with ``extra_dist``, k2).  ``drop`` of the observations removed (NaN), every point keeping ``min_cams``
    cameras; ``noise`` px; a share ``outliers`` of the observations moved by 50-200 px.  Start = truth with cameras
    1.. moved by N(0, 0.01) rad and N(0, 10) mm (section 8.6) and the points by N(0, 15) mm."""
    rng = np.random.default_rng(seed)
    C = len(models)
    base = synth.make_cameras(C)
    ids = np.array([MODEL_IDS[m] for m in models])
    fixed = np.zeros((C, 11))
    params = np.zeros((C, 9))
    for c, cam in enumerate(base):
        params[c, :3], params[c, 3:6] = np.ravel(cam["rvec"]), np.ravel(cam["tvec"])
        fixed[c, 0] = ids[c]
        if ids[c] == OMNIDIR:
            K = np.asarray(cam["K"])
            fixed[c, 1:7] = [K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2], float(np.ravel(cam["xi"])[0])]
            fixed[c, 7:11] = np.ravel(cam["D"])[:4]
            # what get_params reads from an omnidir camera's matrix and distortions: carried, never used
            params[c, 6] = cam["matrix"][0, 0]
        else:
            m = np.asarray(cam["matrix"])
            fixed[c, 1:3] = [m[0, 2], m[1, 2]]
            scale = (0.05, 0.02) if ids[c] == PINHOLE else (0.02, 0.005)
            k = rng.normal(0.0, 1.0, 2) * scale
            params[c, 6:9] = [m[0, 0], k[0], k[1] if extra_dist else 0.0]
    pts = rng.uniform(-1.0, 1.0, (N, 3)) * np.array([600.0, 600.0, 300.0])
    use = rng.uniform(size=(N, C)) >= drop
    for i in range(N):
        while use[i].sum() < min(min_cams, C):
            use[i, rng.integers(C)] = True
    p2ds = project_all(ids, fixed, params, pts) + rng.normal(0.0, 1.0, (C, N, 2)) * noise
    if outliers:
        bad = (rng.uniform(size=(C, N)) < outliers) & use.T
        ang = rng.uniform(0, 2 * np.pi, (C, N))
        p2ds += (bad * rng.uniform(50.0, 200.0, (C, N)))[:, :, None] * np.stack([np.cos(ang), np.sin(ang)], axis=2)
    p2ds[~use.T] = np.nan
    start = params.copy()
    start[1:, :3] += rng.normal(0.0, 0.01, (C - 1, 3))
    start[1:, 3:6] += rng.normal(0.0, 10.0, (C - 1, 3))
    pts_start = pts + rng.normal(0.0, 15.0, (N, 3))
    return dict(models=ids, names=list(models), C=C, N=N, extra_dist=bool(extra_dist), fixed=fixed,
                params_true=params, pts_true=pts, params=start, pts=pts_start, p2ds=p2ds, use=use)


def ref_group(sc):
    return RefGroup(sc["models"], sc["fixed"], sc["params"], sc["extra_dist"])


def start_params(sc):
    """x0 of the reference's layout: every camera's 8 (9) parameters, then the points."""
    P = 8 + sc["extra_dist"]
    return np.hstack([sc["params"][:, :P].ravel(), sc["pts"].ravel()])


def cost(sc, params, pts):
    r = RefGroup(sc["models"], sc["fixed"], params, sc["extra_dist"]).reprojection_error(pts, sc["p2ds"])
    r = r[~np.isnan(sc["p2ds"])]
    return 0.5 * float(r @ r)


def camera_group(sc, params=None):
    """The scene's cameras as an mqhip CameraGroup (host objects; no GPU call is made here)."""
    from mqhip.geometry import Camera, CameraGroup, FisheyeCamera, OmnidirCamera
    params = sc["params"] if params is None else params
    cams = []
    for c in range(sc["C"]):
        p, g = params[c], sc["fixed"][c]
        kw = dict(rvec=p[:3], tvec=p[3:6], name=str(c), size=[2048, 1536], extra_dist=sc["extra_dist"])
        if sc["models"][c] == OMNIDIR:
            K = np.array([[g[1], g[2], g[3]], [0.0, g[4], g[5]], [0.0, 0.0, 1.0]])
            m = np.array([[p[6], 0.0, g[3]], [0.0, p[6], g[5]], [0.0, 0.0, 1.0]])
            cams.append(OmnidirCamera(matrix=m, dist=np.zeros(4), xi=[g[6]], K=K, D=g[7:11], **kw))
        else:
            m = np.array([[p[6], 0.0, g[1]], [0.0, p[6], g[2]], [0.0, 0.0, 1.0]])
            if sc["models"][c] == PINHOLE:
                cams.append(Camera(matrix=m, dist=[p[7], p[8], 0.0, 0.0, 0.0], **kw))
            else:
                cams.append(FisheyeCamera(matrix=m, dist=[p[7], p[8], 0.0, 0.0], **kw))
    return CameraGroup(cams)


def group_params(group):
    """(C, 9) rows of a CameraGroup: get_params per camera, k2 = 0 where it is not a parameter."""
    out = np.zeros((len(group.cameras), 9))
    for c, cam in enumerate(group.cameras):
        p = cam.get_params()
        out[c, :p.size] = p
    return out
