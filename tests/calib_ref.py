"""CPU reference of the view calibration (csrc/calib.hip, mqhip/calib.py): seeded chessboard and cage scenes, a NumPy
restatement of both projections and of the closed-form start, and the same least-squares problem handed to scipy
(least_squares, method='trf', x_scale='jac') on the same unknowns from the same start.

OpenCV is not installed, so nothing here is pinned to cv2 itself: the projections restate csrc/camera.hpp (which
restates OpenCV 4.11), the start restates csrc/calib_dev.hpp.  Derivatives for scipy are complex-step, exact to
rounding; the views are independent given the intrinsics, so 16 evaluations give the whole Jacobian.
"""
import numpy as np

MODEL_OMNIDIR, MODEL_PINHOLE = 0, 1
IMAGE_SIZE = (2048, 1536)
DEFAULT_FREE = {MODEL_PINHOLE: np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 0], dtype=bool),
                MODEL_OMNIDIR: np.array([1, 1, 0, 0, 0, 1, 1, 1, 1, 1], dtype=bool)}
LOOSE, TIGHT = 1e-8, 1e-15          # scipy's ftol = xtol = gtol of the two runs that make its band


def board_points(nx=9, ny=6, square=30.0):
    """The chessboard's inner corners, row by row, z = 0 (the reference's objp, 9 x 6, 30 mm)."""
    g = np.zeros((nx * ny, 3))
    g[:, :2] = np.mgrid[0:nx, 0:ny].T.reshape(-1, 2) * square
    return g


def rodrigues(rvecs):
    """(V, 3) -> (V, 3, 3); csrc/bundle_dev.hpp ba_rodrigues (real or complex)."""
    r = np.asarray(rvecs)
    th = np.sqrt(np.sum(r * r, axis=1))
    u = r / th[:, None]
    c, s = np.cos(th), np.sin(th)
    K = np.zeros(r.shape[:1] + (3, 3), dtype=r.dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -u[:, 2], u[:, 1], u[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -u[:, 0], -u[:, 1], u[:, 0]
    eye = np.eye(3)[None]
    return c[:, None, None] * eye + (1 - c)[:, None, None] * u[:, :, None] * u[:, None, :] + s[:, None, None] * K


def project(model, k, poses, obj):
    """k (10,), poses (V, 6), obj (V, n, 3) -> pixels (V, n, 2); camera.hpp's pinhole_project / omni_project."""
    poses = np.asarray(poses)
    R = rodrigues(poses[:, :3])
    Xc = np.einsum('vij,vnj->vni', R, obj) + poses[:, None, 3:]
    if model == MODEL_PINHOLE:
        fx, fy, cx, cy, k1, k2, p1, p2, k3 = k[:9]
        iz = 1.0 / Xc[..., 2]
        x, y = Xc[..., 0] * iz, Xc[..., 1] * iz
        r2 = x * x + y * y
        r4 = r2 * r2
        r6 = r4 * r2
        a1, a2, a3 = 2 * x * y, r2 + 2 * x * x, r2 + 2 * y * y
        cd = 1 + k1 * r2 + k2 * r4 + k3 * r6
        xd = x * cd + p1 * a1 + p2 * a2
        yd = y * cd + p1 * a3 + p2 * a1
        return np.stack([xd * fx + cx, yd * fy + cy], axis=-1)
    fx, fy, s, cx, cy, xi, k1, k2, p1, p2 = k
    nrm = np.sqrt(np.sum(Xc * Xc, axis=-1))
    xs, ys, zs = Xc[..., 0] / nrm, Xc[..., 1] / nrm, Xc[..., 2] / nrm
    xu, yu = xs / (zs + xi), ys / (zs + xi)
    r2 = xu * xu + yu * yu
    r4 = r2 * r2
    xd = xu * (1 + k1 * r2 + k2 * r4) + 2 * p1 * xu * yu + p2 * (r2 + 2 * xu * xu)
    yd = yu * (1 + k1 * r2 + k2 * r4) + p1 * (r2 + 2 * yu * yu) + 2 * p2 * xu * yu
    return np.stack([fx * xd + s * yd + cx, fy * yd + cy], axis=-1)


def project_views(model, k, poses, obj_list):
    """As ``project`` for views of different sizes: a list of (n, 2)."""
    return [project(model, k, np.asarray(poses)[v:v + 1], np.asarray(o)[None])[0] for v, o in enumerate(obj_list)]


def cost(model, k, poses, obj_list, img_list):
    return 0.5 * sum(float(np.sum((p - np.asarray(i)) ** 2))
                     for p, i in zip(project_views(model, k, poses, obj_list), img_list))


# ----------------------------------------------------------------------------- scenes
def true_intrinsics(model, xi=2.0):
    w, h = IMAGE_SIZE
    if model == MODEL_PINHOLE:
        return np.array([1810.0, 1795.0, 1040.0, 755.0, -0.12, 0.06, 0.0012, -0.0008, 0.02, 0.0])
    f = 1250.0 * (1.0 + xi)       # the centre is the fixed one: the omnidir fit does not move it
    return np.array([f, f * 0.995, 0.0, w / 2 - 0.5, h / 2 - 0.5, xi, -0.15, 0.04, 0.001, -0.0007])


def make_scene(model, V, seed, noise=0.3, xi=2.0, boards=None):
    """V views of the board: rvec ~ N(0, 0.35), t_z in [450, 900] mm, every corner inside the image (margin 8 px).
    ``boards``: per view (nx, ny), default the 9 x 6 board.  Returns a dict of arrays and lists."""
    rng = np.random.default_rng([seed, V, model, int(round(100 * xi))])
    k = true_intrinsics(model, xi)
    w, h = IMAGE_SIZE
    boards = boards or [(9, 6)] * V
    obj, img, poses = [], [], []
    for v in range(V):
        o = board_points(*boards[v])
        while True:
            rv = rng.normal(0.0, 0.35, 3)
            tz = rng.uniform(450.0, 900.0)
            t = np.array([rng.uniform(-0.5, 0.5) * tz - o[:, 0].mean(), rng.uniform(-0.4, 0.4) * tz - o[:, 1].mean(), tz])
            pose = np.concatenate([rv, t])
            uv = project(model, k, pose[None], o[None])[0]
            if uv[:, 0].min() > 8 and uv[:, 0].max() < w - 8 and uv[:, 1].min() > 8 and uv[:, 1].max() < h - 8:
                break
        obj.append(o)
        img.append(uv + noise * rng.normal(size=uv.shape))
        poses.append(pose)
    return {"model": model, "k_true": k, "poses_true": np.array(poses), "obj": obj, "img": img}


def make_cage_scene(kind, seed=0, noise=0.3):
    """A pose-only scene on a pinhole camera: 'cage10' 10 non-planar points, 'cage6' exactly 6, 'plane4' 4
    coplanar points on a plane that is not z = 0."""
    rng = np.random.default_rng([seed, {"cage10": 10, "cage6": 6, "plane4": 4}[kind]])
    k = true_intrinsics(MODEL_PINHOLE)
    if kind == "plane4":
        q = np.array([[0, 0, 0], [600, 0, 0], [600, 400, 0], [0, 400, 0.0]])
        Rp = rodrigues(np.array([[0.5, -0.4, 0.3]]))[0]
        o = q @ Rp.T + np.array([100.0, -50.0, 300.0])
    else:
        n = 10 if kind == "cage10" else 6
        corners = np.array([[x, y, z] for x in (0, 1200.0) for y in (0, 900.0) for z in (0, 800.0)])
        o = np.concatenate([corners, [[600, 450, 0], [600, 0, 400.0]]])[:n] if n == 10 else corners[[0, 1, 2, 4, 7, 5]]
        o = o + rng.normal(0, 5.0, o.shape)
    w, h = IMAGE_SIZE
    while True:
        rv = rng.normal(0.0, 0.5, 3)
        c = o.mean(axis=0)
        R = rodrigues(rv[None])[0]
        t = np.array([rng.uniform(-200, 200), rng.uniform(-150, 150), rng.uniform(2200, 3000)]) - R @ c
        pose = np.concatenate([rv, t])
        uv = project(MODEL_PINHOLE, k, pose[None], o[None])[0]
        if uv[:, 0].min() > 8 and uv[:, 0].max() < w - 8 and uv[:, 1].min() > 8 and uv[:, 1].max() < h - 8:
            break
    return {"model": MODEL_PINHOLE, "k_true": k, "poses_true": pose[None], "obj": [o],
            "img": [uv + noise * rng.normal(size=uv.shape)]}


# ----------------------------------------------------------------------------- the closed-form start
def _frame(o):
    c = o.mean(axis=0)
    ev, E = np.linalg.eigh((o - c).T @ (o - c))
    E = E[:, ::-1].copy()
    if np.linalg.det(E) < 0:
        E[:, 2] = -E[:, 2]
    return c, E, ev[::-1]


def homography(q, uv):
    """Hartley-normalised DLT from plane coordinates q (n, 2) to image points uv (n, 2)."""
    def norm(p):
        m = p.mean(axis=0)
        s = np.sqrt(2.0) / np.mean(np.linalg.norm(p - m, axis=1))
        return (p - m) * s, np.array([[s, 0, -s * m[0]], [0, s, -s * m[1]], [0, 0, 1.0]])
    qn, Tq = norm(q)
    un, Tu = norm(uv)
    X, Y, u, v = qn[:, 0], qn[:, 1], un[:, 0], un[:, 1]
    z, o = np.zeros_like(X), np.ones_like(X)
    A = np.concatenate([np.stack([-X, -Y, -o, z, z, z, u * X, u * Y, u], axis=1),
                        np.stack([z, z, z, -X, -Y, -o, v * X, v * Y, v], axis=1)])
    Hn = np.linalg.svd(A)[2][-1].reshape(3, 3)
    return np.linalg.inv(Tu) @ Hn @ Tq


def _polar(M):
    U, _, Vt = np.linalg.svd(M)
    return U @ Vt


def rvec_from_R(R):
    rx, ry, rz = R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]
    s = 0.5 * np.sqrt(rx * rx + ry * ry + rz * rz)
    c = np.clip(0.5 * (np.trace(R) - 1), -1, 1)
    th = np.arctan2(s, c)
    assert s > 1e-5, "the restatement covers generic rotations only"
    return np.array([rx, ry, rz]) * th / (2 * s)


def init_numpy(model, obj_list, img_list, image_size=IMAGE_SIZE):
    """calib_dev.hpp's start without given intrinsics: (k0 (10,), poses0 (V, 6)).  ValueError when Zhang's
    focal-length system is singular."""
    w, h = image_size
    cx, cy = 0.5 * (w - 1), 0.5 * (h - 1)
    frames, Hs = [], []
    N, b = np.zeros((2, 2)), np.zeros(2)
    for o, uv in zip(obj_list, img_list):
        o, uv = np.asarray(o, dtype=float), np.asarray(uv, dtype=float)
        c, E, ev = _frame(o)
        if not ev[2] < 1e-3 * ev[1]:
            raise ValueError("a view is not planar")
        H = homography((o - c) @ E[:, :2], uv)
        frames.append((c, E))
        Hs.append(H)
        S = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]]) @ H
        hv, vv = S[:, 0], S[:, 1]
        d1, d2 = (hv + vv) / 2, (hv - vv) / 2
        hv, vv, d1, d2 = (x / np.linalg.norm(x) for x in (hv, vv, d1, d2))
        A = np.array([[hv[0] * vv[0], hv[1] * vv[1]], [d1[0] * d2[0], d1[1] * d2[1]]])
        r = np.array([-hv[2] * vv[2], -d1[2] * d2[2]])
        N += A.T @ A
        b += A.T @ r
    if not np.linalg.det(N) > 1e-9 * np.trace(N) ** 2:
        raise ValueError("the focal-length system is singular")
    f = np.sqrt(np.abs(1.0 / np.linalg.solve(N, b)))
    if not (np.isfinite(f).all() and (f > 0).all()):
        raise ValueError("the focal-length system gives no finite length")
    poses = []
    Kinv = np.array([[1 / f[0], 0, -cx / f[0]], [0, 1 / f[1], -cy / f[1]], [0, 0, 1.0]])
    for (c, E), H in zip(frames, Hs):
        M = Kinv @ H
        sc = 1.0 / np.linalg.norm(M[:, 0])
        if M[2, 2] * sc < 0:
            sc = -sc
        r1, r2, tp = M[:, 0] * sc, M[:, 1] * sc, M[:, 2] * sc
        R = _polar(np.stack([r1, r2, np.cross(r1, r2)], axis=1)) @ E.T
        poses.append(np.concatenate([rvec_from_R(R), tp - R @ c]))
    if model == MODEL_PINHOLE:
        k0 = np.array([f[0], f[1], cx, cy, 0, 0, 0, 0, 0, 0.0])
    else:
        k0 = np.array([2 * f[0], 2 * f[1], 0, cx, cy, 1.0, 0, 0, 0, 0])
    return k0, np.array(poses)


# ----------------------------------------------------------------------------- scipy on the same unknowns
def _pad(obj_list, img_list):
    n = max(len(o) for o in obj_list)
    V = len(obj_list)
    obj, img, use = np.zeros((V, n, 3)), np.zeros((V, n, 2)), np.zeros((V, n), dtype=bool)
    for v, (o, i) in enumerate(zip(obj_list, img_list)):
        obj[v, :len(o)], img[v, :len(o)], use[v, :len(o)] = o, i, True
    obj[~use] = obj[:, :1].repeat(n, axis=1)[~use]     # padding repeats a real point; it is masked out below
    return obj, img, use


def solve_scipy(model, k0, poses0, obj_list, img_list, free_mask=None, tol=TIGHT, max_nfev=None, sparse=False):
    """least_squares(trf, x_scale='jac', ftol = xtol = gtol = tol) on [free slots, poses] from (k0, poses0).
    ``sparse`` hands scipy the Jacobian as a sparse matrix (its lsmr trust-region solver: for problems whose dense
    Jacobian is too large to factor).  Returns (k, poses, cost, result)."""
    from scipy.optimize import least_squares
    free = np.asarray(DEFAULT_FREE[model] if free_mask is None else free_mask, dtype=bool)
    fi = np.flatnonzero(free)
    nf, V = fi.size, len(obj_list)
    obj, img, use = _pad(obj_list, img_list)
    k0 = np.asarray(k0, dtype=float)

    def unpack(x):
        k = k0.astype(x.dtype)
        k[fi] = x[:nf]
        return k, x[nf:].reshape(V, 6)

    def fun(x):
        k, poses = unpack(x)
        return (project(model, k, poses, obj) - img)[use].ravel()

    vv, jj = np.nonzero(use)                    # residual pair p belongs to view vv[p]
    m = 2 * vv.size

    def jac(x):
        hstep = 1e-30
        Jk = np.zeros((m, nf))
        for c in range(nf):
            xc = x.astype(complex)
            xc[c] += 1j * hstep
            Jk[:, c] = fun(xc).imag / hstep
        rows, cols, vals = [], [], []
        for c in range(6):           # column c of every view at once: the views do not share poses
            xc = x.astype(complex)
            xc[nf + c::6] += 1j * hstep
            d = ((project(model, *unpack(xc), obj) - img).imag / hstep)[use]      # (pairs, 2)
            for e in range(2):
                rows.append(2 * np.arange(vv.size) + e)
                cols.append(nf + 6 * vv + c)
                vals.append(d[:, e])
        rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
        if sparse:
            from scipy.sparse import coo_matrix, csr_matrix, hstack
            return hstack([csr_matrix(Jk), coo_matrix((vals, (rows, cols - nf)), shape=(m, 6 * V))]).tocsr()
        J = np.zeros((m, x.size))
        J[:, :nf] = Jk
        J[rows, cols] = vals
        return J

    x0 = np.concatenate([k0[fi], np.asarray(poses0, dtype=float).ravel()])
    res = least_squares(fun, x0, jac=jac, method='trf', x_scale='jac', ftol=tol, xtol=tol, gtol=tol,
                        max_nfev=max_nfev)
    k, poses = unpack(res.x)
    return k, poses.copy(), float(res.cost), res


def rotation_distance(ra, rb):
    """max |R(ra) - R(rb)| per view: the rotation angle between them to first order."""
    return np.abs(rodrigues(np.atleast_2d(ra)) - rodrigues(np.atleast_2d(rb))).max(axis=(1, 2))


# ----------------------------------------------------------------------------- the named scenes of the golden file
# name -> (kind, model, V, seed, noise, xi, boards)
SCENES = {f"pin_V{V}_s{s}": ("board", MODEL_PINHOLE, V, s, 0.3, 2.0, None) for V in (3, 5, 20) for s in (0, 1)}
SCENES.update({f"omni_xi{xi}": ("board", MODEL_OMNIDIR, 20, 0, 0.3, xi, None) for xi in (0.84, 2.0, 4.43)})
SCENES["omni_clean"] = ("board", MODEL_OMNIDIR, 20, 0, 0.0, 2.0, None)
# one 13 x 5 board (65 points: two passes of a 64-lane wave) next to 54-point views
SCENES["pin_mixed"] = ("board", MODEL_PINHOLE, 4, 0, 0.3, 2.0, [(13, 5), (9, 6), (9, 6), (9, 6)])
SCENES.update({kind: ("cage", MODEL_PINHOLE, 1, 0, 0.3, 2.0, None) for kind in ("cage10", "cage6", "plane4")})
SCENES["board_pose1"] = ("pose", MODEL_PINHOLE, 1, 0, 0.3, 2.0, None)      # one board view, pose only
GOLDEN = "calib_scenes.npz"


def scene(name):
    kind, model, V, seed, noise, xi, boards = SCENES[name]
    if kind == "cage":
        return make_cage_scene(name, seed, noise)
    return make_scene(model, V, seed, noise, xi, boards)


def scene_start(name, sc):
    """(k0, poses0, free_mask) scipy and the library start from: the closed-form start of a board scene; the true
    intrinsics (frozen) and the true pose for a pose-only scene, whose minimum is next to it."""
    if SCENES[name][0] in ("cage", "pose"):
        return sc["k_true"].copy(), sc["poses_true"].copy(), np.zeros(10, dtype=bool)
    k0, p0 = init_numpy(sc["model"], sc["obj"], sc["img"])
    return k0, p0, DEFAULT_FREE[sc["model"]]


def load_golden(path):
    """{name: dict} with obj / img split back into per-view lists."""
    out = {}
    with np.load(path) as z:
        for name in SCENES:
            d = {key.split("/", 1)[1]: z[key] for key in z.files if key.startswith(name + "/")}
            cuts = np.cumsum(d["counts"])[:-1]
            d["obj"], d["img"] = np.split(d["obj"], cuts), np.split(d["img"], cuts)
            d["model"] = int(d["model"])
            out[name] = d
    return out


# ----------------------------------------------------------------------------- the calibration chain
CHAIN_IDS = [11, 12, 13, 14]
CAGE = np.array([[x, y, z] for x in (0, 1200.0) for y in (0, 900.0) for z in (0, 800.0)] +
                [[600, 450, 0], [600, 0, 400.0]])          # 10 annotated cage points, mm


def _look_at(pos, target):
    z = (target - pos) / np.linalg.norm(target - pos)
    x = np.cross([0, 0, 1.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])               # world -> camera
    return np.concatenate([rvec_from_R(R), -R @ pos])


def make_chain_scene(seed=0, noise=0.3):
    """4 omnidir cameras (xi = 2) around the cage: 8 chessboard views each, the 10 cage points as annotation rows
    (flag, u, v on the 640-wide preview, X, Y, Z), a 45-row marker trace (40 frames are used, x < 0 = not seen) and
    20 held-out marker positions with their noise-free pixels."""
    rng = np.random.default_rng([seed, 4])
    k = true_intrinsics(MODEL_OMNIDIR, 2.0)
    centre = np.array([600.0, 450.0, 400.0])
    ext = np.array([_look_at(centre + 2600.0 * np.array([np.cos(a), np.sin(a), h]), centre)
                    for a, h in ((0.3, 0.35), (1.9, 0.25), (3.4, 0.4), (5.0, 0.3))])
    boards = [make_scene(MODEL_OMNIDIR, 8, 100 + c, noise) for c in range(4)]
    cage = []
    for c in range(4):
        uv = project(MODEL_OMNIDIR, k, ext[c:c + 1], CAGE[None])[0] + noise * rng.normal(size=(10, 2))
        cage.append(np.concatenate([np.ones((10, 1)), uv * 640 / 2048, CAGE], axis=1))
    X = centre + rng.uniform(-1, 1, (45, 3)) * [500, 380, 330]
    trace = []
    for c in range(4):
        uv = project(MODEL_OMNIDIR, k, ext[c:c + 1], X[None])[0] + noise * rng.normal(size=(45, 2))
        uv[rng.uniform(size=45) < 0.15] = -1.0
        trace.append(uv)
    held = centre + rng.uniform(-1, 1, (20, 3)) * [500, 380, 330]
    held_uv = np.stack([project(MODEL_OMNIDIR, k, ext[c:c + 1], held[None])[0] for c in range(4)])
    return {"k_true": k, "ext_true": ext, "boards": boards, "cage": cage, "trace": trace, "held": held,
            "held_uv": held_uv}


def chain_scipy(sc, tol):
    """scipy's side of the chain: per camera the pinhole and the omnidir fit from the closed-form start, then the
    pose-only fit of the cage points through the fitted pinhole camera (from the true pose: its minimum is next to
    it).  Returns (k_pinhole (4, 10), k_omnidir (4, 10), extrinsics (4, 6))."""
    kp, ko, ext = [], [], []
    for c, b in enumerate(sc["boards"]):
        k0, p0 = init_numpy(MODEL_PINHOLE, b["obj"], b["img"])
        kp.append(solve_scipy(MODEL_PINHOLE, k0, p0, b["obj"], b["img"], tol=tol)[0])
        k0, p0 = init_numpy(MODEL_OMNIDIR, b["obj"], b["img"])
        ko.append(solve_scipy(MODEL_OMNIDIR, k0, p0, b["obj"], b["img"], tol=tol)[0])
        rows = sc["cage"][c]
        ext.append(solve_scipy(MODEL_PINHOLE, kp[-1], sc["ext_true"][c:c + 1], [rows[:, 3:]], [rows[:, 1:3] * 2048 / 640],
                               free_mask=np.zeros(10), tol=tol)[1][0])
    return np.array(kp), np.array(ko), np.array(ext)


def load_chain(path):
    sc = make_chain_scene()
    with np.load(path) as z:
        for tag in ("loose", "tight"):
            sc[tag] = tuple(z[f"chain/{key}_{tag}"] for key in ("k_pinhole", "k_omnidir", "ext"))
        sc["check"] = {key: z[f"chain/{key}"] for key in ("trace", "cage", "board_img")}
    return sc
