"""NumPy restatement of the chessboard-corner detector (csrc/chessboard.hip, csrc/chessboard_dev.hpp; DESIGN.md
section 8.14), stage by stage, and a renderer of chessboard views with analytic corner positions.

Stages 2-5 are integer arithmetic (Python ints where a product could leave int64's comfortable range), so the
kernels equal them exactly.  Stage 6 is float64 with sums in index order; the kernel adds in another order."""
import functools
import math

import numpy as np

PATTERN = (9, 6)
N_CORNERS = 54
MAX_SEEDS = 54
MAX_PASSES = 55
GRID_OFF = 10   # cells live in [-GRID_OFF, GRID_OFF]^2 around the seed; a placement outside is refused
NMS_R = 4       # 9 x 9 neighbourhood
BORDER = 5

RING = ((5, 0), (5, 2), (4, 4), (2, 5), (0, 5), (-2, 5), (-4, 4), (-5, 2), (-5, 0), (-5, -2), (-4, -4), (-2, -5),
        (0, -5), (2, -5), (4, -4), (5, -2))


def default_scale(width):
    return 0.5 if width > 1024 else 1.0


# ----------------------------------------------------------------------------- 2. response
def blur3(gray):
    g = np.pad(np.asarray(gray).astype(np.int32), 1, mode="edge")
    h = g[:, :-2] + 2 * g[:, 1:-1] + g[:, 2:]
    return (h[:-2] + 2 * h[1:-1] + h[2:] + 8) >> 4


def chess_response(gray):
    """uint8 (h, w) -> int32 (h, w): ChESS on the 3 x 3 binomial blur, 0 in the 5-pixel border."""
    b = blur3(gray)
    h, w = b.shape
    out = np.zeros((h, w), np.int32)
    if h <= 2 * BORDER or w <= 2 * BORDER:
        return out
    ys, xs = slice(BORDER, h - BORDER), slice(BORDER, w - BORDER)

    def sh(dx, dy):
        return b[BORDER + dy:h - BORDER + dy, BORDER + dx:w - BORDER + dx]

    I = [sh(dx, dy) for dx, dy in RING]
    SR = sum(np.abs(I[k] + I[k + 8] - I[k + 4] - I[k + 12]) for k in range(4))
    DR = sum(np.abs(I[k] - I[k + 8]) for k in range(8))
    S = sum(I)
    L = sh(0, 0) + sh(1, 0) + sh(-1, 0) + sh(0, 1) + sh(0, -1)
    out[ys, xs] = np.maximum(0, 5 * SR - 5 * DR - np.abs(5 * S - 16 * L))
    return out


# ----------------------------------------------------------------------------- 3. candidates
def chess_candidates(resp, K=256):
    """int32 (h, w) -> pos (K, 2) int32 [x, y], resp (K,) int32, count.  R > 0 and R == max over 9 x 9 (clipped at
    the image); the first K under (R descending, y ascending, x ascending); rows past count are zero."""
    r = np.asarray(resp, np.int64)
    h, w = r.shape
    p = np.pad(r, NMS_R, mode="constant")
    m = np.zeros_like(r)
    for dy in range(2 * NMS_R + 1):
        for dx in range(2 * NMS_R + 1):
            np.maximum(m, p[dy:dy + h, dx:dx + w], out=m)
    ys, xs = np.nonzero((r > 0) & (r == m))
    rv = r[ys, xs]
    order = np.lexsort((xs, ys, -rv))[:K]
    n = len(order)
    pos = np.zeros((K, 2), np.int32)
    val = np.zeros(K, np.int32)
    pos[:n, 0], pos[:n, 1], val[:n] = xs[order], ys[order], rv[order]
    return pos, val, n


# ----------------------------------------------------------------------------- 4. grid
def _nearest(P, n, x, y, skip=-1):
    """Index of the candidate nearest to (x, y) and its squared distance; ties go to the lowest index."""
    best, bd = -1, None
    for c in range(n):
        if c == skip:
            continue
        d = (P[c][0] - x) ** 2 + (P[c][1] - y) ** 2
        if bd is None or d < bd:
            best, bd = c, d
    return best, bd


_DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1))


def _grow(P, n, s):
    """Cells (list of (i, j, candidate)) grown from seed s, or None."""
    a, du = _nearest(P, n, P[s][0], P[s][1], skip=s)
    if a < 0 or du == 0:
        return None
    ux, uy = P[a][0] - P[s][0], P[a][1] - P[s][1]
    b, dv = -1, None
    for c in range(n):
        if c == s or c == a:
            continue
        dx, dy = P[c][0] - P[s][0], P[c][1] - P[s][1]
        dd = dx * dx + dy * dy
        dot = ux * dx + uy * dy
        if dd == 0 or 4 * dot * dot >= 3 * du * dd:   # within 30 degrees of +-u
            continue
        if dv is None or dd < dv:
            b, dv = c, dd
    if b < 0 or 4 * dv > 25 * du:
        return None
    G = 2 * GRID_OFF + 1
    grid = [[-1] * G for _ in range(G)]
    used = [False] * n
    cells = []

    def at(i, j):
        if -GRID_OFF <= i <= GRID_OFF and -GRID_OFF <= j <= GRID_OFF:
            return grid[j + GRID_OFF][i + GRID_OFF]
        return -2   # outside: neither empty nor placed

    def put(i, j, c):
        grid[j + GRID_OFF][i + GRID_OFF] = c
        used[c] = True
        cells.append((i, j, c))

    put(0, 0, s)
    put(1, 0, a)
    put(0, 1, b)
    for _ in range(MAX_PASSES):
        snap = len(cells)
        for k in range(snap):
            i, j, c = cells[k]
            px, py = P[c]
            for di, dj in _DIRS:
                if at(i + di, j + dj) != -1:
                    continue
                o = at(i - di, j - dj)
                pred = None
                if o >= 0:
                    pred = (2 * px - P[o][0], 2 * py - P[o][1])
                else:
                    qi, qj = abs(dj), abs(di)
                    for sg in (1, -1):
                        q = at(i + sg * qi, j + sg * qj)
                        qd = at(i + sg * qi + di, j + sg * qj + dj)
                        if q >= 0 and qd >= 0:
                            pred = (px + P[qd][0] - P[q][0], py + P[qd][1] - P[q][1])
                            break
                if pred is None:
                    continue
                step = (pred[0] - px) ** 2 + (pred[1] - py) ** 2
                if step == 0:
                    continue
                c2, d2 = _nearest(P, n, pred[0], pred[1])
                if c2 < 0 or used[c2] or 100 * d2 > 9 * step:
                    continue
                put(i + di, j + dj, c2)
                if len(cells) > N_CORNERS:
                    return None
        if len(cells) == snap:
            break
    return cells


def _canonical(P, cells):
    """54 candidate indices in objp's order (9 fast, 6 slow, not mirrored, first corner with the smaller (y, x)),
    or None."""
    if cells is None or len(cells) != N_CORNERS:
        return None
    i0, i1 = min(c[0] for c in cells), max(c[0] for c in cells)
    j0, j1 = min(c[1] for c in cells), max(c[1] for c in cells)
    ni, nj = i1 - i0 + 1, j1 - j0 + 1
    if (ni, nj) not in ((9, 6), (6, 9)):
        return None
    g = [[-1] * 9 for _ in range(6)]
    for i, j, c in cells:
        r, k = (j - j0, i - i0) if ni == 9 else (i - i0, j - j0)
        g[r][k] = c
    if any(c < 0 for row in g for c in row):
        return None
    a, b, d = P[g[0][0]], P[g[0][1]], P[g[1][0]]
    cross = (b[0] - a[0]) * (d[1] - a[1]) - (b[1] - a[1]) * (d[0] - a[0])
    if cross == 0:
        return None
    if cross < 0:
        g = [row[::-1] for row in g]
    f, l = P[g[0][0]], P[g[5][8]]
    if (l[1], l[0]) < (f[1], f[0]):
        g = [row[::-1] for row in g[::-1]]
    return [c for row in g for c in row]


GATE = 4        # the grid uses the candidates with GATE * R >= the strongest candidate's R


def gated_count(resp, count):
    """Candidates are sorted by R descending: the gate keeps a prefix.  It drops the weak maxima that noise leaves at
    the centres of the squares, which otherwise sit between the corners as nearest neighbours."""
    n = int(count)
    r0 = int(resp[0]) if n else 0
    while n > 0 and GATE * int(resp[n - 1]) < r0:
        n -= 1
    return n


def chess_grid(pos, resp, count, scale=1.0):
    """Candidates of one image -> (found, corners (54, 2) float64 in full-frame pixels (NaN if not found),
    idx (54,) int32 candidate indices (-1 if not found), seed used (-1 if none))."""
    n = gated_count(resp, count)
    P = [(int(x), int(y)) for x, y in np.asarray(pos)[:n]]
    for s in range(min(n, MAX_SEEDS)):
        if n < N_CORNERS:
            break
        order = _canonical(P, _grow(P, n, s))
        if order is not None:
            xy = np.array([P[c] for c in order], np.float64)
            return True, xy / scale + (1.0 / scale - 1.0) / 2.0, np.array(order, np.int32), s
    return False, np.full((N_CORNERS, 2), np.nan), np.full(N_CORNERS, -1, np.int32), -1


# ----------------------------------------------------------------------------- 6. cornerSubPix
def _patch(img, cx, cy, size):
    """cv2.getRectSubPix: (size, size) float64 samples centred on (cx, cy), bilinear, replicated border."""
    h, w = img.shape
    x0, y0 = cx - (size - 1) * 0.5, cy - (size - 1) * 0.5
    ix, iy = math.floor(x0), math.floor(y0)
    fx, fy = x0 - ix, y0 - iy
    xs = np.clip(np.arange(ix, ix + size + 1), 0, w - 1)
    ys = np.clip(np.arange(iy, iy + size + 1), 0, h - 1)
    t = img[np.ix_(ys, xs)].astype(np.float64)
    top = t[:-1, :-1] * (1.0 - fx) + t[:-1, 1:] * fx
    bot = t[1:, :-1] * (1.0 - fx) + t[1:, 1:] * fx
    return top * (1.0 - fy) + bot * fy


def corner_subpix(gray, corners, win=11, criteria=(30, 1e-3)):
    """cv2.cornerSubPix(gray, corners, (win, win), (-1, -1), (EPS + MAX_ITER, max_iter, eps)) as documented, in
    float64.  gray uint8 (h, w); corners (n, 2) [x, y]; returns the refined (n, 2).  NaN rows stay NaN."""
    img = np.asarray(gray)
    h, w = img.shape
    max_iter, eps = int(criteria[0]), float(criteria[1])
    eps = eps * eps
    k = np.arange(-win, win + 1, dtype=np.float64)
    wt = np.exp(-(k / win) * (k / win))
    m = wt[:, None] * wt[None, :]
    px, py = k[None, :], k[:, None]
    out = np.array(corners, np.float64).reshape(-1, 2).copy()
    tiny = np.finfo(np.float64).eps ** 2
    for n in range(out.shape[0]):
        x0, y0 = out[n]
        if not (np.isfinite(x0) and np.isfinite(y0)):
            continue
        x, y = x0, y0
        for _ in range(max(max_iter, 1)):
            s = _patch(img, x, y, 2 * win + 3)
            gx = s[1:-1, 2:] - s[1:-1, :-2]
            gy = s[2:, 1:-1] - s[:-2, 1:-1]
            gxx, gxy, gyy = gx * gx * m, gx * gy * m, gy * gy * m
            a, b, c = gxx.sum(), gxy.sum(), gyy.sum()
            bb1 = (gxx * px + gxy * py).sum()
            bb2 = (gxy * px + gyy * py).sum()
            det = a * c - b * b
            if abs(det) <= tiny:
                break
            sc = 1.0 / det
            nx = x + (c * sc * bb1 - b * sc * bb2)
            ny = y + (a * sc * bb2 - b * sc * bb1)
            err = (nx - x) ** 2 + (ny - y) ** 2
            x, y = nx, ny
            if x < 0 or x >= w or y < 0 or y >= h:
                break
            if err <= eps:
                break
        if abs(x - x0) > win or abs(y - y0) > win:
            x, y = x0, y0
        out[n] = x, y
    return out.reshape(np.shape(corners))


# ----------------------------------------------------------------------------- the chain
def resize_gray(gray, scale):
    """mq_cmc_preprocess's resize of a gray image (cv2 INTER_LINEAR, 11-bit taps) for scale < 1."""
    if scale == 1.0:
        return np.asarray(gray)
    from cmc_ref import resize_linear_u8
    return resize_linear_u8(np.asarray(gray), scale)


def find_chessboard(gray, scale=None, win=11, criteria=(30, 1e-3), K=256, refine=True):
    """gray uint8 (H, W) -> (found, corners (54, 2) float64): stages 2-6."""
    gray = np.asarray(gray)
    scale = default_scale(gray.shape[1]) if scale is None else float(scale)
    small = resize_gray(gray, scale)
    pos, val, n = chess_candidates(chess_response(small), K)
    found, corners, _, _ = chess_grid(pos, val, n, scale)
    if found and refine:
        corners = corner_subpix(gray, corners, win, criteria)
    return found, corners


# ----------------------------------------------------------------------------- renderer
def rot_xyz(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def board_corners(square=1.0):
    """objp of the reference (:34-35): (54, 3), x fastest over 9, y over 6."""
    o = np.zeros((N_CORNERS, 3))
    o[:, :2] = np.mgrid[0:9, 0:6].T.reshape(-1, 2) * square
    return o


def project(X, R, t, f, cx, cy, k1):
    Xc = X @ R.T + t
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    d = 1.0 + k1 * (x * x + y * y)
    return np.stack([f * x * d + cx, f * y * d + cy], 1)


def render_view(width, height, f, R, t, k1=0.0, ss=3, seed=0, noise=3.0, background=True, margin=0.6):
    """A 10 x 7-square board (inner corners at board (0..8, 0..5, 0), unit squares) at pose (R, t) seen by a pinhole
    camera with one radial coefficient: every sub-sample's ray is undistorted (fixed-point iteration), cast onto the
    board plane and coloured; ss x ss sub-samples are box-filtered.  Returns (gray uint8 (height, width), the analytic
    corner pixels (54, 2) in objp's order)."""
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    rng = np.random.default_rng(seed)
    sub = (np.arange(ss) + 0.5) / ss - 0.5
    xs = (np.arange(width)[:, None] + sub[None, :]).ravel()
    ys = (np.arange(height)[:, None] + sub[None, :]).ravel()
    xd, yd = np.meshgrid((xs - cx) / f, (ys - cy) / f)
    xu, yu = xd.copy(), yd.copy()
    for _ in range(25):
        d = 1.0 + k1 * (xu * xu + yu * yu)
        xu, yu = xd / d, yd / d
    # ray (xu, yu, 1) meets the plane z_board = 0: board point = R^T (lam ray - t)
    r2 = R[:, 2]
    den = r2[0] * xu + r2[1] * yu + r2[2]
    lam = float(r2 @ t) / np.where(np.abs(den) < 1e-12, 1e-12, den)
    Xc = np.stack([lam * xu - t[0], lam * yu - t[1], lam - t[2]], -1)
    bx, by = Xc @ R[:, 0], Xc @ R[:, 1]
    hit = lam > 0
    inside = hit & (bx >= -1) & (bx < 9) & (by >= -1) & (by < 6)
    rim = hit & (bx >= -1 - margin) & (bx < 9 + margin) & (by >= -1 - margin) & (by < 6 + margin)
    black = ((np.floor(bx).astype(np.int64) + np.floor(by).astype(np.int64)) & 1) == 0
    if background:
        blk = 16
        bg = rng.integers(40, 200, size=((height + blk - 1) // blk, (width + blk - 1) // blk)).astype(np.float64)
        bg = np.kron(bg, np.ones((blk * ss, blk * ss)))[:height * ss, :width * ss]
    else:
        bg = np.full((height * ss, width * ss), 120.0)
    img = np.where(rim, 225.0, bg)
    img = np.where(inside, np.where(black, 30.0, 225.0), img)
    img = img.reshape(height, ss, width, ss).mean(axis=(1, 3))
    img = img + noise * rng.standard_normal(img.shape)
    gray = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return gray, project(board_corners(), R, t, f, cx, cy, k1)


def canonical_truth(uv):
    """The analytic corners in the detector's canonical order: of the two orderings 180 degrees apart, the one whose
    first corner has the smaller (y, x)."""
    uv = np.asarray(uv)
    f, l = uv[0], uv[-1]
    return uv[::-1].copy() if (l[1], l[0]) < (f[1], f[0]) else uv.copy()


@functools.lru_cache(maxsize=None)
def make_view(name):
    """The named test views: (gray, truth in canonical order, refinement window for its spacing).  Cached: callers
    share one rendering and must not write to it."""
    c = np.array([4.0, 2.5, 0.0])

    def pose(rx, ry, rz, z, off=(0.0, 0.0)):
        R = rot_xyz(math.radians(rx), math.radians(ry), math.radians(rz))
        return R, np.array([off[0], off[1], z]) - R @ c

    views = {
        # name: (width, height, f, (rx, ry, rz, z, offset), k1, ss, seed, win)
        "frontal": (640, 480, 520.0, (0, 0, 0, 16.0), -0.25, 3, 1, 11),
        "tilt_x": (640, 480, 520.0, (40, 0, 8, 17.0), -0.25, 3, 2, 11),
        "tilt_y": (640, 480, 520.0, (10, -45, -12, 17.0, (0.5, 0.3)), -0.3, 3, 3, 11),
        "rot170": (640, 480, 520.0, (15, 10, 170, 16.0), -0.25, 3, 4, 11),
        "big": (1280, 960, 1040.0, (20, -15, 25, 16.0), -0.25, 3, 5, 11),
        "cut": (640, 480, 520.0, (0, 0, 5, 16.0, (8.5, 0.0)), -0.25, 3, 6, 11),
        "small_a": (320, 240, 260.0, (0, 0, 10, 13.0), -0.25, 4, 7, 5),
        "small_b": (320, 240, 260.0, (25, 20, -30, 13.5), -0.25, 4, 8, 5),
        "small_cut": (320, 240, 260.0, (0, 0, 0, 13.0, (7.0, 0.0)), -0.25, 4, 9, 5),
    }
    w, h, f, p, k1, ss, seed, win = views[name]
    R, t = pose(*p)
    gray, uv = render_view(w, h, f, R, t, k1, ss, seed)
    truth = canonical_truth(uv)
    gray.setflags(write=False)
    truth.setflags(write=False)
    return gray, truth, win


def subpix_edge_case():
    """A crop of the frontal view that leaves its first corner 3 px from the left and top edges: (gray, truth)."""
    gray, truth, _ = make_view("frontal")
    x0, y0 = int(round(truth[0, 0])) - 3, int(round(truth[0, 1])) - 3
    return np.ascontiguousarray(gray[y0:, x0:]), truth - np.array([x0, y0], np.float64)


@functools.lru_cache(maxsize=None)
def make_empty(width=640, height=480, seed=11):
    """A frame without a board: the blocky background and noise only."""
    R, t = rot_xyz(0, 0, 0), np.array([0.0, 0.0, -10.0])   # the board is behind the camera
    return render_view(width, height, 500.0, R, t, 0.0, 1, seed)[0]


@functools.lru_cache(maxsize=None)
def calibration_views(n=8, width=640, height=480, f=520.0, k1=-0.1):
    """n rendered views of one camera for the end-to-end calibration: (frames list of gray, truth list, f)."""
    c = np.array([4.0, 2.5, 0.0])
    poses = [(0, 0, 0, 16.0, (0, 0)), (35, 0, 5, 17.0, (0.5, 0)), (-35, 5, -8, 17.0, (0, 0.5)),
             (5, 38, 12, 17.0, (-0.5, 0)), (0, -38, -15, 17.0, (0, -0.5)), (25, 25, 30, 17.5, (1.0, 0.5)),
             (-25, 20, 160, 17.5, (-1.0, 0.5)), (20, -28, -40, 17.5, (0.5, -1.0))][:n]
    frames, truth = [], []
    for s, (rx, ry, rz, z, off) in enumerate(poses):
        R = rot_xyz(math.radians(rx), math.radians(ry), math.radians(rz))
        t = np.array([off[0], off[1], z]) - R @ c
        g, uv = render_view(width, height, f, R, t, k1, 3, 20 + s)
        frames.append(g)
        truth.append(canonical_truth(uv))
    return frames, truth, f
