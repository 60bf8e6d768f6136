"""NumPy restatement of the ArUco-marker detector (csrc/aruco.hip, csrc/aruco_dev.hpp), the
definition the kernels are held to, with the marker renderer and the seeded test dictionary the tests use.

The detector is this project's own (cv2 is not a dependency; parity with cv2.aruco is not pinned):
  1. detection image   resize (mq_resize_bilinear's fixed-point rule), then gray (mq_cmc_preprocess at scale 1)
  2. threshold         dark = gray n < boxsum - c n over a (2 r + 1)^2 window, replicated border, integers
  3. label             4-connected components of the dark pixels, label = smallest linear index, light = -1
  4. components        area, bounding box, extreme pixel in 8 directions; gates; ascending label order
  5. quads             corner set by shoelace area, sub-pixel sides by profiles + total least squares, homography,
                       6 x 6 cells, border test, dictionary match over four rotations
  6. find_markers      order by (id, label), map to frame pixels p ratio + (ratio - 1) / 2
Stages 2-4 are integer and unique; stage 5 is float64 in the order of the per-lane core."""
import functools
import math

import numpy as np

import cmc_ref
import track_video_ref

# ----------------------------------------------------------------------------- constants
THR_R = 11              # half window of the adaptive threshold
THR_C = 7               # its constant (cv2's adaptiveThreshConstant)
MIN_AREA = 100          # dark pixels of a component
MIN_BOX = 12            # bounding-box side, pixels
MAX_QUADS = 64
CAND_FIELDS = 16        # label, area, x0, y0, x1, y1, 8 extremes (linear indices), 2 spare
DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))   # x, x+y, y, y-x, -x, -x-y, -y, x-y
DIAG_SET = (5, 7, 1, 3)  # top-left, top-right, bottom-right, bottom-left: clockwise with y down
AXIS_SET = (6, 0, 2, 4)  # top, right, bottom, left
MIN_SIDE = 10           # pixels between adjacent corners
FILL_LO = (1, 16)       # component area / quad area >= 1 / 16: the border alone is 20 / 36, but the threshold hollows
                        # dark regions wider than its window to a band of about 10 px along the outline, 40 / side
FILL_HI = (5, 4)        # ... <= 5 / 4 (an all-dark marker, pixel centres against pixel areas)
N_PROF = 16             # profiles per side, at 0.2 + 0.6 (j + 0.5) / 16 along it
PROF_HALF = 3.0         # profile from -3 (inside) to +3 px (outside) in steps of 0.5: 13 samples
PROF_N = 13
MIN_EDGE = 20.0         # gray levels between a profile's ends
MIN_PROFILES = 8        # valid profiles a side needs
MAX_MOVE = 4.0          # a refined corner stays this near its pixel corner, per axis
MIN_CONTRAST = 30.0     # gray levels between the darkest and lightest cell
CELL_OFF = (0.3, 0.5, 0.7)   # 3 x 3 samples inside each cell


# ----------------------------------------------------------------------------- dictionary
def code_bits(code):
    """uint16 -> (4, 4) 0 / 1, row-major from the most significant bit, white = 1."""
    return np.array([(int(code) >> (15 - k)) & 1 for k in range(16)], np.int64).reshape(4, 4)


def bits_code(m):
    return int(sum(int(b) << (15 - k) for k, b in enumerate(np.asarray(m).ravel())))


def rot_code(code, r):
    """The code of the marker turned clockwise r times by 90 degrees."""
    return bits_code(np.rot90(code_bits(code), -int(r)))


def hamming(a, b):
    return bin((int(a) ^ int(b)) & 0xFFFF).count("1")


@functools.lru_cache(maxsize=None)
def make_dictionary(n=16, seed=5, min_dist=4):
    """n seeded 4 x 4 codes whose Hamming distance over all rotations (a code against its own turns included) is at
    least min_dist.  Not cv2's dictionary."""
    rng = np.random.default_rng(seed)
    codes = []
    while len(codes) < n:
        c = int(rng.integers(0, 1 << 16))
        ok = all(hamming(c, rot_code(c, r)) >= min_dist for r in (1, 2, 3))
        ok = ok and all(hamming(c, rot_code(d, r)) >= min_dist for d in codes for r in range(4))
        if ok:
            codes.append(c)
    out = np.array(codes, np.uint16)
    out.setflags(write=False)
    return out


def marker_cells(code):
    """(6, 6) cells, 1 = white: a dark border around the code."""
    m = np.zeros((6, 6), np.int64)
    m[1:5, 1:5] = code_bits(code)
    return m


# ----------------------------------------------------------------------------- renderer
def rot_xyz(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


FLIP = np.diag([1.0, -1.0, -1.0])   # the marker's frame has y up and z towards the camera


def marker_pose(rx, ry, rz, pos):
    """Marker frame -> camera frame: angles in degrees about the camera's axes (0, 0, 0: upright, facing the
    camera), pos the marker's centre in the camera frame."""
    return rot_xyz(math.radians(rx), math.radians(ry), math.radians(rz)) @ FLIP, np.asarray(pos, np.float64)


def marker_objp(L):
    """cv2's order: top-left, top-right, bottom-right, bottom-left in the marker's frame (y up)."""
    return np.array([[-L / 2, L / 2, 0], [L / 2, L / 2, 0], [L / 2, -L / 2, 0], [-L / 2, -L / 2, 0]], np.float64)


def project(X, R, t, f, cx, cy, k1=0.0):
    Xc = np.atleast_2d(X) @ R.T + t
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    d = 1.0 + k1 * (x * x + y * y)
    return np.stack([f * x * d + cx, f * y * d + cy], 1)


def render_scene(width, height, f, markers, k1=0.0, ss=3, seed=0, noise=3.0, quiet=1.5, centre=None):
    """markers: a list of (R, t, L, cells (6, 6)); each is a plane patch of side L in a white quiet zone of `quiet`
    cells, seen by a pinhole camera with one radial coefficient.  Every sub-sample's ray is undistorted, cast onto
    the marker's plane and coloured; ss x ss sub-samples are box-filtered over a seeded blocky background, then
    noise.  Returns (gray uint8 (height, width), [corners (4, 2) in cv2's order], [centre (2,)])."""
    cx, cy = ((width - 1) / 2.0, (height - 1) / 2.0) if centre is None else centre
    rng = np.random.default_rng(seed)
    sub = (np.arange(ss) + 0.5) / ss - 0.5
    xs = (np.arange(width)[:, None] + sub[None, :]).ravel()
    ys = (np.arange(height)[:, None] + sub[None, :]).ravel()
    xd, yd = np.meshgrid((xs - cx) / f, (ys - cy) / f)
    xu, yu = xd.copy(), yd.copy()
    if k1 != 0.0:
        for _ in range(25):
            d = 1.0 + k1 * (xu * xu + yu * yu)
            xu, yu = xd / d, yd / d
    blk = 16
    bg = rng.integers(60, 200, size=((height + blk - 1) // blk, (width + blk - 1) // blk)).astype(np.float64)
    img = np.kron(bg, np.ones((blk * ss, blk * ss)))[:height * ss, :width * ss]
    corners, centres = [], []
    for R, t, L, cells in markers:
        cell = L / 6.0
        r2 = R[:, 2]
        den = r2[0] * xu + r2[1] * yu + r2[2]
        lam = float(r2 @ t) / np.where(np.abs(den) < 1e-12, 1e-12, den)
        Xc = np.stack([lam * xu - t[0], lam * yu - t[1], lam - t[2]], -1)
        col = (Xc @ R[:, 0]) / cell + 3.0            # cells from the marker's left edge
        row = 3.0 - (Xc @ R[:, 1]) / cell            # cells from its top edge
        hit = lam > 0
        inside = hit & (col >= 0) & (col < 6) & (row >= 0) & (row < 6)
        rim = hit & (col >= -quiet) & (col < 6 + quiet) & (row >= -quiet) & (row < 6 + quiet)
        ci, ri = np.clip(np.floor(col).astype(np.int64), 0, 5), np.clip(np.floor(row).astype(np.int64), 0, 5)
        white = np.asarray(cells)[ri, ci] > 0
        img = np.where(rim, 225.0, img)
        img = np.where(inside, np.where(white, 225.0, 30.0), img)
        corners.append(project(marker_objp(L), R, t, f, cx, cy, k1))
        centres.append(project(np.zeros((1, 3)), R, t, f, cx, cy, k1)[0])
    img = img.reshape(height, ss, width, ss).mean(axis=(1, 3))
    img = img + noise * rng.standard_normal(img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), corners, centres


VIEW_F = 300.0
VIEW_K1 = -0.15
VIEW_L = 1.0
# name: (rx, ry, rz, position, dictionary index, seed)
VIEWS = {
    "frontal": (0, 0, 0, (0.2, -0.1, 4.5), 3, 1),
    "tilt40": (40, 0, 8, (-0.3, 0.2, 4.0), 5, 2),
    "rot45": (0, 0, 45, (0.4, 0.3, 4.5), 7, 3),
    "rot22": (10, -15, 22.5, (-0.5, -0.2, 4.5), 9, 4),
    "small30": (0, 0, 100, (1.0, 0.8, 10.0), 11, 5),        # side 300 / 10 = 30 px, turned past 90 degrees
    "cut": (0, 0, 5, (2.55, 0.0, 4.5), 2, 6),               # the right edge of the frame cuts the marker
}
VIEW_NAMES = ("frontal", "tilt40", "rot45", "rot22", "small30")


@functools.lru_cache(maxsize=None)
def make_view(name, width=320, height=240, scale=1):
    """A named test view: (gray, corners (4, 2) in cv2's order, centre (2,), id).  scale renders the same view at
    scale times the size.  Cached: callers share one rendering and must not write to it."""
    rx, ry, rz, pos, k, seed = VIEWS[name]
    R, t = marker_pose(rx, ry, rz, pos)
    code = int(make_dictionary()[k])
    gray, c, m = render_scene(width * scale, height * scale, VIEW_F * scale, [(R, t, VIEW_L, marker_cells(code))],
                              VIEW_K1, 3, seed)
    for a in (gray, c[0], m[0]):
        a.setflags(write=False)
    return gray, c[0], m[0], k


@functools.lru_cache(maxsize=None)
def make_special(name, width=320, height=240):
    """Frames in which nothing must be found (and the codes near a dictionary code): gray only."""
    R, t = marker_pose(5, -5, 10, (0.1, 0.1, 4.5))
    d = make_dictionary()
    if name == "empty":
        gray = render_scene(width, height, VIEW_F, [], 0.0, 1, 11)[0]
    elif name == "bad_border":                       # a dark square whose border has three white cells
        cells = marker_cells(int(d[4]))
        cells[0, 2] = cells[3, 0] = cells[5, 4] = 1
        gray = render_scene(width, height, VIEW_F, [(R, t, VIEW_L, cells)], VIEW_K1, 3, 12)[0]
    elif name == "foreign":                          # a well-formed marker whose code is not in the dictionary
        code = next(c for c in range(1, 1 << 16) if min(hamming(c, rot_code(int(e), r)) for e in d for r in range(4)) >= 3)
        gray = render_scene(width, height, VIEW_F, [(R, t, VIEW_L, marker_cells(code))], VIEW_K1, 3, 13)[0]
    elif name in ("one_off", "two_off"):             # dictionary code 6 with one / two bits flipped
        code = int(d[6]) ^ (0x0040 if name == "one_off" else 0x0240)
        gray = render_scene(width, height, VIEW_F, [(R, t, VIEW_L, marker_cells(code))], VIEW_K1, 3, 14)[0]
    else:
        raise KeyError(name)
    gray.setflags(write=False)
    return gray


# ----------------------------------------------------------------------------- 2. threshold
def threshold(gray, r=THR_R, c=THR_C):
    """gray uint8 (h, w) -> uint8 (h, w), 1 where dark."""
    g = np.asarray(gray).astype(np.int64)
    h, w = g.shape
    k = 2 * r + 1
    p = np.pad(g, r, mode="edge")
    ii = np.zeros((h + k, w + k), np.int64)
    ii[1:, 1:] = p.cumsum(0).cumsum(1)
    box = ii[k:, k:] - ii[:-k, k:] - ii[k:, :-k] + ii[:-k, :-k]
    n = k * k
    return (g * n < box - c * n).astype(np.uint8)


# ----------------------------------------------------------------------------- 3. label
def label(dark):
    """uint8 / bool (h, w) -> int32 (h, w): the smallest linear index of the pixel's 4-connected component of dark
    pixels, -1 where light."""
    dark = np.asarray(dark).astype(bool)
    h, w = dark.shape
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    left = np.zeros_like(dark)
    left[:, 1:] = dark[:, :-1]
    run = np.maximum.accumulate(np.where(dark & ~left, idx, -1), axis=1)
    parent = np.where(dark, run, -1).ravel().copy()

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    need = dark[1:] & dark[:-1] & ~(left[1:] & left[:-1])      # the pair to the left already joins the two runs
    ys, xs = np.nonzero(need)
    for a, b in zip(((ys + 1) * w + xs).tolist(), (ys * w + xs).tolist()):
        ra, rb = find(a), find(b)
        if ra < rb:
            parent[rb] = ra
        elif rb < ra:
            parent[ra] = rb
    on = parent >= 0
    while True:
        nxt = parent.copy()
        nxt[on] = parent[parent[on]]
        if (nxt == parent).all():
            break
        parent = nxt
    return parent.reshape(h, w).astype(np.int32)


# ----------------------------------------------------------------------------- 4. components
def components(labels, max_quads=MAX_QUADS, min_area=MIN_AREA, min_box=MIN_BOX):
    """int32 (h, w) labels -> (count, cand int32 (max_quads, 16)): the components with area >= min_area, both
    bounding-box sides >= min_box and the box clear of the image border, in ascending label order; count is their
    number, of which cand holds the first max_quads: label, area, x0, y0, x1, y1, then the extreme pixel (linear
    index) in each of DIRS, the largest index among equal projections; the rest zero."""
    lab = np.asarray(labels)
    h, w = lab.shape
    cand = np.zeros((max_quads, CAND_FIELDS), np.int32)
    flat = lab.ravel()
    on = np.nonzero(flat >= 0)[0]
    roots, inv, area = np.unique(flat[on], return_inverse=True, return_counts=True)
    count = 0
    for k in np.nonzero(area >= min_area)[0]:
        px = on[inv == k]
        y, x = px // w, px % w
        x0, y0, x1, y1 = x.min(), y.min(), x.max(), y.max()
        if x1 - x0 + 1 < min_box or y1 - y0 + 1 < min_box or x0 < 1 or y0 < 1 or x1 > w - 2 or y1 > h - 2:
            continue
        if count < max_quads:
            ext = []
            for dx, dy in DIRS:
                proj = dx * x + dy * y
                ext.append(px[proj == proj.max()].max())
            cand[count, :14] = [roots[k], area[k], x0, y0, x1, y1] + ext
        count += 1
    return count, cand


# ----------------------------------------------------------------------------- 5. quads
def shoelace2(q):
    """Twice the signed area of the polygon q (k, 2), positive clockwise with y down."""
    x, y = q[:, 0].astype(np.int64), q[:, 1].astype(np.int64)
    return int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def pick_quad(cand, w):
    """One candidate row -> the pixel quad (4, 2) int64 [x, y], clockwise from the top-left (diagonal set) or the top
    (axis set), or None."""
    ext = cand[6:14].astype(np.int64)
    pts = np.stack([ext % w, ext // w], 1)
    qd, qa = pts[list(DIAG_SET)], pts[list(AXIS_SET)]
    q = qd if shoelace2(qd) >= shoelace2(qa) else qa
    a2 = shoelace2(q)
    for k in range(4):
        a, b, c = q[k], q[(k + 1) % 4], q[(k + 2) % 4]
        e0, e1 = b - a, c - b
        if e0[0] * e1[1] - e0[1] * e1[0] <= 0 or e0[0] * e0[0] + e0[1] * e0[1] < MIN_SIDE * MIN_SIDE:
            return None
    area = int(cand[1])
    if 2 * area * FILL_LO[1] < FILL_LO[0] * a2 or 2 * area * FILL_HI[1] > FILL_HI[0] * a2:
        return None
    return q


def bilinear(gray, x, y):
    """float64 bilinear samples with replicated border; x, y arrays."""
    h, w = gray.shape
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb = np.clip(xi, 0, w - 1), np.clip(xi + 1, 0, w - 1)
    ya, yb = np.clip(yi, 0, h - 1), np.clip(yi + 1, 0, h - 1)
    g = gray.astype(np.float64)
    top = (1.0 - fx) * g[ya, xa] + fx * g[ya, xb]
    bot = (1.0 - fx) * g[yb, xa] + fx * g[yb, xb]
    return (1.0 - fy) * top + fy * bot


def refine_quad(gray, q):
    """Pixel quad -> sub-pixel corners (4, 2) float64, or None: per side 16 profiles across it, the crossing of each
    profile's mid-level, a total-least-squares line, corners = intersections of adjacent lines."""
    q = q.astype(np.float64)
    mean, vec = [], []
    for k in range(4):
        a, b = q[k], q[(k + 1) % 4]
        d = b - a
        ln = math.sqrt(d[0] * d[0] + d[1] * d[1])
        tx, ty = d[0] / ln, d[1] / ln
        nx, ny = ty, -tx                                        # outward for a clockwise quad, y down
        sj = 0.2 + 0.6 * ((np.arange(N_PROF) + 0.5) / N_PROF)
        bxs, bys = a[0] + sj * d[0], a[1] + sj * d[1]
        u = -PROF_HALF + 0.5 * np.arange(PROF_N)
        prof = bilinear(gray, bxs[:, None] + u[None, :] * nx, bys[:, None] + u[None, :] * ny)
        pts = []
        for j in range(N_PROF):
            p, bx, by = prof[j], bxs[j], bys[j]
            lo, hi = p.min(), p.max()
            if hi - lo < MIN_EDGE:
                continue
            mid = 0.5 * (lo + hi)
            m = next((m for m in range(PROF_N - 1) if p[m] < mid <= p[m + 1]), None)
            if m is None:
                continue
            us = u[m] + 0.5 * (mid - p[m]) / (p[m + 1] - p[m])
            pts.append((bx + us * nx, by + us * ny))
        if len(pts) < MIN_PROFILES:
            return None
        pts = np.array(pts)
        mx, my = pts[:, 0].sum() / len(pts), pts[:, 1].sum() / len(pts)
        dx, dy = pts[:, 0] - mx, pts[:, 1] - my
        sxx, sxy, syy = (dx * dx).sum(), (dx * dy).sum(), (dy * dy).sum()
        lam = 0.5 * (sxx + syy) + math.sqrt((0.5 * (sxx - syy)) ** 2 + sxy * sxy)
        v = (lam - syy, sxy) if sxx >= syy else (sxy, lam - sxx)
        nv = math.sqrt(v[0] * v[0] + v[1] * v[1])
        if not nv > 0.0:
            return None
        mean.append((mx, my))
        vec.append((v[0] / nv, v[1] / nv))
    out = np.zeros((4, 2))
    for k in range(4):
        (ax, ay), (avx, avy) = mean[(k + 3) % 4], vec[(k + 3) % 4]
        (bx, by), (bvx, bvy) = mean[k], vec[k]
        den = avx * bvy - avy * bvx
        if abs(den) < 1e-6:
            return None
        s = ((bx - ax) * bvy - (by - ay) * bvx) / den
        out[k] = ax + s * avx, ay + s * avy
        if abs(out[k, 0] - q[k, 0]) > MAX_MOVE or abs(out[k, 1] - q[k, 1]) > MAX_MOVE:
            return None
    return out


def square_to_quad(c):
    """(a, b, c, d, e, f, g, h) of the homography that takes the unit square's (0,0), (1,0), (1,1), (0,1) to the quad's
    corners: x = (a u + b v + c) / (g u + h v + 1), y = (d u + e v + f) / (g u + h v + 1)."""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = c
    dx1, dx2, sx = x1 - x2, x3 - x2, x0 - x1 + x2 - x3
    dy1, dy2, sy = y1 - y2, y3 - y2, y0 - y1 + y2 - y3
    den = dx1 * dy2 - dx2 * dy1
    g = (sx * dy2 - dx2 * sy) / den
    h = (dx1 * sy - sx * dy1) / den
    return x1 - x0 + g * x1, x3 - x0 + h * x3, x0, y1 - y0 + g * y1, y3 - y0 + h * y3, y0, g, h


def cell_sums(gray, c):
    """Refined corners -> (6, 6) sums of the 3 x 3 samples inside each cell."""
    A, B, C, D, E, F, G, H = square_to_quad(c)
    rr, cc = np.mgrid[0:6, 0:6]
    out = np.zeros((6, 6))
    for a in CELL_OFF:
        for b in CELL_OFF:
            u, v = (cc + b) / 6.0, (rr + a) / 6.0
            den = G * u + H * v + 1.0
            out = out + bilinear(gray, (A * u + B * v + C) / den, (D * u + E * v + F) / den)
    return out


def decode(gray, c, border_errors=0):
    """Refined corners -> the 16-bit code read in the quad's own orientation, or None."""
    s = cell_sums(gray, c)
    mn, mx = s.min(), s.max()
    if mx - mn < 9.0 * MIN_CONTRAST:
        return None
    bits = (s > 0.5 * (mn + mx)).astype(np.int64)
    border = bits.sum() - bits[1:5, 1:5].sum()
    if border > border_errors:
        return None
    return bits_code(bits[1:5, 1:5])


def match(code, dictionary, max_correction_bits=0):
    """-> (id, rot) of the smallest Hamming distance over the four turns of every code (ties: lowest id, then lowest
    rot), or None above max_correction_bits.  dictionary None: (-1, 0)."""
    if dictionary is None:
        return -1, 0
    best = None
    for i, d in enumerate(np.asarray(dictionary).tolist()):
        for r in range(4):
            key = (hamming(code, rot_code(d, r)), i, r)
            best = key if best is None or key < best else best
    if best is None or best[0] > max_correction_bits:
        return None
    return best[1], best[2]


def quads(gray, count, cand, dictionary, max_correction_bits=0, border_errors=0):
    """Stage 5 on one image: (ok (max_quads,) int32, ids, rot, corners (max_quads, 4, 2) float64 in detection pixels,
    corner 0 the marker's top-left, clockwise; NaN where not ok)."""
    mq = cand.shape[0]
    ok, ids, rot = np.zeros(mq, np.int32), np.full(mq, -1, np.int32), np.zeros(mq, np.int32)
    corners = np.full((mq, 4, 2), np.nan)
    h, w = gray.shape
    for k in range(min(int(count), mq)):
        q = pick_quad(cand[k], w)
        if q is None:
            continue
        c = refine_quad(gray, q)
        if c is None:
            continue
        code = decode(gray, c, border_errors)
        if code is None:
            continue
        m = match(code, dictionary, max_correction_bits)
        if m is None:
            continue
        ok[k], ids[k], rot[k] = 1, m[0], m[1]
        corners[k] = c[[(j + m[1]) % 4 for j in range(4)]]
    return ok, ids, rot, corners


# ----------------------------------------------------------------------------- 1 + 6. the chain
def detection_image(frame, det_size):
    """uint8 BGR (H, W, 3) or gray (H, W) -> gray at det_size = (width, height): resize, then gray."""
    f = np.asarray(frame)
    if f.ndim == 2:
        f = np.repeat(f[:, :, None], 3, axis=2)
    if (f.shape[1], f.shape[0]) != tuple(det_size):
        f = track_video_ref.resize_bilinear(f, det_size[1], det_size[0])
    return cmc_ref.bgr_to_gray(f)


def find_markers(frame, dictionary, det_size=(640, 480), max_markers=8, max_quads=MAX_QUADS, max_correction_bits=0,
                 border_errors=0, return_stages=False):
    """One frame -> (count, ids (max_markers,) int32, corners (max_markers, 4, 2) float64 in frame pixels, NaN past the
    count), ordered by (id, label)."""
    f = np.asarray(frame)
    H, W = f.shape[:2]
    gray = detection_image(f, det_size)
    lab = label(threshold(gray))
    n, cand = components(lab, max_quads)
    ok, ids, rot, c = quads(gray, n, cand, dictionary, max_correction_bits, border_errors)
    order = sorted((int(ids[k]), int(cand[k, 0]), k) for k in range(max_quads) if ok[k])[:max_markers]
    out_ids = np.full(max_markers, -1, np.int32)
    out_c = np.full((max_markers, 4, 2), np.nan)
    rx, ry = W / det_size[0], H / det_size[1]
    for j, (_, _, k) in enumerate(order):
        out_ids[j] = ids[k]
        out_c[j, :, 0] = c[k, :, 0] * rx + (rx - 1.0) / 2.0
        out_c[j, :, 1] = c[k, :, 1] * ry + (ry - 1.0) / 2.0
    res = (len(order), out_ids, out_c)
    return res + ({"gray": gray, "labels": lab, "n_cand": n, "cand": cand, "ok": ok, "ids": ids, "rot": rot,
                   "corners": c},) if return_stages else res


def marker_centre(corners, f, cx, cy, k1=0.0):
    """Where the marker's centre projects, from its four corners: what a pose fitted to the corners and
    cv2.projectPoints of the origin give for an exact fit.  The corners are undistorted, the diagonals of the quad
    meet at the image of the square's centre, and that point is distorted again."""
    c = np.asarray(corners, np.float64)
    xd, yd = (c[:, 0] - cx) / f, (c[:, 1] - cy) / f
    xu, yu = xd.copy(), yd.copy()
    for _ in range(25):
        d = 1.0 + k1 * (xu * xu + yu * yu)
        xu, yu = xd / d, yd / d
    p0, p1, p2, p3 = np.stack([xu, yu], 1)
    a, b = p2 - p0, p3 - p1
    s = ((p1[0] - p0[0]) * b[1] - (p1[1] - p0[1]) * b[0]) / (a[0] * b[1] - a[1] * b[0])
    m = p0 + s * a
    d = 1.0 + k1 * (m[0] * m[0] + m[1] * m[1])
    return np.array([f * m[0] * d + cx, f * m[1] * d + cy])


# ----------------------------------------------------------------------------- a four-camera rig
RIG_F = 300.0
RIG_SIZE = (320, 240)


def look_at(position, target=(0.0, 0.0, 0.0)):
    """World -> camera (R, t) of a camera at `position` looking at `target`, image x to the right, y down, world y up."""
    C = np.asarray(position, np.float64)
    fwd = np.asarray(target, np.float64) - C
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right = right / np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    return R, -R @ C


def rodrigues_vec(R):
    """Rotation matrix -> rotation vector (angles well below pi)."""
    th = math.acos(max(-1.0, min(1.0, (np.trace(R) - 1.0) / 2.0)))
    if th < 1e-12:
        return np.zeros(3)
    return th / (2.0 * math.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


@functools.lru_cache(maxsize=None)
def rig_scene(n_pos=16, n_pad=5):
    """Four pinhole cameras (no distortion) around the z axis look at the origin; one marker (dictionary code 1, side
    1) faces them and moves through n_pos positions; n_pad frames without a marker follow (optimize_extrinsic leaves
    the last five rows out).  Returns (frames {cam: (n_pos + n_pad, 240, 320) uint8}, cams [(R, t)], centres
    (4, n_pos, 2) analytic, positions (n_pos, 3))."""
    W, H = RIG_SIZE
    cams = [look_at(p) for p in ((-1.8, 1.2, 5.0), (1.8, 1.2, 5.2), (-1.8, -1.2, 5.4), (1.8, -1.2, 5.0))]
    cells = marker_cells(int(make_dictionary()[1]))
    rng = np.random.default_rng(21)
    pos = np.stack([np.array([-0.9 + 0.6 * (k % 4), -0.6 + 0.4 * (k // 4), 0.0]) for k in range(n_pos)])
    pos[:, 2] = rng.uniform(-0.5, 0.5, n_pos)
    ang = rng.uniform(-12.0, 12.0, (n_pos, 3))
    frames = {c: [] for c in range(4)}
    centres = np.zeros((4, n_pos, 2))
    for k in range(n_pos):
        Rm = rot_xyz(*np.radians(ang[k]))
        for c, (Rc, tc) in enumerate(cams):
            R = Rc @ Rm                              # the marker's frame is the world's, turned a little
            g, _, m = render_scene(W, H, RIG_F, [(R, Rc @ pos[k] + tc, 1.0, cells)], 0.0, 2, 100 + 4 * k + c)
            frames[c].append(g)
            centres[c, k] = m[0]
    for c in range(4):
        for j in range(n_pad):
            frames[c].append(render_scene(W, H, RIG_F, [], 0.0, 1, 200 + 4 * j + c)[0])
        frames[c] = np.stack(frames[c])
        frames[c].setflags(write=False)
    return frames, cams, centres, pos


# ----------------------------------------------------------------------------- two markers and a cube's centre
CUBE_SIZE = 1.2


def cube_scene(tilt_b, seed, width=320, height=240):
    """Two markers (dictionary codes 2 and 8, side 1) in one frame, the first nearly frontal, the second tilted by
    tilt_b degrees; no lens distortion.  Returns (gray, [analytic projection of (0, 0, -CUBE_SIZE / 2) per marker])."""
    d = make_dictionary()
    off = np.array([[0.0, 0.0, -CUBE_SIZE / 2.0]])
    A = marker_pose(4, -3, 10, (-1.2, 0.1, 5.3))
    B = marker_pose(tilt_b, 4, -20, (1.2, -0.2, 5.3))
    marks = [(A[0], A[1], 1.0, marker_cells(int(d[2]))), (B[0], B[1], 1.0, marker_cells(int(d[8])))]
    gray = render_scene(width, height, VIEW_F, marks, 0.0, 3, seed)[0]
    proj = [project(off, R, t, VIEW_F, (width - 1) / 2.0, (height - 1) / 2.0)[0] for R, t in (A, B)]
    return gray, proj


def project_from_corners(corners, point, f, cx, cy, L=1.0):
    """The pose of a marker of side L from its four corners (a least-squares fit by scipy from a frontal start, no
    distortion) and the projection of `point` of the marker's frame: the CPU stand-in for calibrate_views +
    mq_camera_project."""
    from scipy.optimize import least_squares
    obj = marker_objp(L)

    def rot(r):
        th = np.linalg.norm(r)
        if th < 1e-12:
            return np.eye(3)
        k = r / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K

    def res(x):
        return (project(obj, rot(x[:3]), x[3:], f, cx, cy) - corners).ravel()

    side = np.linalg.norm(corners[1] - corners[0])
    c = corners.mean(axis=0)
    z = f * L / side
    x0 = np.concatenate([[math.pi, 0.0, 0.0], [(c[0] - cx) / f * z, (c[1] - cy) / f * z, z]])
    sol = least_squares(res, x0, xtol=1e-14, ftol=1e-14, gtol=1e-14).x
    return project(np.asarray(point, np.float64)[None], rot(sol[:3]), sol[3:], f, cx, cy)[0]


# ----------------------------------------------------------------------------- label test cases
def label_cases(h, w, seed=0):
    """name -> dark uint8 (h, w): the shapes that stress a parallel labelling."""
    rng = np.random.default_rng(seed)
    out = {}
    sp = np.zeros((h, w), np.uint8)                  # a rectangular spiral, one pixel wide, one pixel apart
    x = y = stuck = 0
    dx, dy = 1, 0
    sp[0, 0] = 1
    while stuck < 2:
        nx, ny = x + dx, y + dy
        ax, ay = nx + dx, ny + dy
        if 0 <= nx < w and 0 <= ny < h and not sp[ny, nx] and not (0 <= ax < w and 0 <= ay < h and sp[ay, ax]):
            x, y, stuck = nx, ny, 0
            sp[y, x] = 1
        else:
            dx, dy, stuck = -dy, dx, stuck + 1
    out["spiral"] = sp
    comb = np.zeros((h, w), np.uint8)                # teeth from a spine along the bottom row
    comb[h - 1, :] = 1
    comb[1:, ::2] = 1
    out["comb"] = comb
    u = np.zeros((h, w), np.uint8)                   # two arms that meet only in the last rows and columns
    u[0:h - 1, 1] = 1
    u[0:h - 1, w - 2] = 1
    u[h - 2, 1:w - 1] = 1
    out["u"] = u
    out["dark"] = np.ones((h, w), np.uint8)
    out["light"] = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    out["checker"] = ((yy + xx) & 1).astype(np.uint8)
    out["noise"] = (rng.random((h, w)) < 0.5).astype(np.uint8)
    return out
