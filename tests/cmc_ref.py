"""numpy restatement of boxmot 12.0.7 ``cmc/sift.py`` ``SIFT.apply`` (test helper, not product code).

Five stages, float32 where csrc/cmc.hip uses float32 and in the same operation order:

1. ``preprocess``     cv2.cvtColor(BGR2GRAY) + cv2.resize(fx=fy=scale, INTER_LINEAR), integer arithmetic;
2. ``make_mask``      the 2 % border and the scaled detection boxes;
3. ``sift_detect`` / ``sift_describe``   Lowe 2004 as cv2.SIFT_create(nOctaveLayers=3, contrastThreshold=0.02,
   edgeThreshold=20), sigma 1.6, assumed input blur 0.5;
4. ``match_knn2`` / ``filter_matches``   brute-force 2-NN on integer squared L2, ratio 0.9, spatial gate,
   boxmot's one-sided 2.5 sigma rule;
5. ``affine_partial_ransac``   2-point RANSAC for the 4-dof similarity on a deterministic hypothesis set,
   closed-form least-squares refit.

Where this restatement (and the kernels) fix a choice that cv2 leaves to its implementation:
orientation by atan2 rather than cv2's 0.3 degree fastAtan2 polynomial; the 3x3 refinement solve by the
adjugate in float32; octave decimation takes pixel (2y, 2x); octaves smaller than 11 px are not built (the 5 px
border leaves them no interior); histogram sums are accumulated in 2^-20 fixed point so that they do not
depend on summation order; at most MAXPEAK orientation peaks per extremum (lowest bins first), at most KCAND
extrema per image (scan order octave, layer, row, column) and at most KMAX keypoints, sorted by
(octave, layer, y, x, angle).  cv2 parity is unpinned.

Every keypoint carries a fragility margin: the smallest slack of any discrete decision that produced it,
expressed in DoG intensity units (see ``_Margin``).
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
KMAX = 2048
KCAND = 4096
MAXPEAK = 4
N_LAYERS = 3
CONTRAST = 0.02
EDGE = 20.0
SIGMA = 1.6
BORDER = 5
MAX_OCT = 8
PREFILTER = 0.5 * CONTRAST / N_LAYERS * 255  # |DoG| a candidate needs (cv2 floors this to 0 for float images)
FIX = 1048576.0  # 2^20 fixed-point scale of the histogram sums
FLT_EPS = f32(1.1920929e-07)


# ----------------------------------------------------------------------------- 1. preprocess
def bgr_to_gray(img):
    i = img.astype(np.int64)
    return ((i[..., 0] * 1868 + i[..., 1] * 9617 + i[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def _resize_taps(src, dst, scale):
    inv = 1.0 / scale
    d = np.arange(dst, dtype=np.float64)
    fx = ((d + 0.5) * inv - 0.5).astype(f32)
    sx = np.floor(fx).astype(np.int64)
    fx = fx - sx.astype(f32)
    lo = sx < 0
    fx[lo], sx[lo] = 0, 0
    hi = sx >= src - 1
    fx[hi], sx[hi] = 0, src - 1
    a0 = np.rint((f32(1) - fx) * f32(2048)).astype(np.int64)
    a1 = np.rint(fx * f32(2048)).astype(np.int64)
    return sx, np.minimum(sx + 1, src - 1), a0, a1


def small_size(h, w, scale=0.1):
    return int(np.rint(h * scale)), int(np.rint(w * scale))


def resize_linear_u8(gray, scale=0.1):
    """cv2.resize(gray, (0, 0), fx=scale, fy=scale, INTER_LINEAR) for uint8: 11-bit fixed-point weights."""
    h, w = gray.shape
    dh, dw = small_size(h, w, scale)
    x0, x1, a0, a1 = _resize_taps(w, dw, scale)
    y0, y1, b0, b1 = _resize_taps(h, dh, scale)
    g = gray.astype(np.int64)
    rows = g[:, x0] * a0 + g[:, x1] * a1
    r0, r1 = rows[y0], rows[y1]
    out = (((b0[:, None] * (r0 >> 4)) >> 16) + ((b1[:, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def preprocess(img_bgr, scale=0.1):
    return resize_linear_u8(bgr_to_gray(img_bgr), scale)


# ----------------------------------------------------------------------------- 2. mask
def make_mask(h, w, dets, scale=0.1):
    """(h, w) of the small image; dets (n, >=4) full-resolution x1, y1, x2, y2."""
    m = np.zeros((h, w), np.uint8)
    m[int(0.02 * h):int(0.98 * h), int(0.02 * w):int(0.98 * w)] = 255
    if dets is not None:
        for d in np.asarray(dets, np.float64).reshape(-1, np.shape(dets)[-1] if np.size(dets) else 4):
            x1, y1, x2, y2 = (int(v * scale) for v in d[:4])
            x1, x2 = min(max(x1, 0), w), min(max(x2, 0), w)
            y1, y2 = min(max(y1, 0), h), min(max(y2, 0), h)
            m[y1:y2, x1:x2] = 0
    return m


# ----------------------------------------------------------------------------- 3. SIFT
def gaussian_kernel(sigma):
    """cv2.getGaussianKernel for a float image with ksize 0: ksize = round(8 sigma + 1) | 1."""
    k = int(np.rint(sigma * 8 + 1)) | 1
    r = (k - 1) // 2
    w = [float(np.exp(-(float(i - r) * float(i - r)) / (2.0 * sigma * sigma))) for i in range(k)]
    s = 0.0
    for v in w:
        s += v
    return np.array([v / s for v in w], np.float64)


def _reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    m = 2 * n - 2
    i = np.mod(i, m)
    return np.where(i >= n, m - i, i)


def blur(img, sigma, dtype=f32):
    """Separable Gaussian, BORDER_REFLECT_101, rows first; taps accumulated in ascending order."""
    k = gaussian_kernel(sigma).astype(f32).astype(dtype)  # the kernels hold float32 coefficients
    r = (len(k) - 1) // 2
    h, w = img.shape
    xi = [_reflect101(np.arange(w) + t - r, w) for t in range(len(k))]
    acc = k[0] * img[:, xi[0]]
    for t in range(1, len(k)):
        acc = acc + k[t] * img[:, xi[t]]
    yi = [_reflect101(np.arange(h) + t - r, h) for t in range(len(k))]
    out = k[0] * acc[yi[0]]
    for t in range(1, len(k)):
        out = out + k[t] * acc[yi[t]]
    return out.astype(dtype)


def upsample2(img, dtype=f32):
    """cv2.resize(2x, INTER_LINEAR) of a float image."""
    h, w = img.shape

    def taps(src, dst):
        d = np.arange(dst, dtype=np.float64)
        fx = ((d + 0.5) * 0.5 - 0.5).astype(f32)
        sx = np.floor(fx).astype(np.int64)
        fx = fx - sx.astype(f32)
        lo = sx < 0
        fx[lo], sx[lo] = 0, 0
        hi = sx >= src - 1
        fx[hi], sx[hi] = 0, src - 1
        return sx, np.minimum(sx + 1, src - 1), (f32(1) - fx).astype(dtype), fx.astype(dtype)

    x0, x1, a0, a1 = taps(w, 2 * w)
    y0, y1, b0, b1 = taps(h, 2 * h)
    rows = img[:, x0] * a0 + img[:, x1] * a1
    return (rows[y0] * b0[:, None] + rows[y1] * b1[:, None]).astype(dtype)


def layer_sigmas():
    k = 2.0 ** (1.0 / N_LAYERS)
    sig = [SIGMA]
    for i in range(1, N_LAYERS + 3):
        prev = SIGMA * k ** (i - 1)
        sig.append(float(np.sqrt((prev * k) ** 2 - prev ** 2)))
    return sig


def octave_shapes(h, w, first_octave):
    bh, bw = (2 * h, 2 * w) if first_octave < 0 else (h, w)
    n = int(np.rint(np.log(float(min(bh, bw))) / np.log(2.0) - 2)) - first_octave
    n = max(1, min(n, MAX_OCT))
    shapes = []
    for _ in range(n):
        if min(bh, bw) < 2 * BORDER + 1 and shapes:
            break
        shapes.append((bh, bw))
        bh, bw = bh // 2, bw // 2
    return shapes


def build_pyramid(gray, first_octave=-1, dtype=f32):
    """-> (gauss, dog): per octave arrays (6, h, w) and (5, h, w)."""
    img = gray.astype(dtype)
    if first_octave < 0:
        base = blur(upsample2(img, dtype), float(np.sqrt(max(SIGMA * SIGMA - 4 * 0.25, 0.01))), dtype)
    else:
        base = blur(img, float(np.sqrt(max(SIGMA * SIGMA - 0.25, 0.01))), dtype)
    sig = layer_sigmas()
    gauss, dog = [], []
    for o, (oh, ow) in enumerate(octave_shapes(gray.shape[0], gray.shape[1], first_octave)):
        g = np.empty((N_LAYERS + 3, oh, ow), dtype)
        g[0] = base if o == 0 else gauss[-1][N_LAYERS][0:2 * oh:2, 0:2 * ow:2]
        for i in range(1, N_LAYERS + 3):
            g[i] = blur(g[i - 1], sig[i], dtype)
        gauss.append(g)
        dog.append((g[1:] - g[:-1]).astype(dtype))
    return gauss, dog


def dog_precision(gray, first_octave=-1):
    """Largest |float32 - float64| deviation of the restatement's own DoG pyramid."""
    _, d32 = build_pyramid(gray, first_octave, f32)
    _, d64 = build_pyramid(gray, first_octave, np.float64)
    return max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(d32, d64))


def find_extrema(dog_o):
    """(layer, r, c) of the 26-neighbour extrema of one octave (|v| > 0, ties pass), scan order."""
    nl, h, w = dog_o.shape
    if h < 2 * BORDER + 1 or w < 2 * BORDER + 1:
        return np.zeros((0, 3), np.int64), np.zeros(0)
    thr = f32(PREFILTER)
    out, gaps = [], []
    for layer in range(1, N_LAYERS + 1):
        v = dog_o[layer, BORDER:h - BORDER, BORDER:w - BORDER]
        nmax = np.full(v.shape, -np.inf, dog_o.dtype)
        nmin = np.full(v.shape, np.inf, dog_o.dtype)
        for dl in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dl == 0 and dy == 0 and dx == 0:
                        continue
                    nb = dog_o[layer + dl, BORDER + dy:h - BORDER + dy, BORDER + dx:w - BORDER + dx]
                    nmax = np.maximum(nmax, nb)
                    nmin = np.minimum(nmin, nb)
        ok = (np.abs(v) > thr) & (((v > 0) & (v >= nmax)) | ((v < 0) & (v <= nmin)))
        rr, cc = np.nonzero(ok)
        gap = np.minimum(np.where(v > 0, v - nmax, nmin - v), np.abs(v) - thr)
        out.append(np.stack([np.full(len(rr), layer), rr + BORDER, cc + BORDER], 1))
        gaps.append(gap[rr, cc])
    return np.concatenate(out), np.concatenate(gaps)


class _Margin:
    """Smallest slack of the discrete decisions behind one keypoint, in DoG intensity units.  Slacks that are
    not intensities are converted by first-order sensitivity: an offset slack (px) by the smallest curvature
    times 255, the edge test by the gradient of 441 det - 20 tr^2 in the second derivatives (each a sum of four
    DoG samples / 255), an orientation-histogram slack by the sample weight that enters the bins compared."""

    def __init__(self):
        self.v, self.kind = np.inf, ""

    def add(self, slack, kind=""):
        if abs(float(slack)) < self.v:
            self.v, self.kind = abs(float(slack)), kind


def _refine(dog_o, layer, r, c, mg):
    """cv2 adjustLocalExtrema in float32.  -> None or (layer, r, c, xc, xr, xi, contr, curv)."""
    nl, h, w = dog_o.shape
    img_scale = f32(1.0) / f32(255.0)
    deriv = img_scale * f32(0.5)
    cross = img_scale * f32(0.25)
    xc = xr = xi = f32(0)
    for it in range(5):
        p, m, n = dog_o[layer - 1], dog_o[layer], dog_o[layer + 1]
        g0 = (m[r, c + 1] - m[r, c - 1]) * deriv
        g1 = (m[r + 1, c] - m[r - 1, c]) * deriv
        g2 = (n[r, c] - p[r, c]) * deriv
        v2 = m[r, c] * f32(2)
        dxx = (m[r, c + 1] + m[r, c - 1] - v2) * img_scale
        dyy = (m[r + 1, c] + m[r - 1, c] - v2) * img_scale
        dss = (n[r, c] + p[r, c] - v2) * img_scale
        dxy = (m[r + 1, c + 1] - m[r + 1, c - 1] - m[r - 1, c + 1] + m[r - 1, c - 1]) * cross
        dxs = (n[r, c + 1] - n[r, c - 1] - p[r, c + 1] + p[r, c - 1]) * cross
        dys = (n[r + 1, c] - n[r - 1, c] - p[r + 1, c] + p[r - 1, c]) * cross
        c00 = dyy * dss - dys * dys
        c01 = dxs * dys - dxy * dss
        c02 = dxy * dys - dxs * dyy
        det = dxx * c00 + dxy * c01 + dxs * c02
        if not (det != 0) or not np.isfinite(det):
            return None
        c11 = dxx * dss - dxs * dxs
        c12 = dxy * dxs - dxx * dys
        c22 = dxx * dyy - dxy * dxy
        xc = -((c00 * g0 + c01 * g1 + c02 * g2) / det)
        xr = -((c01 * g0 + c11 * g1 + c12 * g2) / det)
        xi = -((c02 * g0 + c12 * g1 + c22 * g2) / det)
        if not (np.isfinite(xc) and np.isfinite(xr) and np.isfinite(xi)):
            return None
        curv = min(abs(float(dxx)), abs(float(dyy)), abs(float(dss))) * 255.0
        for x in (xc, xr, xi):
            mg.add((abs(float(x)) - 0.5) * curv, 'offset')
        if abs(xi) < 0.5 and abs(xr) < 0.5 and abs(xc) < 0.5:
            break
        if max(abs(xi), abs(xr), abs(xc)) > 2147483647 / 3:
            return None
        c += int(np.rint(xc))
        r += int(np.rint(xr))
        layer += int(np.rint(xi))
        if layer < 1 or layer > N_LAYERS or c < BORDER or c >= w - BORDER or r < BORDER or r >= h - BORDER:
            return None
    else:
        return None
    t = g0 * xc + g1 * xr + g2 * xi
    contr = m[r, c] * img_scale + t * f32(0.5)
    if abs(contr) * f32(N_LAYERS) < f32(CONTRAST):
        return None
    mg.add((abs(float(contr)) * N_LAYERS - CONTRAST) / N_LAYERS * 255.0, 'contrast')
    tr = dxx + dyy
    det2 = dxx * dyy - dxy * dxy
    e = f32(EDGE)
    lhs = tr * tr * e
    rhs = (e + f32(1)) * (e + f32(1)) * det2
    if det2 <= 0 or lhs >= rhs:
        return None
    sens = 441.0 * (abs(float(dxx)) + abs(float(dyy)) + 2 * abs(float(dxy))) + 80.0 * abs(float(tr))
    mg.add(min(float(rhs - lhs), 441.0 * float(det2)) / max(sens, 1e-30) * 255.0 / 4.0, 'edge')
    return layer, r, c, xc, xr, xi, abs(contr), curv


def _orientation_hist(img, r, c, radius, sigma):
    h, w = img.shape
    ii, jj = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    y, x = r + ii, c + jj
    ok = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    y, x, ii, jj = y[ok], x[ok], ii[ok], jj[ok]
    dx = img[y, x + 1] - img[y, x - 1]
    dy = img[y - 1, x] - img[y + 1, x]
    scale = f32(-1.0) / (f32(2.0) * sigma * sigma)
    wgt = np.exp((ii * ii + jj * jj).astype(f32) * scale)
    ori = np.arctan2(dy, dx) * f32(57.29577951308232)
    ori = np.where(ori < 0, ori + f32(360), ori)
    mag = np.sqrt(dx * dx + dy * dy)
    b = np.rint(f32(0.1) * ori).astype(np.int64)
    b = np.where(b >= 36, b - 36, b)
    b = np.where(b < 0, b + 36, b)
    q = np.rint((wgt * mag) * f32(FIX)).astype(np.int64)
    acc = np.zeros(36, np.int64)
    np.add.at(acc, b, q)
    t = acc.astype(f32) * f32(1.0 / FIX)
    hist = ((np.roll(t, 2) + np.roll(t, -2)) * f32(1.0 / 16) + (np.roll(t, 1) + np.roll(t, -1)) * f32(4.0 / 16)
            + t * f32(6.0 / 16))
    wb = np.bincount(b, weights=wgt.astype(np.float64), minlength=36)
    ws = (np.roll(wb, 2) + np.roll(wb, -2)) / 16 + (np.roll(wb, 1) + np.roll(wb, -1)) * 4 / 16 + wb * 6 / 16
    return hist.astype(f32), ws


def sift_detect(gray, first_octave=-1, mask=None, pyramid=None):
    """-> dict(kps (n, 7) float32 [x, y, size, angle, octave, layer, response], margin (n,), n_extrema,
    rejected (list of margins of candidates that a decision removed), gauss, dog)."""
    gauss, dog = pyramid if pyramid is not None else build_pyramid(gray, first_octave, f32)
    h, w = gray.shape
    cands = []
    for o, d in enumerate(dog):
        ex, gaps = find_extrema(d)
        cands += [(o, int(l), int(r), int(c), float(g)) for (l, r, c), g in zip(ex, gaps)]
    n_extrema = len(cands)
    cands = cands[:KCAND]
    rows, margins, rejected = [], [], []
    for o, layer, r, c, gap in cands:
        mg = _Margin()
        mg.add(gap, 'gap')
        res = _refine(dog[o], layer, r, c, mg)
        if res is None:
            rejected.append(mg.v)
            continue
        layer, r, c, xc, xr, xi, resp, curv = res
        osc = f32(2.0 ** o)
        x = (f32(c) + xc) * osc
        y = (f32(r) + xr) * osc
        size = f32(SIGMA) * np.exp2((f32(layer) + xi) / f32(N_LAYERS)) * osc * f32(2)
        scl = size * f32(0.5) / osc
        if first_octave < 0:
            x, y, size = x * f32(0.5), y * f32(0.5), size * f32(0.5)
        px, py = int(np.rint(x)), int(np.rint(y))
        if px < 0 or px >= w or py < 0 or py >= h:
            rejected.append(mg.v)
            continue
        if mask is not None:
            near = mask[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2]
            if (near == 0).any() != (near == 0).all():  # a mask edge within one pixel
                mg.add(min(abs(abs(float(x) - px) - 0.5), abs(abs(float(y) - py) - 0.5)) * curv, 'mask')
            if mask[py, px] == 0:
                rejected.append(mg.v)
                continue
        radius = min(int(np.rint(f32(3 * 1.5) * scl)), 64)
        hist, ws = _orientation_hist(gauss[o][layer], r, c, radius, f32(1.5) * scl)
        mx = hist.max()
        thr = mx * f32(0.8)
        npk = 0
        for j in range(36):
            hl, hr, hj = hist[(j - 1) % 36], hist[(j + 1) % 36], hist[j]
            is_pk = hj > hl and hj > hr
            # slack of each condition over the sample weight entering the bins it compares
            jm = int(np.argmax(hist))
            conds = [float(hj - thr) / max(ws[j] + 0.8 * ws[jm], 1e-30),
                     float(hj - hl) / max(ws[j] + ws[(j - 1) % 36], 1e-30),
                     float(hj - hr) / max(ws[j] + ws[(j + 1) % 36], 1e-30)]  # emitted iff all hold
            fails = [-v for v, ok in zip(conds, (hj >= thr, hj > hl, hj > hr)) if not ok]
            mg.add(max(fails) if fails else min(conds), 'ori')
            if is_pk and hj >= thr and npk < MAXPEAK:
                b = f32(j) + f32(0.5) * (hl - hr) / (hl - f32(2) * hj + hr)
                b = b + f32(36) if b < 0 else (b - f32(36) if b >= 36 else b)
                ang = f32(360) - f32(10) * b
                if abs(ang - f32(360)) < FLT_EPS:
                    ang = f32(0)
                rows.append([x, y, size, ang, f32(o + first_octave), f32(layer), resp])
                margins.append(mg)
                npk += 1
    kps = np.array(rows, f32).reshape(-1, 7)
    mv = np.array([m.v for m in margins])
    kinds = np.array([m.kind for m in margins])
    order = np.lexsort((kps[:, 3], kps[:, 0], kps[:, 1], kps[:, 5], kps[:, 4]))[:KMAX]
    return dict(kps=kps[order], margin=mv[order], kind=kinds[order], n_extrema=n_extrema, rejected=np.array(rejected), gauss=gauss,
                dog=dog)


def sift_describe(gray, kps, first_octave=-1, pyramid=None):
    """cv2 calcSIFTDescriptor (d = 4, n = 8) -> (n, 128) uint8."""
    gauss, _ = pyramid if pyramid is not None else build_pyramid(gray, first_octave, f32)
    out = np.zeros((len(kps), 128), np.uint8)
    d, n = 4, 8
    for k, kp in enumerate(np.asarray(kps, f32)):
        octave, layer = int(kp[4]), int(kp[5])
        sc = f32(2.0 ** (-octave))
        img = gauss[octave - first_octave][layer]
        rows, cols = img.shape
        ptx, pty, size = kp[0] * sc, kp[1] * sc, kp[2] * sc
        ang = f32(360) - kp[3]
        if abs(ang - f32(360)) < FLT_EPS:
            ang = f32(0)
        scl = size * f32(0.5)
        pc, pr = int(np.rint(ptx)), int(np.rint(pty))
        rad = ang * f32(np.pi / 180)
        cos_t, sin_t = np.cos(rad, dtype=f32), np.sin(rad, dtype=f32)
        hw = f32(3) * scl
        radius = int(np.rint(hw * f32(1.4142135623730951) * f32(2.5)))
        radius = min(radius, int(np.sqrt(float(cols * cols + rows * rows))))
        cos_t, sin_t = cos_t / hw, sin_t / hw
        ii, jj = np.mgrid[-radius:radius + 1, -radius:radius + 1]
        fi, fj = ii.astype(f32), jj.astype(f32)
        c_rot = fj * cos_t - fi * sin_t
        r_rot = fj * sin_t + fi * cos_t
        rbin = r_rot + f32(d // 2) - f32(0.5)
        cbin = c_rot + f32(d // 2) - f32(0.5)
        r, c = pr + ii, pc + jj
        ok = (rbin > -1) & (rbin < d) & (cbin > -1) & (cbin < d) & (r > 0) & (r < rows - 1) & (c > 0) & (c < cols - 1)
        r, c, rbin, cbin, c_rot, r_rot = r[ok], c[ok], rbin[ok], cbin[ok], c_rot[ok], r_rot[ok]
        dx = img[r, c + 1] - img[r, c - 1]
        dy = img[r - 1, c] - img[r + 1, c]
        wgt = np.exp((c_rot * c_rot + r_rot * r_rot) * f32(-0.125))
        ori = np.arctan2(dy, dx) * f32(57.29577951308232)
        ori = np.where(ori < 0, ori + f32(360), ori)
        mag = np.sqrt(dx * dx + dy * dy) * wgt
        obin = (ori - ang) * f32(n / 360.0)
        r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
        fr, fc, fo = rbin - r0, cbin - c0, obin - o0
        r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
        o0 = np.where(o0 < 0, o0 + n, o0)
        o0 = np.where(o0 >= n, o0 - n, o0)
        v_r1 = mag * fr
        v_r0 = mag - v_r1
        v_rc11 = v_r1 * fc
        v_rc10 = v_r1 - v_rc11
        v_rc01 = v_r0 * fc
        v_rc00 = v_r0 - v_rc01
        hist = np.zeros((d + 2) * (d + 2) * (n + 2), np.int64)
        idx = ((r0 + 1) * (d + 2) + c0 + 1) * (n + 2) + o0
        for v, off in ((v_rc00, 0), (v_rc01, n + 2), (v_rc10, (d + 2) * (n + 2)), (v_rc11, (d + 3) * (n + 2))):
            v1 = v * fo
            v0 = v - v1
            np.add.at(hist, idx + off, np.rint(v0 * f32(FIX)).astype(np.int64))
            np.add.at(hist, idx + off + 1, np.rint(v1 * f32(FIX)).astype(np.int64))
        hist = hist.reshape(d + 2, d + 2, n + 2)
        hist[:, :, 0] += hist[:, :, n]
        hist[:, :, 1] += hist[:, :, n + 1]
        dst = hist[1:d + 1, 1:d + 1, :n].reshape(-1).astype(f32) * f32(1.0 / FIX)
        nrm2 = np.sum(dst * dst, dtype=f32)
        thr = np.sqrt(nrm2) * f32(0.2)
        dst = np.minimum(dst, thr)
        nrm2 = np.sum(dst * dst, dtype=f32)
        s = f32(512) / max(np.sqrt(nrm2), FLT_EPS)
        out[k] = np.clip(np.rint(dst * s), 0, 255).astype(np.uint8)
    return out


# ----------------------------------------------------------------------------- 4. match
def match_knn2(query, train):
    """-> idx (nq, 2) int32 (-1 = absent), dist (nq, 2) int32 squared L2; equal distance: lower index first."""
    q = np.asarray(query, np.int64).reshape(-1, 128)
    t = np.asarray(train, np.int64).reshape(-1, 128)
    idx = np.full((len(q), 2), -1, np.int32)
    dist = np.full((len(q), 2), -1, np.int32)
    if len(q) == 0 or len(t) == 0:
        return idx, dist
    d = (q * q).sum(1)[:, None] + (t * t).sum(1)[None] - 2 * (q @ t.T)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]
    for k in range(min(2, len(t))):
        idx[:, k] = order[:, k]
        dist[:, k] = np.take_along_axis(d, order[:, k:k + 1], 1)[:, 0]
    return idx, dist


def ratio_ok(d1_sq, d2_sq):
    """m.distance < 0.9 n.distance on the exact squares: 100 d1^2 < 81 d2^2."""
    return 100 * np.asarray(d1_sq, np.int64) < 81 * np.asarray(d2_sq, np.int64)


def filter_matches(idx, dist, prev_xy, cur_xy, h, w):
    """boxmot's gates.  -> (prev (n, 2), cur (n, 2)) float64 of the good matches, n_knn."""
    pp, cc = [], []
    for qi in range(len(idx)):
        if idx[qi, 1] < 0 or not ratio_ok(dist[qi, 0], dist[qi, 1]):
            continue
        p = np.asarray(prev_xy[qi], np.float64)
        c = np.asarray(cur_xy[idx[qi, 0]], np.float64)
        if abs(p[0] - c[0]) < 0.25 * w and abs(p[1] - c[1]) < 0.25 * h:
            pp.append(p)
            cc.append(c)
    n_knn = len(pp)
    if n_knn == 0:
        return np.zeros((0, 2)), np.zeros((0, 2)), 0
    pp, cc = np.array(pp), np.array(cc)
    sp = pp - cc
    keep = np.ones(n_knn, bool)
    for a in range(2):
        s = 0.0
        for v in sp[:, a]:
            s += v
        mean = s / n_knn
        s2 = 0.0
        for v in sp[:, a]:
            s2 += (v - mean) * (v - mean)
        std = np.sqrt(s2 / n_knn)
        keep &= (sp[:, a] - mean) < 2.5 * std
    return pp[keep], cc[keep], n_knn


# ----------------------------------------------------------------------------- 5. partial affine
def _hash32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


MAX_HYP = 2000


def ransac_pairs(n):
    if n * (n - 1) // 2 <= MAX_HYP:
        return [(i, j) for i in range(n) for j in range(i + 1, n)]
    out = []
    for k in range(MAX_HYP):
        i = _hash32(2 * k) % n
        out.append((i, (i + 1 + _hash32(2 * k + 1) % (n - 1)) % n))
    return out


def affine_partial_ransac(src, dst, thresh=3.0):
    """-> dict(warp (2, 3) float64 mapping src -> dst, hyp, n_inliers, mask)."""
    src = np.asarray(src, np.float64).reshape(-1, 2)
    dst = np.asarray(dst, np.float64).reshape(-1, 2)
    n = len(src)
    ident = dict(warp=np.eye(2, 3), hyp=-1, n_inliers=0, mask=np.zeros(n, bool))
    if n <= 4:
        return ident
    best, best_h, best_mask = 0, -1, None
    px, py, qx, qy = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
    for hi, (i, j) in enumerate(ransac_pairs(n)):
        dpx, dpy = px[j] - px[i], py[j] - py[i]
        dqx, dqy = qx[j] - qx[i], qy[j] - qy[i]
        den = dpx * dpx + dpy * dpy
        if not den > 0:
            continue
        a = (dqx * dpx + dqy * dpy) / den
        b = (dqy * dpx - dqx * dpy) / den
        tx = qx[i] - (a * px[i] - b * py[i])
        ty = qy[i] - (b * px[i] + a * py[i])
        ex = a * px - b * py + tx - qx
        ey = b * px + a * py + ty - qy
        m = ex * ex + ey * ey < thresh * thresh
        cnt = int(m.sum())
        if cnt > best:
            best, best_h, best_mask = cnt, hi, m
    if best < 2:
        return ident
    sx = sy = ux = uy = 0.0
    for k in np.nonzero(best_mask)[0]:
        sx += px[k]
        sy += py[k]
        ux += qx[k]
        uy += qy[k]
    sx, sy, ux, uy = sx / best, sy / best, ux / best, uy / best
    num_a = num_b = den = 0.0
    for k in np.nonzero(best_mask)[0]:
        x, y, u, v = px[k] - sx, py[k] - sy, qx[k] - ux, qy[k] - uy
        num_a += x * u + y * v
        num_b += x * v - y * u
        den += x * x + y * y
    if not den > 0:
        return ident
    a, b = num_a / den, num_b / den
    tx = ux - (a * sx - b * sy)
    ty = uy - (b * sx + a * sy)
    return dict(warp=np.array([[a, -b, tx], [b, a, ty]]), hyp=best_h, n_inliers=best, mask=best_mask)


# ----------------------------------------------------------------------------- SIFT.apply
class SiftCmcRef:
    """boxmot SIFT.apply: warp maps previous-frame to current-frame coordinates (full resolution)."""

    def __init__(self, scale=0.1, first_octave=-1):
        self.scale, self.first_octave = scale, first_octave
        self.prev = None
        self.stats = dict(n_kp=0, n_knn=0, n_good=0, n_inliers=0)

    def apply(self, img, dets=None):
        small = preprocess(img, self.scale)
        h, w = small.shape
        mask = make_mask(h, w, dets, self.scale)
        pyr = build_pyramid(small, self.first_octave)
        det = sift_detect(small, self.first_octave, mask, pyr)
        kps = det["kps"]
        desc = sift_describe(small, kps, self.first_octave, pyr)
        prev, self.prev = self.prev, (kps, desc)
        self.stats = dict(n_kp=len(kps), n_knn=0, n_good=0, n_inliers=0)
        warp = np.eye(2, 3)
        if prev is None or len(kps) == 0 or len(prev[0]) == 0:
            return warp
        idx, dist = match_knn2(prev[1], desc)
        pp, cc, n_knn = filter_matches(idx, dist, prev[0][:, :2], kps[:, :2], h, w)
        self.stats.update(n_knn=n_knn, n_good=len(pp))
        if len(pp) > 4:
            res = affine_partial_ransac(pp, cc)
            self.stats["n_inliers"] = res["n_inliers"]
            warp = res["warp"].copy()
            warp[0, 2] /= self.scale
            warp[1, 2] /= self.scale
        return warp


# ----------------------------------------------------------------------------- synthetic frames
def blob_field(seed=7, n=1500, height=1536, width=2048):
    rng = np.random.default_rng(seed)
    cx = rng.uniform(-200, width + 200, n)
    cy = rng.uniform(-200, height + 200, n)
    sig = rng.uniform(12, 45, n)
    amp = rng.uniform(-1, 1, n)
    return np.stack([cx, cy, sig, amp], 1)


def similarity(rot_deg=0.5, scale=1.01, t=(93.0, -41.0)):
    a = np.deg2rad(rot_deg)
    return np.array([[scale * np.cos(a), -scale * np.sin(a), t[0]], [scale * np.sin(a), scale * np.cos(a), t[1]]])


def render_blobs(blobs, height=1536, width=2048, warp=None):
    """clip(rint(128 + 40 sum of Gaussians)) replicated to 3 channels; ``warp`` moves the blobs analytically
    (centres A c + t, sigma sqrt(det A)), no image interpolation."""
    b = np.array(blobs, np.float64)
    if warp is not None:
        A, t = warp[:, :2], warp[:, 2]
        b[:, :2] = b[:, :2] @ A.T + t
        b[:, 2] *= np.sqrt(abs(np.linalg.det(A)))
    acc = np.zeros((height, width))
    for cx, cy, s, a in b:
        r = 4.5 * s
        x0, x1 = max(int(np.floor(cx - r)), 0), min(int(np.ceil(cx + r)) + 1, width)
        y0, y1 = max(int(np.floor(cy - r)), 0), min(int(np.ceil(cy + r)) + 1, height)
        if x0 >= x1 or y0 >= y1:
            continue
        gx = np.exp(-(np.arange(x0, x1) - cx) ** 2 / (2 * s * s))
        gy = np.exp(-(np.arange(y0, y1) - cy) ** 2 / (2 * s * s))
        acc[y0:y1, x0:x1] += a * np.outer(gy, gx)
    img = np.clip(np.rint(128 + 40 * acc), 0, 255).astype(np.uint8)
    return np.repeat(img[:, :, None], 3, 2)


def corner_error(warp, truth, height=1536, width=2048):
    """Largest displacement error over the four frame corners, full-resolution px."""
    c = np.array([[0, 0, 1], [width, 0, 1], [0, height, 1], [width, height, 1]], np.float64)
    return float(np.linalg.norm(c @ np.asarray(warp).T - c @ np.asarray(truth).T, axis=1).max())


_CACHE = {}


def standard_pair():
    """The shared frame pair: blob field seed 7 and its re-render under rotation 0.5 deg, scale 1.01,
    t = (93, -41) px.  -> (frame0, frame1, truth 2x3).  Rendered once per process."""
    if "pair" not in _CACHE:
        blobs, truth = blob_field(), similarity()
        _CACHE["pair"] = (render_blobs(blobs), render_blobs(blobs, warp=truth), truth)
    return _CACHE["pair"]


def six_blob_image():
    """256 x 256 uint8 with six isolated Gaussian blobs centred on multiples of 4, >= 64 px apart."""
    centres = [(48, 48), (128, 52), (204, 48), (52, 156), (128, 180), (200, 200)]
    yy, xx = np.mgrid[0:256, 0:256].astype(np.float64)
    acc = np.zeros((256, 256))
    for cx, cy in centres:
        acc += np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * 5.0 ** 2))
    return np.clip(np.rint(20 + 60 * acc), 0, 255).astype(np.uint8), centres
