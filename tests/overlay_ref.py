"""NumPy restatement of the pose overlay (csrc/overlay.hip): the reference's visualize_result.py proc :220-242,
clean_kp :30-51 (show_as_possible) and draw_kps :71-110, with this project's two exact coverage rules in place
of cv2.circle / cv2.ellipse.  Projection comes through oracle/geometry.py.  Coverage is evaluated inside each
primitive's bounding box only, so a full-size image takes well under a second.

  disc (cx, cy, r), integers:  (X - cx)^2 + (Y - cy)^2 <= r^2 + r
  limb (x1, y1)-(x2, y2), minor axis m, float64 in this order:
    ex = x2 - x1, ey = y2 - y1, d2 = ex*ex + ey*ey, cx = (x1 + x2)/2, cy = (y1 + y2)/2, px = X - cx, py = Y - cy,
    u = px*ex + py*ey, v = py*ex - px*ey, a2 = d2/4, b2 = m*m/4;  inside iff d2 > 0 and u*u*b2 + v*v*a2 <= a2*b2*d2
"""
import numpy as np

from oracle.geometry import make_cam

COLOURS = ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255))   # BGR; animals >= 4 are black
JOINT_DISC, JOINT_NULLED = 1, 2


def colour_of(animal):
    return COLOURS[animal] if animal < 4 else (0, 0, 0)


def disc_mask(cx, cy, r, xs, ys):
    """Coverage of the integer disc on the pixel columns ``xs`` and rows ``ys`` (int arrays): (len(ys), len(xs))."""
    dx = np.asarray(xs, dtype=np.int64)[None, :] - int(cx)
    dy = np.asarray(ys, dtype=np.int64)[:, None] - int(cy)
    return dx * dx + dy * dy <= r * r + r


def limb_mask(x1, y1, x2, y2, m, xs, ys):
    """Coverage of the limb ellipse (centre at the midpoint, full axes (d, m)) on columns ``xs`` and rows ``ys``."""
    x1, y1, x2, y2, m = (np.float64(t) for t in (x1, y1, x2, y2, m))
    ex, ey = x2 - x1, y2 - y1
    d2 = ex * ex + ey * ey
    cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
    px = np.asarray(xs, dtype=np.float64)[None, :] - cx
    py = np.asarray(ys, dtype=np.float64)[:, None] - cy
    u = px * ex + py * ey
    v = py * ex - px * ey
    a2, b2 = d2 / 4, m * m / 4
    inside = u * u * b2 + v * v * a2 <= a2 * b2 * d2
    return inside if d2 > 0 else np.zeros(inside.shape, dtype=bool)


def animal_primitives(cam, x3, s, pairs, radius, flags, mrksize):
    """One animal in one camera: ``x3`` (J, 3), ``s`` (J,) -> (prim_i (J + 1 + P, 8) int32, prim_d (P, 4) f64).
    proc :224-233 (neck, reprojection, the 0/1 flag), clean_kp :32-51, the geometry of draw_kps :100-110."""
    J, P = len(x3), len(pairs)
    x = np.concatenate([x3, ((x3[5, :] + x3[6, :]) / 2)[None, :]], axis=0)
    sc = np.concatenate([s, ((s[5] + s[6]) / 2)[None]], axis=0)
    p = cam.project(x)
    I = np.logical_and(np.logical_not(x[:, 0] == 0), sc > 0.0)
    cnt = int(np.count_nonzero(I.astype(np.float64) > 0.3))
    kp = []
    for j in range(J + 1):
        u, v = p[j]
        if flags[j] & JOINT_NULLED or cnt == 0 or np.isnan(u):
            kp.append(None)
        elif u > 3000 or u < -1000 or v > 3000 or v < -1000:
            kp.append(None)
        elif np.isnan(v):          # int(nan) raises in the reference; nothing is drawn
            kp.append(None)
        else:
            kp.append((u, v))
    prim_i = np.zeros((J + 1 + P, 8), dtype=np.int32)
    prim_d = np.zeros((P, 4), dtype=np.float64)
    for j in range(J + 1):
        if kp[j] is not None and flags[j] & JOINT_DISC:
            cx, cy, r = int(kp[j][0]), int(kp[j][1]), int(radius[j])
            prim_i[j] = [1, cx, cy, r, cx - r, cy - r, cx + r, cy + r]
    hm = np.float64(mrksize) / 2
    for k, (i1, i2) in enumerate(pairs):
        if kp[i1] is not None and kp[i2] is not None:
            (x1, y1), (x2, y2) = kp[i1], kp[i2]
            prim_d[k] = [x1, y1, x2, y2]
            prim_i[J + 1 + k] = [1, 0, 0, 0, int(np.floor(min(x1, x2) - hm)), int(np.floor(min(y1, y2) - hm)),
                                 int(np.ceil(max(x1, x2) + hm)), int(np.ceil(max(y1, y2) + hm))]
    return prim_i, prim_d


def primitives(cam_dicts, cam_of_img, kp3d, score, pairs, radius, flags, mrksize=3):
    """``kp3d`` (B, A, J, 3), ``score`` (B, A, J) -> prim_i (B, A, J + 1 + P, 8), prim_d (B, A, P, 4)."""
    cams = [make_cam(d) for d in cam_dicts]
    B, A, J, _ = kp3d.shape
    P = len(pairs)
    prim_i = np.zeros((B, A, J + 1 + P, 8), dtype=np.int32)
    prim_d = np.zeros((B, A, P, 4), dtype=np.float64)
    for b in range(B):
        for a in range(A):
            prim_i[b, a], prim_d[b, a] = animal_primitives(cams[int(cam_of_img[b])], kp3d[b, a], score[b, a], pairs,
                                                           radius, flags, mrksize)
    return prim_i, prim_d


def draw_image(img, prim_i, prim_d, n_joints, mrksize=3):
    """Draw one image's tables (A, J + 1 + P, 8) / (A, P, 4) over a copy of ``img`` (H, W, 3): animals in index
    order, each in its colour (the painter's order of proc :220-242), clipped to the image."""
    out = np.array(img, dtype=np.uint8, copy=True)
    H, W = out.shape[:2]
    for a in range(prim_i.shape[0]):
        clr = colour_of(a)
        for k in range(prim_i.shape[1]):
            valid, cx, cy, r, x0, y0, x1, y1 = (int(t) for t in prim_i[a, k])
            if not valid:
                continue
            x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
            if x0 > x1 or y0 > y1:
                continue
            xs, ys = np.arange(x0, x1 + 1), np.arange(y0, y1 + 1)
            if k <= n_joints:
                m = disc_mask(cx, cy, r, xs, ys)
            else:
                m = limb_mask(*prim_d[a, k - n_joints - 1], mrksize, xs, ys)
            out[y0:y1 + 1, x0:x1 + 1][m] = clr
    return out


def oracle_renderer_factory(calibration_toml, calls=None):
    """A ``renderer`` for ``visualize_result.proc``: the NumPy composition on the camera ``proc`` selected, read
    from the same calibration.toml.  ``calls`` (a list) records (number of pool images, src_index) per batch."""
    from mqhip import io as mqio
    from mqhip.overlay import SKELETONS
    cal = mqio.load_toml(calibration_toml)
    by_name = {str(d["name"]): d for k, d in cal.items() if k != "metadata"}

    class _Renderer:
        def __init__(self, cgroup, height, width, skeleton, mrksize, device):
            self.cam = by_name[str(cgroup.get_names()[0])]
            self.sk, self.mrksize = SKELETONS[skeleton], mrksize

        def render(self, frames, cam_idx, kp3d, score, src_index=None):
            if calls is not None:
                calls.append((len(frames), np.array(src_index)))
            B = kp3d.shape[0]
            return render(frames, [self.cam], np.zeros(B, dtype=int), kp3d, score, self.sk.pairs,
                          self.sk.radius(self.mrksize), self.sk.flags, self.mrksize, src_index)

    return _Renderer


def render(frames, cam_dicts, cam_of_img, kp3d, score, pairs, radius, flags, mrksize=3, src_index=None):
    """The whole stage for B outputs: (B, H, W, 3) uint8; output b is drawn over ``frames[src_index[b]]``."""
    B, _, J, _ = kp3d.shape
    src = np.arange(B) if src_index is None else np.asarray(src_index)
    prim_i, prim_d = primitives(cam_dicts, cam_of_img, kp3d, score, pairs, radius, flags, mrksize)
    return np.stack([draw_image(frames[int(src[b])], prim_i[b], prim_d[b], J, mrksize) for b in range(B)])
