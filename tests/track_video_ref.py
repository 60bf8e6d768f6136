"""NumPy restatement of what step 3's tracking video adds to the pose overlay (csrc/overlay.hip's labelled kernels,
csrc/resize.hip): the label origin of step3_crossframematching.py visualize :1658-1666, this project's exact
integer capsule rule for the label strokes, the colour table (:1642-1646) and the 8-bit fixed-point bilinear resize
(:1685).  Discs, limbs and the projection come from overlay_ref; the JPEG encoder of the video from jpeg_ref.

  label segment p0 -> p1 (origin added), thickness t, Python integers: e = p1 - p0, w = X - p0
    w.e <= 0: 4|w|^2 <= t^2;   w.e >= |e|^2: 4|X - p1|^2 <= t^2;   else 4 (w x e)^2 <= t^2 |e|^2
  resize, per axis with scale = src / dst in float64:
    f = float32((d + 0.5) * scale - 0.5); s = floor(f); f -= s; s < 0: s = 0, f = 0; s >= src - 1: s = src - 1, f = 0
    taps s, min(s + 1, src - 1); c1 = rint(f * 2048f), c0 = rint((1f - f) * 2048f) in float32
    R = I[s] * a0 + I[s1] * a1;  out = (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2, saturated
"""
import numpy as np

import jpeg_ref  # noqa: F401  (the video's encoder: tests build the oracle chain from this module alone)
import overlay_ref
from overlay_ref import COLOURS, make_cam

MAX_LABEL_COORD = 8192


def colour_of_index(c):
    """The colour table's rule: 0..3 are the four colours, anything else (step 3's Cid = -1) is black."""
    c = int(c)
    return COLOURS[c] if 0 <= c < 4 else (0, 0, 0)


# ------------------------------------------------------------------------------------------------ labels
def label_origin(p):
    """``p`` (J + 1, 2) reprojected slots -> (x, y) integers or None (visualize :1658-1667)."""
    out = []
    for axis in (0, 1):
        v = p[:, axis]
        v = v[~np.isnan(v)]
        if len(v) == 0:
            return None
        m = v.min()
        if m > 3000 or m < -1000:
            return None
        out.append(int(m))          # truncates toward zero
    return tuple(out)


def label_slot(cam, x3, seg, n, t):
    """The label's primitive slot [valid, ox, oy, 0, x0, y0, x1, y1] of one animal: ``seg`` (S, 4), ``n`` in use."""
    x = np.concatenate([x3, ((x3[5, :] + x3[6, :]) / 2)[None, :]], axis=0)
    org = label_origin(cam.project(x))
    n = min(max(int(n), 0), len(seg))
    row = np.zeros(8, dtype=np.int32)
    if org is None or n == 0:
        return row
    g = np.asarray(seg[:n], dtype=np.int64)
    x0, y0 = min(g[:, 0].min(), g[:, 2].min()), min(g[:, 1].min(), g[:, 3].min())
    x1, y1 = max(g[:, 0].max(), g[:, 2].max()), max(g[:, 1].max(), g[:, 3].max())
    if min(x0, y0) < -MAX_LABEL_COORD or max(x1, y1) > MAX_LABEL_COORD:
        return row
    pad = (int(t) + 1) // 2
    row[:] = [1, org[0], org[1], 0, org[0] + x0 - pad, org[1] + y0 - pad, org[0] + x1 + pad, org[1] + y1 + pad]
    return row


def capsule_mask(p0, p1, t, xs, ys):
    """Coverage of the stroke p0 -> p1 of thickness ``t`` on columns ``xs`` and rows ``ys``: (len(ys), len(xs)).
    Python integers throughout (object arrays), so nothing can overflow."""
    X = np.asarray(xs, dtype=object)[None, :] + np.zeros((len(ys), 1), dtype=object)
    Y = np.asarray(ys, dtype=object)[:, None] + np.zeros((1, len(xs)), dtype=object)
    ex, ey = int(p1[0]) - int(p0[0]), int(p1[1]) - int(p0[1])
    wx, wy = X - int(p0[0]), Y - int(p0[1])
    vx, vy = X - int(p1[0]), Y - int(p1[1])
    we, ee, t2 = wx * ex + wy * ey, ex * ex + ey * ey, int(t) * int(t)
    cr = wx * ey - wy * ex
    head = 4 * (wx * wx + wy * wy) <= t2
    tail = 4 * (vx * vx + vy * vy) <= t2
    body = 4 * cr * cr <= t2 * ee
    return np.where(we <= 0, head, np.where(we >= ee, tail, body)).astype(bool)


def label_mask(slot, seg, n, t, xs, ys):
    """Union of the label's strokes on the pixel grid ``xs`` x ``ys``."""
    m = np.zeros((len(ys), len(xs)), dtype=bool)
    ox, oy = int(slot[1]), int(slot[2])
    pad = (int(t) + 1) // 2
    for x0, y0, x1, y1 in np.asarray(seg[:min(max(int(n), 0), len(seg))], dtype=np.int64):
        ax, ay, bx, by = ox + int(x0), oy + int(y0), ox + int(x1), oy + int(y1)
        ix = np.nonzero((xs >= min(ax, bx) - pad) & (xs <= max(ax, bx) + pad))[0]
        iy = np.nonzero((ys >= min(ay, by) - pad) & (ys <= max(ay, by) + pad))[0]
        if len(ix) and len(iy):
            m[np.ix_(iy, ix)] |= capsule_mask((ax, ay), (bx, by), t, xs[ix], ys[iy])
    return m


def primitives(cam_dicts, cam_of_img, kp3d, score, pairs, radius, flags, mrksize, seg, n, t):
    """overlay_ref.primitives with the label slot appended: prim_i (B, A, J + 2 + P, 8), prim_d (B, A, P, 4).
    ``seg`` (B, A, S, 4) / ``n`` (B, A), or None for no labels."""
    cams = [make_cam(d) for d in cam_dicts]
    base_i, prim_d = overlay_ref.primitives(cam_dicts, cam_of_img, kp3d, score, pairs, radius, flags, mrksize)
    B, A = kp3d.shape[:2]
    prim_i = np.zeros((B, A, base_i.shape[2] + 1, 8), dtype=np.int32)
    prim_i[:, :, :-1] = base_i
    if seg is not None:
        for b in range(B):
            for a in range(A):
                prim_i[b, a, -1] = label_slot(cams[int(cam_of_img[b])], kp3d[b, a], seg[b, a], n[b, a], t)
    return prim_i, prim_d


def draw_image(img, prim_i, prim_d, n_joints, mrksize, colour, seg, n, t):
    """One image: animals in index order, each animal's discs and limbs and then its label, in colour
    ``colour[a]`` (None: the animal index), clipped to the image."""
    out = np.array(img, dtype=np.uint8, copy=True)
    H, W = out.shape[:2]
    for a in range(prim_i.shape[0]):
        clr = colour_of_index(a if colour is None else colour[a])
        for k in range(prim_i.shape[1]):
            valid, cx, cy, r, x0, y0, x1, y1 = (int(v) for v in prim_i[a, k])
            if not valid:
                continue
            x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
            if x0 > x1 or y0 > y1:
                continue
            xs, ys = np.arange(x0, x1 + 1), np.arange(y0, y1 + 1)
            if k == prim_i.shape[1] - 1:
                m = label_mask(prim_i[a, k], seg[a], n[a], t, xs, ys)
            elif k <= n_joints:
                m = overlay_ref.disc_mask(cx, cy, r, xs, ys)
            else:
                m = overlay_ref.limb_mask(*prim_d[a, k - n_joints - 1], mrksize, xs, ys)
            out[y0:y1 + 1, x0:x1 + 1][m] = clr
    return out


def render(frames, cam_dicts, cam_of_img, kp3d, score, pairs, radius, flags, mrksize=3, src_index=None, colour=None,
           seg=None, n=None, t=5):
    """The labelled stage for B outputs: (B, H, W, 3) uint8; any number of animals (one painter's-order pass)."""
    B, A, J, _ = kp3d.shape
    src = np.arange(B) if src_index is None else np.asarray(src_index)
    prim_i, prim_d = primitives(cam_dicts, cam_of_img, kp3d, score, pairs, radius, flags, mrksize, seg, n, t)
    if seg is None:
        seg, n = np.zeros((B, A, 1, 4), dtype=np.int32), np.zeros((B, A), dtype=np.int32)
    return np.stack([draw_image(frames[int(src[b])], prim_i[b], prim_d[b], J, mrksize,
                                None if colour is None else colour[b], seg[b], n[b], t) for b in range(B)])


# ------------------------------------------------------------------------------------------------ resize
def resize_taps(src, dst):
    """(s0, s1, c0, c1, f) per destination index of one axis; ``f`` is the float32 fraction after clamping."""
    scale = np.float64(src) / np.float64(dst)
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    fl = np.floor(f)
    s = fl.astype(np.int64)
    f = f - fl
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    c1 = np.rint(f * np.float32(2048)).astype(np.int64)
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, src - 1), c0, c1, f


def resize_bilinear(frames, height, width):
    """uint8 (n, H, W, 3) or (H, W, 3) -> the same rank at (height, width), the fixed-point rule."""
    a = np.asarray(frames)
    single = a.ndim == 3
    a = (a[None] if single else a).astype(np.int64)
    y0, y1, b0, b1, _ = resize_taps(a.shape[1], height)
    x0, x1, a0, a1, _ = resize_taps(a.shape[2], width)
    R = a[:, :, x0] * a0[None, None, :, None] + a[:, :, x1] * a1[None, None, :, None]      # (n, H, w, 3)
    R0, R1 = R[:, y0] >> 4, R[:, y1] >> 4
    out = (((b0[None, :, None, None] * R0) >> 16) + ((b1[None, :, None, None] * R1) >> 16) + 2) >> 2
    out = np.clip(out, 0, 255).astype(np.uint8)
    return out[0] if single else out


def resize_float(frames, height, width):
    """float64 bilinear at the same sample positions (the taps and the float32 fractions of ``resize_taps``)."""
    a = np.asarray(frames)
    single = a.ndim == 3
    a = (a[None] if single else a).astype(np.float64)
    y0, y1, _, _, fy = resize_taps(a.shape[1], height)
    x0, x1, _, _, fx = resize_taps(a.shape[2], width)
    fx, fy = fx.astype(np.float64)[None, None, :, None], fy.astype(np.float64)[None, :, None, None]
    R = a[:, :, x0] * (1 - fx) + a[:, :, x1] * fx
    out = R[:, y0] * (1 - fy) + R[:, y1] * fy
    return out[0] if single else out


# ------------------------------------------------------------------------------------------------ factories
def oracle_renderer_factory(cam_dict, calls=None):
    """A ``renderer`` for step 3's ``visualize``: the NumPy composition in the camera ``cam_dict``.  ``calls``
    (a list) records (colour, labels) per render call."""
    from mqhip.overlay import SKELETONS, label_tables

    class _Renderer:
        def __init__(self, cgroup, height, width, skeleton, mrksize, device):
            self.sk, self.mrksize = SKELETONS[skeleton], mrksize

        def render(self, frames, cam_idx, kp3d, score, src_index=None, colour=None, labels=None, label_scale=2.0,
                   label_thickness=5):
            frames = frames.cpu().numpy() if hasattr(frames, "cpu") else np.asarray(frames)
            B, A = kp3d.shape[:2]
            if calls is not None:
                calls.append((None if colour is None else np.array(colour), labels))
            seg, n = label_tables(labels, B, A, label_scale, label_thickness) if labels is not None else (None, None)
            return render(frames, [cam_dict], np.zeros(B, dtype=int), kp3d, score, self.sk.pairs,
                          self.sk.radius(self.mrksize), self.sk.flags, self.mrksize, src_index, colour, seg, n,
                          label_thickness)

    return _Renderer


def oracle_resizer(frames, height, width, device=0):
    frames = frames.cpu().numpy() if hasattr(frames, "cpu") else np.asarray(frames)
    return resize_bilinear(frames, height, width)


# ------------------------------------------------------------------------------------------------ the video
SMALL_RECIPE = {"seed": 44, "n_frame": 62, "n_cam": 4, "n_animal": 3, "p_seen": 0.95, "p_dup": 0.05,
                "events": [["switch", 1, 0, 30], ["noid", 2], ["kf_drop", 2, 1]]}


def write_scene(root, recipe, height, width, vis_cam):
    """A step3_scenes scene scaled to ``height`` x ``width`` pixels and written where step 3 reads it: config.yaml,
    per camera alldata.json and frame_num.npy, match_keyframe.pickle, and camera ``vis_cam``'s frame store (a pool
    of two random images).  Returns a dict: cams, camparam, T, keyframes, cfg, rd (the result directory), raw."""
    import json
    import os
    import pickle

    import yaml

    import step3_scenes as scenes
    from mqhip import io as mqio
    from mqhip import synth
    cams, T, keyframes = scenes.build_scene(recipe)
    sx, sy = width / 2048.0, height / 1536.0
    for c in cams:
        c["K"] = np.asarray(c["K"], dtype=np.float64) * np.array([[sx], [sy], [1.0]])
    for cam in T:
        for rows in cam:
            for r in rows:
                r[1], r[2], r[3], r[4] = r[1] * sx, r[2] * sy, r[3] * sx, r[4] * sy
                r[5] = [[v[0] * sx, v[1] * sy, v[2]] for v in r[5]]
    F = recipe["n_frame"]
    rd = os.path.join(str(root), "results3D", "clip")
    raw = os.path.join(str(root), "videos")
    cfg = os.path.join(str(root), "config.yaml")
    os.makedirs(rd)
    with open(cfg, "w") as f:
        yaml.safe_dump({"camera_id": [int(c["name"]) for c in cams]}, f)
    numbers = 100 + np.arange(F)
    for c, cam in enumerate(cams):
        os.makedirs(os.path.join(rd, str(cam["name"])))
        with open(os.path.join(rd, str(cam["name"]), "alldata.json"), "w") as f:
            json.dump(T[c], f)
        np.save(os.path.join(rd, str(cam["name"]), "frame_num.npy"), numbers.astype(np.int32))
    with open(os.path.join(rd, "match_keyframe.pickle"), "wb") as f:
        pickle.dump(keyframes, f)
    pool = np.random.default_rng(recipe["seed"]).integers(0, 256, (2, height, width, 3), dtype=np.uint8)
    name = str(cams[vis_cam]["name"])
    mqio.write_frame_store(os.path.join(raw, f"clip.{name}"), pool, 10.0 + numbers / 24.0, numbers,
                           [[] for _ in numbers], name, frame_index=np.arange(F) % 2)
    return dict(cams=cams, camparam=synth.camparam_from_cams(cams), T=T, keyframes=keyframes, cfg=cfg, rd=rd, raw=raw,
                pool=pool, numbers=numbers)


class RecordingLift:
    """Wraps a lift (``TrackletLift`` or the oracle's) and keeps the joints it returned per (Trk position, frame)."""

    def __init__(self, inner):
        self.inner, self.p3d, self.calls = inner, {}, 0

    def traces(self, Trk, cells=None, return_p3d=False, **kw):
        out = self.inner.traces(Trk, cells=cells, return_p3d=return_p3d, **kw)
        self.calls += 1
        if return_p3d and cells is not None:
            for (i, f), p in zip(np.asarray(cells).reshape(-1, 2), out[2]):
                self.p3d[(int(i), int(f))] = np.array(p)
        return out


def oracle_video(cam_dict, pool, Trk, Cid, p3d, size, step=3, quality=90, n_joints=17):
    """The oracle chain of step 3's video for frame rows ``range(0, n_frame, step)`` (store image = row % 2 of
    ``pool``): every live tracklet in ``Trk``'s key order in ONE painter's-order pass, then the fixed-point resize
    to ``size`` = (width, height), then jpeg_ref.  ``p3d``: {(Trk position, frame): (J, 3)}.  Returns
    [(frame row, colour list, label list, JPEG bytes)]."""
    from mqhip.overlay import SKELETONS, label_tables
    sk = SKELETONS["v1"]
    keys = list(Trk.keys())
    out = []
    for f in range(0, Trk[keys[0]].shape[0], step):
        live = [i for i, k in enumerate(keys) if np.any(Trk[k][f] >= 0)]
        A = max(1, len(live))
        kp3d = np.full((1, A, n_joints, 3), np.nan)
        colour = np.full((1, A), -1, dtype=np.int32)
        labels = [[None] * A]
        for a, i in enumerate(live):
            kp3d[0, a], colour[0, a], labels[0][a] = p3d[(i, f)], int(Cid[keys[i]][f]), str(keys[i])
        seg, n = label_tables(labels, 1, A, 2.0, 5)
        img = render(pool[[f % 2]], [cam_dict], [0], kp3d, np.ones((1, A, n_joints)), sk.pairs, sk.radius(3), sk.flags,
                     3, None, colour, seg, n, 5)
        small = resize_bilinear(img, size[1], size[0])[0]
        out.append((f, colour[0, :len(live)].tolist(), [labels[0][a] for a in range(len(live))],
                    jpeg_ref.encode(small, quality, 16)[0]))
    return out
