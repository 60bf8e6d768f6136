"""Camera-motion compensation for step 1's BoT-SORT on MI355X: boxmot 12.0.7 ``cmc/sift.py`` ``SIFT.apply``
(``cmc_method='sift'``, step1_proc2d.py:88) restated stage by stage in ``csrc/cmc.hip`` -- cv2 gray + 0.1x resize,
the 2 % border / detection-box mask, SIFT detect + describe (nOctaveLayers 3, contrastThreshold 0.02,
edgeThreshold 20), brute-force 2-NN match with boxmot's ratio, spatial and 2.5 sigma gates, and the partial-affine
RANSAC (deterministic hypotheses instead of cv2's RNG).  Everything from the uint8 frame to the 2x3 warp runs on
the GPU; one copy of 6 doubles per image comes back.  There is no CPU fallback.  cv2 / boxmot parity is unpinned
(neither is installed); ``tests/cmc_ref.py`` is the numpy restatement the kernels are tested against.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

KMAX = 2048


class SiftCmc:
    """``SiftCmc(height, width).apply(img, dets)`` -> (2, 3) float64 warp from the previous frame's to this
    frame's coordinates: the ``cmc`` callable of ``mqhip.tracker.BotSort``.  ``n_slots`` cameras keep their
    previous frame on the device; ``apply_batch`` runs all cameras of a time step in one call."""

    def __init__(self, height, width, n_slots=1, scale=0.1, device=0, max_kp=KMAX):
        self._h = None
        self.ctx = _lib.Context.get(device)
        self.height, self.width, self.n_slots, self.scale, self.device = int(height), int(width), int(n_slots), scale, device
        h = C.c_void_p()
        _lib.check(self.ctx.lib.mq_cmc_create(self.ctx.handle, self.n_slots, self.height, self.width, float(scale),
                                              int(max_kp), C.byref(h)), "mq_cmc_create")
        self._h = h
        self.stats = [dict(n_kp=0, n_knn=0, n_good=0, n_inliers=0) for _ in range(self.n_slots)]

    def __del__(self):
        try:
            if self._h is not None:
                self.ctx.lib.mq_cmc_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def reset(self, slot=-1):
        """Forget the previous frame of ``slot`` (-1: of every slot)."""
        _lib.check(self.ctx.lib.mq_cmc_reset(self._h, int(slot)), "mq_cmc_reset")

    def _frames(self, frames):
        import torch
        if isinstance(frames, torch.Tensor):
            t = frames
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(frames, np.uint8)))
        if t.dim() == 3:
            t = t[None]
        if t.dtype != torch.uint8 or tuple(t.shape[1:]) != (self.height, self.width, 3):
            raise ValueError(f"SiftCmc: frames must be uint8 (n, {self.height}, {self.width}, 3), got "
                             f"{t.dtype} {tuple(t.shape)}")
        return t.to(f"cuda:{self.device}").contiguous()

    def apply_batch(self, frames, dets_per_image=None, slots=None):
        """frames (n, H, W, 3) uint8 BGR (numpy or device tensor); dets_per_image: per image None or (k, >= 4)
        boxes x1 y1 x2 y2 (masked out of the keypoint search); slots: the camera of each image (default
        0 .. n-1).  -> (n, 2, 3) float64."""
        import torch
        t = self._frames(frames)
        n = t.shape[0]
        slots = np.arange(n, dtype=np.int32) if slots is None else np.ascontiguousarray(slots, np.int32)
        if len(slots) != n:
            raise ValueError("SiftCmc: one slot per image")
        dets = [None] * n if dets_per_image is None else list(dets_per_image)
        dets = [np.zeros((0, 4)) if d is None or np.size(d) == 0 else np.asarray(d, np.float64).reshape(len(d), -1)[:, :4]
                for d in dets]
        mb = max(len(d) for d in dets)
        boxes = np.zeros((n, max(mb, 1), 4), np.float64)
        counts = np.zeros(n, np.int32)
        for i, d in enumerate(dets):
            boxes[i, :len(d)] = d
            counts[i] = len(d)
        warps = np.zeros((n, 6), np.float64)
        stats = np.zeros((n, 4), np.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.ctx.lib.mq_cmc_apply(self._h, _lib.ptr(t), int(t.stride(0)), n, slots.ctypes.data,
                                                 boxes.ctypes.data, counts.ctypes.data, int(mb), warps.ctypes.data,
                                                 stats.ctypes.data, _lib.stream_ptr(self.device)), "mq_cmc_apply")
        for i, s in enumerate(slots):
            self.stats[int(s)] = dict(zip(("n_kp", "n_knn", "n_good", "n_inliers"), (int(v) for v in stats[i])))
        return warps.reshape(n, 2, 3)

    def apply(self, img, dets=None, slot=0):
        return self.apply_batch(img, [dets], [slot])[0]

    __call__ = apply

    def for_slot(self, slot):
        """The ``cmc`` callable of one camera."""
        return lambda img, dets=None: self.apply(img, dets, slot)


# ----------------------------------------------------------------------------- stage entry points
def _dev(a, dtype, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(f"cuda:{device}")


def preprocess(frames, scale=0.1, device=0):
    """mq_cmc_preprocess: uint8 BGR (n, H, W, 3) -> uint8 gray (n, rint(H scale), rint(W scale))."""
    import torch
    ctx = _lib.Context.get(device)
    f = _dev(frames, np.uint8, device)
    n, H, W, _ = f.shape
    out = torch.zeros((n, int(np.rint(H * scale)), int(np.rint(W * scale))), dtype=torch.uint8, device=f.device)
    _lib.check(ctx.lib.mq_cmc_preprocess(ctx.handle, _lib.ptr(f), int(f.stride(0)), n, H, W, float(scale),
                                         _lib.ptr(out), _lib.stream_ptr(device)), "mq_cmc_preprocess")
    return out.cpu().numpy()


def dog_layout(h, w, first_octave=-1):
    """Octave shapes of the pyramid that mq_sift_detect builds for an (h, w) image."""
    bh, bw = (2 * h, 2 * w) if first_octave < 0 else (h, w)
    n = max(1, min(int(np.rint(np.log(float(min(bh, bw))) / np.log(2.0) - 2)) - first_octave, 8))
    shapes = []
    for _ in range(n):
        if min(bh, bw) < 11 and shapes:
            break
        shapes.append((bh, bw))
        bh, bw = bh // 2, bw // 2
    return shapes


def sift_detect(gray, first_octave=-1, mask=None, max_kp=KMAX, device=0, with_dog=False):
    """mq_sift_detect on a batch of gray images (n, h, w): -> list of (k_i, 7) float32 keypoint arrays
    [x, y, size, angle, octave, layer, response] (and, ``with_dog``, per image the list of (5, h_o, w_o) DoG
    octaves)."""
    import torch
    ctx = _lib.Context.get(device)
    g = _dev(gray, np.uint8, device)
    n, h, w = g.shape
    m = None if mask is None else _dev(mask, np.uint8, device)
    kps = torch.zeros((n, max_kp, 7), dtype=torch.float32, device=g.device)
    cnt = torch.zeros((n,), dtype=torch.int32, device=g.device)
    shapes = dog_layout(h, w, first_octave)
    dog = torch.zeros((n, sum(5 * a * b for a, b in shapes)), dtype=torch.float32, device=g.device) if with_dog else None
    _lib.check(ctx.lib.mq_sift_detect(ctx.handle, _lib.ptr(g), n, h, w, int(first_octave), _lib.ptr(m), int(max_kp),
                                      _lib.ptr(kps), _lib.ptr(cnt), _lib.ptr(dog), _lib.stream_ptr(device)),
               "mq_sift_detect")
    c = cnt.cpu().numpy()
    out = [kps[i, :c[i]].cpu().numpy() for i in range(n)]
    if not with_dog:
        return out
    flat, dogs = dog.cpu().numpy(), []
    for i in range(n):
        off, per = 0, []
        for a, b in shapes:
            per.append(flat[i, off:off + 5 * a * b].reshape(5, a, b))
            off += 5 * a * b
        dogs.append(per)
    return out, dogs


def sift_describe(gray, kps_per_image, first_octave=-1, device=0):
    """mq_sift_describe: per image (k_i, 128) uint8 descriptors of the given keypoints."""
    import torch
    ctx = _lib.Context.get(device)
    g = _dev(gray, np.uint8, device)
    n, h, w = g.shape
    K = max(1, max(len(k) for k in kps_per_image))
    kp = np.zeros((n, K, 7), np.float32)
    for i, k in enumerate(kps_per_image):
        kp[i, :len(k)] = k
    cnt = _dev([len(k) for k in kps_per_image], np.int32, device)
    kpd = _dev(kp, np.float32, device)
    desc = torch.zeros((n, K, 128), dtype=torch.uint8, device=g.device)
    _lib.check(ctx.lib.mq_sift_describe(ctx.handle, _lib.ptr(g), n, h, w, int(first_octave), _lib.ptr(kpd),
                                        _lib.ptr(cnt), K, _lib.ptr(desc), _lib.stream_ptr(device)), "mq_sift_describe")
    d = desc.cpu().numpy()
    return [d[i, :len(k)] for i, k in enumerate(kps_per_image)]


def match_knn2(query, train, device=0):
    """mq_desc_match_knn2 for one pair of descriptor sets: idx (nq, 2), dist (nq, 2) int32 (squared L2)."""
    import torch
    ctx = _lib.Context.get(device)
    q = np.asarray(query, np.uint8).reshape(-1, 128)
    t = np.asarray(train, np.uint8).reshape(-1, 128)
    K = max(1, len(q), len(t))
    qb, tb = np.zeros((1, K, 128), np.uint8), np.zeros((1, K, 128), np.uint8)
    qb[0, :len(q)], tb[0, :len(t)] = q, t
    qd, td = _dev(qb, np.uint8, device), _dev(tb, np.uint8, device)
    nq, nt = _dev([len(q)], np.int32, device), _dev([len(t)], np.int32, device)
    idx = torch.zeros((1, K, 2), dtype=torch.int32, device=qd.device)
    dist = torch.zeros((1, K, 2), dtype=torch.int32, device=qd.device)
    _lib.check(ctx.lib.mq_desc_match_knn2(ctx.handle, _lib.ptr(qd), _lib.ptr(nq), _lib.ptr(td), _lib.ptr(nt), 1, K,
                                          _lib.ptr(idx), _lib.ptr(dist), _lib.stream_ptr(device)), "mq_desc_match_knn2")
    return idx[0, :len(q)].cpu().numpy(), dist[0, :len(q)].cpu().numpy()


def affine_partial_ransac(src, dst, thresh=3.0, device=0):
    """mq_affine_partial_ransac for one point set: dict(warp (2, 3), hyp, n_inliers, mask)."""
    import torch
    ctx = _lib.Context.get(device)
    src = np.asarray(src, np.float64).reshape(-1, 2)
    dst = np.asarray(dst, np.float64).reshape(-1, 2)
    n = len(src)
    K = max(1, n)
    pts = np.zeros((1, K, 4), np.float64)
    pts[0, :n, :2], pts[0, :n, 2:] = src, dst
    pd, cnt = _dev(pts, np.float64, device), _dev([n], np.int32, device)
    warp = torch.zeros((1, 6), dtype=torch.float64, device=pd.device)
    info = torch.zeros((1, 2), dtype=torch.int32, device=pd.device)
    mask = torch.zeros((1, K), dtype=torch.uint8, device=pd.device)
    _lib.check(ctx.lib.mq_affine_partial_ransac(ctx.handle, _lib.ptr(pd), _lib.ptr(cnt), 1, K, float(thresh),
                                                _lib.ptr(warp), _lib.ptr(info), _lib.ptr(mask),
                                                _lib.stream_ptr(device)), "mq_affine_partial_ransac")
    i = info.cpu().numpy()[0]
    return dict(warp=warp.cpu().numpy().reshape(2, 3), hyp=int(i[0]), n_inliers=int(i[1]),
                mask=mask.cpu().numpy()[0, :n].astype(bool))
