"""Pose overlay frames on the GPU: the reference's ``visualize_result.proc`` (:220-242 with ``clean_kp`` and
``draw_kps``) from kp3d to the drawn BGR frame, through ``mq_overlay_primitives`` / ``mq_overlay_render``
(csrc/overlay.hip).  The coverage rules are the project's own and exact (see overlay.hip's head and
tests/overlay_ref.py); cv2's rasterisers are not restated.  No CPU fallback.

``render(colour=, labels=)`` is step 3's tracking video (step3_crossframematching.py ``visualize`` :1624-1670):
a colour index per (image, animal) and a text written at the upper left of the skeleton, through
``mq_overlay_render_labelled``.  The text is drawn with ``FONT``, a stroke font of the project's own whose metrics
follow Hershey simplex (what ``cv2.putText`` draws with); cv2's glyph shapes are not available here and are not
restated, so the letter forms are unpinned.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MAX_ANIMALS = 8       # csrc/overlay.hpp OVL_MAX_ANIMALS
MAX_PRIMS = 64        # csrc/overlay.hpp OVL_MAX_PRIMS (disc + limb slots per animal)
JOINT_DISC = 1        # draw_kps draws a disc at the joint
JOINT_NULLED = 2      # clean_kp sets the joint to None: no disc, and no limb that ends there

# BGR, visualize_result.py:191 (clrs scaled by 255 in draw_kps :95-98) and :239-242 (black from the fifth animal)
COLOURS = ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255))

MAX_LABEL_SEGS = 96     # csrc/overlay.hpp OVL_MAX_LABEL_SEGS
MAX_LABEL_COORD = 8192  # csrc/overlay.hpp OVL_MAX_LABEL_COORD
MAX_GLYPH_SEGS = 16
CAP_HEIGHT = 21         # glyph units; Hershey simplex's capital height
ADVANCE = 20            # glyph units from one glyph's origin to the next

# Polylines per glyph on an integer grid: x in [0, ADVANCE], y in [0, CAP_HEIGHT] growing upward from the baseline,
# the origin at the left end of the baseline.
FONT = {
    "0": (((6, 0), (12, 0), (16, 5), (16, 16), (12, 21), (6, 21), (2, 16), (2, 5), (6, 0)),),
    "1": (((5, 17), (9, 21), (9, 0)),),
    "2": (((2, 16), (6, 21), (12, 21), (16, 16), (16, 12), (2, 0), (16, 0)),),
    "3": (((2, 21), (16, 21), (8, 12), (12, 12), (16, 8), (16, 4), (12, 0), (6, 0), (2, 4)),),
    "4": (((12, 0), (12, 21), (2, 7), (17, 7)),),
    "5": (((15, 21), (4, 21), (3, 12), (7, 14), (12, 14), (16, 10), (16, 4), (12, 0), (6, 0), (2, 4)),),
    "6": (((15, 19), (11, 21), (7, 21), (3, 16), (2, 10), (2, 5), (6, 0), (12, 0), (16, 4), (16, 9), (12, 13), (6, 13),
           (2, 9)),),
    "7": (((2, 21), (16, 21), (7, 0)),),
    "8": (((7, 21), (11, 21), (15, 18), (15, 14), (11, 11), (7, 11), (3, 14), (3, 18), (7, 21)),
          ((7, 11), (2, 7), (2, 3), (6, 0), (12, 0), (16, 3), (16, 7), (11, 11))),
    "9": (((3, 2), (7, 0), (11, 0), (15, 5), (16, 11), (16, 16), (12, 21), (6, 21), (2, 17), (2, 12), (6, 8), (12, 8),
           (16, 12)),),
    "-": (((3, 9), (15, 9)),),
}


def glyph_segments(ch):
    """The glyph's strokes as (x0, y0, x1, y1) in glyph units."""
    if ch not in FONT:
        raise ValueError(f"no glyph for {ch!r}: the font has {''.join(sorted(FONT))}")
    return [(a[0], a[1], b[0], b[1]) for line in FONT[ch] for a, b in zip(line[:-1], line[1:])]


def label_segments(text, scale=2.0, thickness=5):
    """The stroke segments of ``text`` as int32 (n, 4) rows x0, y0, x1, y1 in image space (y downward) relative to
    the left end of the baseline, what ``cv2.putText``'s ``org`` is: glyph units times ``scale``, rounded half to
    even.  ValueError for a character outside ``FONT``, more than ``MAX_LABEL_SEGS`` segments, a thickness outside
    [1, 32] or a coordinate beyond ``MAX_LABEL_COORD``."""
    if not 1 <= int(thickness) <= 32:
        raise ValueError("thickness must be in [1, 32]")
    rows = []
    for i, ch in enumerate(str(text)):
        for x0, y0, x1, y1 in glyph_segments(ch):
            rows.append([(i * ADVANCE + x0) * scale, -y0 * scale, (i * ADVANCE + x1) * scale, -y1 * scale])
    if len(rows) > MAX_LABEL_SEGS:
        raise ValueError(f"{text!r} needs {len(rows)} segments, more than {MAX_LABEL_SEGS}")
    seg = np.rint(np.asarray(rows, dtype=np.float64).reshape(-1, 4))
    if len(seg) and not np.abs(seg).max() <= MAX_LABEL_COORD:
        raise ValueError(f"{text!r} at scale {scale} leaves [-{MAX_LABEL_COORD}, {MAX_LABEL_COORD}]")
    return seg.astype(np.int32)


def label_tables(labels, B, A, scale=2.0, thickness=5):
    """``labels``: B lists of A strings or None -> (seg int32 (B, A, S, 4), n int32 (B, A)), S >= 1."""
    if len(labels) != B or any(len(row) != A for row in labels):
        raise ValueError(f"labels must be {B} lists of {A} strings or None")
    segs = [[label_segments(t, scale, thickness) if t is not None else np.zeros((0, 4), np.int32) for t in row]
            for row in labels]
    S = max([1] + [len(g) for row in segs for g in row])
    seg = np.zeros((B, A, S, 4), dtype=np.int32)
    n = np.zeros((B, A), dtype=np.int32)
    for b, row in enumerate(segs):
        for a, g in enumerate(row):
            seg[b, a, :len(g)] = g
            n[b, a] = len(g)
    return seg, n


@dataclass(frozen=True)
class Skeleton:
    """draw_kps' tables for ``n_joints`` joints plus the neck (slot ``n_joints``)."""
    pairs: tuple          # limb (slot, slot) pairs, the reference's kp_con
    radius_add: tuple     # per slot: disc radius = mrksize + radius_add
    flags: tuple          # per slot: JOINT_DISC | JOINT_NULLED
    n_joints: int = 17

    def radius(self, mrksize):
        return np.asarray([mrksize + r for r in self.radius_add], dtype=np.int32)


# visualize_result.py draw_kps :73-93, :100-105: every slot gets a disc, the eyes (1, 2) one pixel larger
_V1 = Skeleton(
    pairs=((0, 2), (0, 1), (2, 4), (1, 3), (6, 8), (5, 7), (8, 10), (7, 9), (12, 14), (11, 13), (14, 16), (13, 15),
           (0, 17), (17, 6), (17, 5), (17, 12), (17, 11)),
    radius_add=tuple(1 if j in (1, 2) else 0 for j in range(18)),
    flags=(JOINT_DISC,) * 18)
# visualize_result_2.py: clean_kp :39-41 sets the eyes to None (so neither their discs nor the five limbs of
# kp_con :98-127 that end at an eye are ever drawn) and draw_kps :136-137 skips their discs
_V2 = Skeleton(
    pairs=((1, 2), (0, 1), (0, 2), (1, 3), (2, 4), (3, 4), (0, 17), (3, 17), (4, 17), (17, 5), (17, 6), (5, 6),
           (17, 11), (17, 12), (11, 12), (5, 7), (7, 9), (6, 8), (8, 10), (11, 13), (13, 15), (12, 14), (14, 16),
           (5, 11), (6, 12), (5, 12), (6, 11)),
    radius_add=(0,) * 18,
    flags=tuple(JOINT_NULLED if j in (1, 2) else JOINT_DISC for j in range(18)))
SKELETONS = {"v1": _V1, "v2": _V2}


def check_skeleton(sk: Skeleton, n_animals=None):
    """The bounds the entry points enforce, raised here with a Python message."""
    J, P = sk.n_joints, len(sk.pairs)
    if J < 7:
        raise ValueError("the neck is the mean of joints 5 and 6: n_joints must be >= 7")
    if len(sk.radius_add) != J + 1 or len(sk.flags) != J + 1:
        raise ValueError("radius_add and flags need n_joints + 1 entries (the neck is the last)")
    if J + 1 + P > MAX_PRIMS:
        raise ValueError(f"{J + 1} discs + {P} limbs exceed {MAX_PRIMS} primitives per animal")
    if any(not (0 <= a <= J and 0 <= b <= J) for a, b in sk.pairs):
        raise ValueError("pair joint outside [0, n_joints]")
    if n_animals is not None and not 1 <= n_animals <= MAX_ANIMALS:
        raise ValueError(f"n_animals must be in [1, {MAX_ANIMALS}], got {n_animals}")


class OverlayRenderer:
    """``cgroup``: a ``mqhip.geometry.CameraGroup``; ``cam_idx`` below indexes its cameras."""

    def __init__(self, cgroup, height, width, skeleton="v1", mrksize=3, device=0):
        import torch

        from . import _lib
        self.sk = SKELETONS[skeleton] if isinstance(skeleton, str) else skeleton
        check_skeleton(self.sk)
        if not 0 <= int(mrksize) <= 254:
            raise ValueError("mrksize must be in [0, 254]")
        self.cgroup, self.H, self.W, self.mrksize = cgroup, int(height), int(width), int(mrksize)
        self.device = device
        self.dev = torch.device("cuda", device)
        self._lib = _lib
        self.ctx = _lib.Context.get(device)
        # host arrays of the skeleton (the entry points read them on the host)
        self._pairs = np.ascontiguousarray(np.asarray(self.sk.pairs, dtype=np.int32).reshape(-1, 2))
        self._radius = np.ascontiguousarray(self.sk.radius(self.mrksize))
        self._flags = np.ascontiguousarray(np.asarray(self.sk.flags, dtype=np.int32))

    # ------------------------------------------------------------------ arguments
    def _pose_args(self, cam_idx, kp3d, score, label_slot=0):
        import torch
        kp3d = np.ascontiguousarray(kp3d, dtype=np.float64)
        score = np.ascontiguousarray(score, dtype=np.float64)
        if kp3d.ndim != 4 or kp3d.shape[3] != 3 or kp3d.shape[2] != self.sk.n_joints:
            raise ValueError(f"kp3d must be (B, A, {self.sk.n_joints}, 3), got {kp3d.shape}")
        B, A, J, _ = kp3d.shape
        if score.shape != (B, A, J):
            raise ValueError(f"score must be {(B, A, J)}, got {score.shape}")
        check_skeleton(self.sk, A)
        cam = np.array(np.broadcast_to(np.asarray(cam_idx, dtype=np.int32), (B,)))   # a writable copy
        C = len(self.cgroup.cameras)
        if B and (cam.min() < 0 or cam.max() >= C):
            raise ValueError(f"cam_idx outside [0, {C})")
        P = len(self.sk.pairs)
        up = lambda a: torch.from_numpy(a).to(self.dev)
        if label_slot and J + 2 + P > MAX_PRIMS:
            raise ValueError(f"{J + 1} discs + {P} limbs + the label exceed {MAX_PRIMS} primitives per animal")
        prim_i = torch.zeros((B, A, J + 1 + P + label_slot, 8), dtype=torch.int32, device=self.dev)
        prim_d = torch.zeros((B, A, P, 4), dtype=torch.float64, device=self.dev)
        return B, A, J, P, C, up(cam), up(kp3d), up(score), prim_i, prim_d

    def _skel_args(self, A, J, P):
        c = lambda a: a.ctypes.data
        return (c(self._pairs), P, c(self._radius), c(self._flags), self.mrksize)

    # ------------------------------------------------------------------ API
    def primitives(self, cam_idx, kp3d, score):
        """The primitive tables of B images: ``(prim_i, prim_d)`` as numpy arrays -- int32 (B, A, J + 1 + P, 8)
        [valid, cx, cy, r, x0, y0, x1, y1] (discs, then limbs) and float64 (B, A, P, 4) limb end points."""
        L = self._lib
        B, A, J, P, C, cam_d, kp_d, sc_d, prim_i, prim_d = self._pose_args(cam_idx, kp3d, score)
        L.check(self.ctx.lib.mq_overlay_primitives(
            self.ctx.handle, L.ptr(self.cgroup.cams_tensor()), C, L.ptr(cam_d), L.ptr(kp_d), L.ptr(sc_d), B, A, J,
            *self._skel_args(A, J, P), L.ptr(prim_i), L.ptr(prim_d), L.stream_ptr(self.dev)),
            "mq_overlay_primitives")
        return prim_i.cpu().numpy(), prim_d.cpu().numpy()

    def _label_args(self, B, A, colour, labels, label_scale, label_thickness):
        """Device tables of the labelled entry points: (colour, seg, n, S, t) and the tensors to keep alive."""
        import torch
        L = self._lib
        if not 1 <= int(label_thickness) <= 32:
            raise ValueError("label_thickness must be in [1, 32]")
        col_d = seg_d = n_d = None
        S = 0
        if colour is not None:
            colour = np.ascontiguousarray(colour, dtype=np.int32)
            if colour.shape != (B, A):
                raise ValueError(f"colour must be {(B, A)}, got {colour.shape}")
            col_d = torch.from_numpy(colour).to(self.dev)
        if labels is not None:
            seg, n = label_tables(labels, B, A, label_scale, label_thickness)
            S = seg.shape[2]
            seg_d, n_d = torch.from_numpy(seg).to(self.dev), torch.from_numpy(n).to(self.dev)
        return (L.ptr(col_d), L.ptr(seg_d), L.ptr(n_d), S, int(label_thickness)), (col_d, seg_d, n_d)

    def primitives_labelled(self, cam_idx, kp3d, score, colour=None, labels=None, label_scale=2.0, label_thickness=5):
        """``primitives`` with the label slot: prim_i int32 (B, A, J + 2 + P, 8), the last slot of an animal
        [valid, origin x, origin y, 0, x0, y0, x1, y1], and prim_d."""
        L = self._lib
        B, A, J, P, C, cam_d, kp_d, sc_d, prim_i, prim_d = self._pose_args(cam_idx, kp3d, score, label_slot=1)
        largs, keep = self._label_args(B, A, colour, labels, label_scale, label_thickness)
        L.check(self.ctx.lib.mq_overlay_primitives_labelled(
            self.ctx.handle, L.ptr(self.cgroup.cams_tensor()), C, L.ptr(cam_d), L.ptr(kp_d), L.ptr(sc_d), B, A, J,
            *self._skel_args(A, J, P), *largs, L.ptr(prim_i), L.ptr(prim_d), L.stream_ptr(self.dev)),
            "mq_overlay_primitives_labelled")
        return prim_i.cpu().numpy(), prim_d.cpu().numpy()

    def render(self, frames, cam_idx, kp3d, score, src_index=None, colour=None, labels=None, label_scale=2.0,
               label_thickness=5):
        """``frames``: uint8 (N, H, W, 3) BGR pool (a numpy array is uploaded once; a device tensor is used as
        is); output b is drawn over ``frames[src_index[b]]`` (default: b).  ``cam_idx``: (B,) or a scalar;
        ``kp3d`` (B, A, J, 3), ``score`` (B, A, J).  Returns a new torch.uint8 (B, H, W, 3) on the device.
        ``colour``: int (B, A), 0..3 picks ``COLOURS``, anything else (step 3's -1) black; None colours by animal
        index.  ``labels``: B lists of A strings or None, written in ``FONT`` at ``label_scale`` with strokes
        ``label_thickness`` wide, the baseline's left end at the upper left of the reprojected skeleton.  With both
        None the unlabelled entry point is called."""
        import torch
        L = self._lib
        if not torch.is_tensor(frames):
            frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint8))
        frames = frames.to(self.dev).contiguous()
        if frames.dtype != torch.uint8 or frames.ndim != 4 or tuple(frames.shape[1:]) != (self.H, self.W, 3):
            raise ValueError(f"frames must be uint8 (N, {self.H}, {self.W}, 3), got {frames.dtype} {tuple(frames.shape)}")
        labelled = colour is not None or labels is not None
        B, A, J, P, C, cam_d, kp_d, sc_d, prim_i, prim_d = self._pose_args(cam_idx, kp3d, score,
                                                                            label_slot=int(labelled))
        n_src = frames.shape[0]
        src = np.arange(B, dtype=np.int32) if src_index is None else np.ascontiguousarray(src_index, dtype=np.int32)
        if src.shape != (B,) or (B and (src.min() < 0 or src.max() >= n_src)):
            raise ValueError(f"src_index must be (B,) in [0, {n_src})")
        src_d = torch.from_numpy(src).to(self.dev)
        out = torch.empty((B, self.H, self.W, 3), dtype=torch.uint8, device=self.dev)
        if B == 0:
            return out
        if labelled:
            largs, keep = self._label_args(B, A, colour, labels, label_scale, label_thickness)
            L.check(self.ctx.lib.mq_overlay_render_labelled(
                self.ctx.handle, L.ptr(self.cgroup.cams_tensor()), C, L.ptr(cam_d), L.ptr(kp_d), L.ptr(sc_d), B, A, J,
                *self._skel_args(A, J, P), L.ptr(frames), self.H * self.W * 3, n_src, L.ptr(src_d), self.H, self.W,
                *largs, L.ptr(prim_i), L.ptr(prim_d), L.ptr(out), L.stream_ptr(self.dev)),
                "mq_overlay_render_labelled")
            return out
        L.check(self.ctx.lib.mq_overlay_render(
            self.ctx.handle, L.ptr(self.cgroup.cams_tensor()), C, L.ptr(cam_d), L.ptr(kp_d), L.ptr(sc_d), B, A, J,
            *self._skel_args(A, J, P), L.ptr(frames), self.H * self.W * 3, n_src, L.ptr(src_d), self.H, self.W,
            L.ptr(prim_i), L.ptr(prim_d), L.ptr(out), L.stream_ptr(self.dev)), "mq_overlay_render")
        return out
