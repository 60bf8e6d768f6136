"""Chessboard corners on the GPU (csrc/chessboard.hip): what the reference's ``analyze_chessboardvid``
(multicam_toolbox.py:22-72) takes from ``cv2.findChessboardCorners`` and ``cv2.cornerSubPix``, as a detector of this
project's own for the 9 x 6 pattern.  ``tests/chessboard_ref.py`` is the numpy restatement.

``find_chessboard_corners`` is the product call: uint8 frames in, ordered sub-pixel corners out, ready for
``calibrate_intrinsic``.  The stage functions (``response``, ``candidates``, ``grid``, ``corner_subpix``) expose the
steps for the tests and the measurement tool.  There is no CPU path: without the library or a GPU every call raises.

``win``: cv2's half-window.  The reference's 11 needs corners more than about 24 px apart; closer corners put the
neighbouring corners inside the window and the refinement drifts (by pixels at 13-15 px spacing, where ``win=5`` stays
within a fraction of a pixel).  That is the algorithm's own property, and cv2's too."""
from __future__ import annotations

import numpy as np

from . import _lib

PATTERN = (9, 6)
N_CORNERS = 54
MAX_CANDIDATES = 1024
MAX_WIN = 16


def default_scale(width: int) -> float:
    """Detection runs on a half-size copy of frames wider than 1024."""
    return 0.5 if width > 1024 else 1.0


def _dev(a, dtype, device):
    import torch
    if not isinstance(a, torch.Tensor):
        a = np.ascontiguousarray(a)
        a = torch.from_numpy(a if a.flags.writeable else a.copy())
    return a.to(device=f"cuda:{device}", dtype=dtype).contiguous()


def _check_pattern(pattern):
    if tuple(pattern) != PATTERN:
        raise NotImplementedError(f"only the {PATTERN} pattern is implemented, got {tuple(pattern)}")


def response(gray, device=0):
    """mq_chess_response: gray uint8 (n, h, w) -> int32 (n, h, w) torch tensor on the device."""
    import torch
    ctx = _lib.Context.get(device)
    g = _dev(gray, torch.uint8, device)
    if g.dim() != 3:
        raise ValueError(f"gray must be (n, h, w), got {tuple(g.shape)}")
    n, h, w = g.shape
    out = torch.zeros((n, h, w), dtype=torch.int32, device=g.device)
    _lib.check(ctx.lib.mq_chess_response(ctx.handle, _lib.ptr(g), n, h, w, _lib.ptr(out), _lib.stream_ptr(device)),
               "mq_chess_response")
    return out


def candidates(resp, max_candidates=256, device=0):
    """mq_chess_candidates: int32 (n, h, w) -> (pos (n, K, 2) int32 [x, y], resp (n, K) int32, count (n,) int32),
    torch tensors on the device."""
    import torch
    ctx = _lib.Context.get(device)
    r = _dev(resp, torch.int32, device)
    if r.dim() != 3:
        raise ValueError(f"resp must be (n, h, w), got {tuple(r.shape)}")
    n, h, w = r.shape
    K = int(max_candidates)
    pos = torch.zeros((n, K, 2), dtype=torch.int32, device=r.device)
    val = torch.zeros((n, K), dtype=torch.int32, device=r.device)
    cnt = torch.zeros((n,), dtype=torch.int32, device=r.device)
    _lib.check(ctx.lib.mq_chess_candidates(ctx.handle, _lib.ptr(r), n, h, w, K, _lib.ptr(pos), _lib.ptr(val),
                                           _lib.ptr(cnt), _lib.stream_ptr(device)), "mq_chess_candidates")
    return pos, val, cnt


def grid(pos, resp, count, scale=1.0, device=0):
    """mq_chess_grid: candidates -> (found (n,) bool, corners (n, 54, 2) float64 in full-frame pixels, NaN where not
    found, index (n, 54) int32 candidate indices, -1 where not found) as numpy arrays."""
    import torch
    ctx = _lib.Context.get(device)
    p, v, c = _dev(pos, torch.int32, device), _dev(resp, torch.int32, device), _dev(count, torch.int32, device)
    if p.dim() != 3 or p.shape[2] != 2 or tuple(v.shape) != tuple(p.shape[:2]) or tuple(c.shape) != (p.shape[0],):
        raise ValueError("pos must be (n, K, 2), resp (n, K) and count (n,)")
    n, K = int(p.shape[0]), int(p.shape[1])
    found = torch.zeros((n,), dtype=torch.int32, device=p.device)
    corners = torch.zeros((n, N_CORNERS, 2), dtype=torch.float64, device=p.device)
    index = torch.zeros((n, N_CORNERS), dtype=torch.int32, device=p.device)
    _lib.check(ctx.lib.mq_chess_grid(ctx.handle, _lib.ptr(p), _lib.ptr(v), _lib.ptr(c), n, K, float(scale),
                                     _lib.ptr(found), _lib.ptr(corners), _lib.ptr(index), _lib.stream_ptr(device)),
               "mq_chess_grid")
    return found.cpu().numpy().astype(bool), corners.cpu().numpy(), index.cpu().numpy()


def corner_subpix(gray, corners, win=11, criteria=(30, 1e-3), device=0):
    """mq_corner_subpix: cv2.cornerSubPix(gray, corners, (win, win), (-1, -1), (EPS + MAX_ITER, *criteria)) in float64.
    gray uint8 (h, w) with corners (p, 2), or (n, h, w) with corners (n, p, 2); returns the refined corners as a
    float64 numpy array of the same shape (NaN rows stay NaN)."""
    import torch
    ctx = _lib.Context.get(device)
    g = _dev(gray, torch.uint8, device)
    c = np.array(corners, dtype=np.float64)
    single = g.dim() == 2
    if single:
        g, c = g[None], c[None]
    if g.dim() != 3 or c.ndim != 3 or c.shape[0] != g.shape[0] or c.shape[2] != 2:
        raise ValueError(f"gray {tuple(g.shape)} and corners {c.shape} do not match")
    n, h, w = g.shape
    d = torch.from_numpy(np.ascontiguousarray(c)).to(g.device)
    _lib.check(ctx.lib.mq_corner_subpix(ctx.handle, _lib.ptr(g), n, h, w, _lib.ptr(d), int(c.shape[1]), None, int(win),
                                        int(criteria[0]), float(criteria[1]), _lib.stream_ptr(device)),
               "mq_corner_subpix")
    out = d.cpu().numpy()
    return out[0] if single else out


def find_chessboard_corners(frames, pattern=PATTERN, scale=None, win=11, criteria=(30, 1e-3), max_candidates=256,
                            device=0, return_info=False):
    """mq_find_chessboard on a batch: frames uint8 (n, H, W, 3) BGR or (n, H, W) gray (numpy or torch) ->
    ``found`` (n,) bool and ``corners`` (n, 54, 2) float64 in objp's order (9 along the fast axis, not mirrored),
    NaN where not found.  ``scale`` None: 0.5 for frames wider than 1024, else 1.  ``return_info`` adds a dict with
    the scale used."""
    import torch
    _check_pattern(pattern)
    ctx = _lib.Context.get(device)
    f = _dev(frames, torch.uint8, device)
    if f.dim() == 3:
        f = f[..., None].expand(-1, -1, -1, 3).contiguous()   # gray in, gray out of BGR2GRAY: (b + g + r) weights sum to 1
    if f.dim() != 4 or f.shape[3] != 3:
        raise ValueError(f"frames must be (n, H, W, 3) or (n, H, W), got {tuple(f.shape)}")
    n, H, W, _ = f.shape
    scale = default_scale(W) if scale is None else float(scale)
    found = torch.zeros((n,), dtype=torch.int32, device=f.device)
    corners = torch.full((n, N_CORNERS, 2), float("nan"), dtype=torch.float64, device=f.device)
    _lib.check(ctx.lib.mq_find_chessboard(ctx.handle, _lib.ptr(f), int(f.stride(0)) if n else H * W * 3, n, H, W,
                                          scale, int(win), int(criteria[0]), float(criteria[1]), int(max_candidates),
                                          _lib.ptr(found), _lib.ptr(corners), _lib.stream_ptr(device)),
               "mq_find_chessboard")
    res = found.cpu().numpy().astype(bool), corners.cpu().numpy()
    return res + ({"scale": scale},) if return_info else res
