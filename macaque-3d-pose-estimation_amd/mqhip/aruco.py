"""ArUco markers on the GPU (csrc/aruco.hip): what the reference's ``analyze_aruco_marker_vid`` and
``analyze_aruco_cube_vid`` (multicam_toolbox.py:244-391) take from ``cv2.resize`` and ``aruco.detectMarkers``, as a
detector of this project's own for 4 x 4 codes.  ``tests/aruco_ref.py`` is the numpy
restatement.

``find_markers`` is the product call: uint8 frames and a dictionary in, marker ids and ordered sub-pixel corners
out.  The dictionary is the caller's: an array of 16-bit codes, row-major from the most significant bit, white = 1
(cv2's predefined dictionaries are not included).  ``dictionary=None`` accepts every quad with a dark border, with
id -1.  The stage functions (``threshold``, ``label``, ``components``, ``quads``) expose the steps for the tests and
the measurement tool.  There is no CPU path: without the library or a GPU every call raises."""
from __future__ import annotations

import numpy as np

from . import _lib

DET_SIZE = (640, 480)      # the reference's detection size (:269-270), (width, height)
MAX_QUADS = 64
MAX_CODES = 1024
CAND_FIELDS = 16


def _dev(a, dtype, device):
    import torch
    if not isinstance(a, torch.Tensor):
        a = np.ascontiguousarray(a)
        a = torch.from_numpy(a if a.flags.writeable else a.copy())
    return a.to(device=f"cuda:{device}", dtype=dtype).contiguous()


def _images(a, dtype, device, what):
    t = _dev(a, dtype, device)
    if t.dim() != 3:
        raise ValueError(f"{what} must be (n, h, w), got {tuple(t.shape)}")
    return t


def _dictionary(dictionary, device):
    """-> (device int16 tensor or None, n_codes)."""
    import torch
    if dictionary is None:
        return None, 0
    if isinstance(dictionary, torch.Tensor):
        d = dictionary.reshape(-1)
        if d.dtype == torch.uint16:
            d = d.view(torch.int16)
        elif d.dtype != torch.int16:              # the same 16 bits: codes above 0x7fff wrap to negative int16
            d = d.to(torch.int64)
            d = torch.where(d >= 0x8000, d - 0x10000, d).to(torch.int16)
        d = d.to(device=f"cuda:{device}").contiguous()
    else:
        codes = np.asarray(dictionary)
        if codes.size and (codes.min() < 0 or codes.max() > 0xFFFF):
            raise ValueError("dictionary codes must fit 16 bits")
        d = torch.from_numpy(np.ascontiguousarray(codes.astype(np.uint16).view(np.int16).reshape(-1))).to(f"cuda:{device}")
    if not 1 <= d.numel() <= MAX_CODES:
        raise ValueError(f"the dictionary must hold 1 to {MAX_CODES} codes, got {d.numel()}")
    return d, int(d.numel())


def threshold(gray, device=0):
    """mq_aruco_threshold: gray uint8 (n, h, w) -> uint8 (n, h, w), 1 where dark; a torch tensor on the device."""
    import torch
    ctx = _lib.Context.get(device)
    g = _images(gray, torch.uint8, device, "gray")
    n, h, w = g.shape
    out = torch.zeros((n, h, w), dtype=torch.uint8, device=g.device)
    _lib.check(ctx.lib.mq_aruco_threshold(ctx.handle, _lib.ptr(g), n, h, w, _lib.ptr(out), _lib.stream_ptr(device)),
               "mq_aruco_threshold")
    return out


def label(dark, device=0):
    """mq_aruco_label: dark uint8 (n, h, w) -> int32 (n, h, w): the smallest linear index of the pixel's 4-connected
    component, -1 where light; a torch tensor on the device."""
    import torch
    ctx = _lib.Context.get(device)
    d = _images(dark, torch.uint8, device, "dark")
    n, h, w = d.shape
    out = torch.full((n, h, w), -1, dtype=torch.int32, device=d.device)
    _lib.check(ctx.lib.mq_aruco_label(ctx.handle, _lib.ptr(d), n, h, w, _lib.ptr(out), _lib.stream_ptr(device)),
               "mq_aruco_label")
    return out


def components(labels, max_quads=MAX_QUADS, device=0):
    """mq_aruco_components: labels int32 (n, h, w) -> (count (n,) int32, cand (n, max_quads, 16) int32), torch
    tensors on the device.  count is the number of components that pass the gates; cand holds the first max_quads."""
    import torch
    ctx = _lib.Context.get(device)
    lab = _images(labels, torch.int32, device, "labels")
    n, h, w = lab.shape
    Q = int(max_quads)
    cnt = torch.zeros((n,), dtype=torch.int32, device=lab.device)
    cand = torch.zeros((n, Q, CAND_FIELDS), dtype=torch.int32, device=lab.device)
    _lib.check(ctx.lib.mq_aruco_components(ctx.handle, _lib.ptr(lab), n, h, w, Q, _lib.ptr(cnt), _lib.ptr(cand),
                                           _lib.stream_ptr(device)), "mq_aruco_components")
    return cnt, cand


def quads(gray, count, cand, dictionary, max_correction_bits=0, border_errors=0, device=0):
    """mq_aruco_quads: gray uint8 (n, h, w) and the candidates -> (ok (n, Q) bool, ids (n, Q) int32, rot (n, Q) int32,
    corners (n, Q, 4, 2) float64 in pixels of gray, NaN where not ok) as numpy arrays."""
    import torch
    ctx = _lib.Context.get(device)
    g = _images(gray, torch.uint8, device, "gray")
    c, q = _dev(count, torch.int32, device), _dev(cand, torch.int32, device)
    n, h, w = g.shape
    if q.dim() != 3 or q.shape[0] != n or q.shape[2] != CAND_FIELDS or tuple(c.shape) != (n,):
        raise ValueError(f"count must be (n,) and cand (n, max_quads, {CAND_FIELDS})")
    Q = int(q.shape[1])
    d, n_codes = _dictionary(dictionary, device)
    ok = torch.zeros((n, Q), dtype=torch.int32, device=g.device)
    ids = torch.full((n, Q), -1, dtype=torch.int32, device=g.device)
    rot = torch.zeros((n, Q), dtype=torch.int32, device=g.device)
    corners = torch.full((n, Q, 4, 2), float("nan"), dtype=torch.float64, device=g.device)
    _lib.check(ctx.lib.mq_aruco_quads(ctx.handle, _lib.ptr(g), n, h, w, _lib.ptr(c), _lib.ptr(q), Q, _lib.ptr(d),
                                      n_codes, int(max_correction_bits), int(border_errors), _lib.ptr(ok),
                                      _lib.ptr(ids), _lib.ptr(rot), _lib.ptr(corners), _lib.stream_ptr(device)),
               "mq_aruco_quads")
    return ok.cpu().numpy().astype(bool), ids.cpu().numpy(), rot.cpu().numpy(), corners.cpu().numpy()


def find_markers(frames, dictionary, det_size=DET_SIZE, max_markers=8, max_quads=MAX_QUADS, max_correction_bits=0,
                 border_errors=0, device=0, return_info=False):
    """mq_find_markers on a batch: frames uint8 (n, H, W, 3) BGR or (n, H, W) gray (numpy or torch) ->
    ``count`` (n,) int32, ``ids`` (n, max_markers) int32 (-1 past the count) and ``corners`` (n, max_markers, 4, 2)
    float64 in frame pixels (NaN past the count), corner 0 the marker's top-left, clockwise, ordered by (id, label).
    ``det_size`` = (width, height) of the detection image, at most the frame's size.  ``return_info`` adds a dict with
    the ratios and the candidate count per frame before ``max_quads`` cut it."""
    import torch
    ctx = _lib.Context.get(device)
    f = _dev(frames, torch.uint8, device)
    if f.dim() == 3:
        f = f[..., None].expand(-1, -1, -1, 3).contiguous()   # gray in, gray out: the BGR2GRAY weights sum to 1
    if f.dim() != 4 or f.shape[3] != 3:
        raise ValueError(f"frames must be (n, H, W, 3) or (n, H, W), got {tuple(f.shape)}")
    n, H, W, _ = f.shape
    dw, dh = int(det_size[0]), int(det_size[1])
    d, n_codes = _dictionary(dictionary, device)
    M = int(max_markers)
    count = torch.zeros((n,), dtype=torch.int32, device=f.device)
    ids = torch.full((n, M), -1, dtype=torch.int32, device=f.device)
    corners = torch.full((n, M, 4, 2), float("nan"), dtype=torch.float64, device=f.device)
    n_cand = torch.zeros((n,), dtype=torch.int32, device=f.device)
    _lib.check(ctx.lib.mq_find_markers(ctx.handle, _lib.ptr(f), int(f.stride(0)) if n else H * W * 3, n, H, W, dw, dh,
                                       _lib.ptr(d), n_codes, int(max_correction_bits), int(border_errors),
                                       int(max_quads), M, _lib.ptr(count), _lib.ptr(ids), _lib.ptr(corners),
                                       _lib.ptr(n_cand), _lib.stream_ptr(device)), "mq_find_markers")
    res = count.cpu().numpy(), ids.cpu().numpy(), corners.cpu().numpy()
    if return_info:
        res += ({"ratio": (W / dw, H / dh), "candidates": n_cand.cpu().numpy()},)
    return res
