"""Image resize on the GPU: ``cv2.resize(img, [800, 600])`` of the reference's videos (step3_crossframematching.py
``visualize`` :1685, visualize_result.py :164, :249) through ``mq_resize_bilinear`` (csrc/resize.hip), after cv2's
8-bit INTER_LINEAR fixed-point scheme.  The rule is the project's restatement (include/mq_hip.h states it,
tests/track_video_ref.py is the NumPy one); parity with cv2 itself is unpinned.  No CPU fallback.
"""
from __future__ import annotations

import numpy as np


def resize_bilinear(frames, height, width, device=0):
    """``frames``: uint8 (n, H, W, 3) BGR, a numpy array (uploaded) or a device tensor (used as is; a view whose
    images are contiguous keeps its stride between images).  Returns a new torch.uint8 (n, height, width, 3) on
    the device."""
    import torch

    from . import _lib as L
    dev = torch.device("cuda", device)
    if not torch.is_tensor(frames):
        frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint8))
    frames = frames.to(dev)
    if frames.dtype != torch.uint8 or frames.ndim != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames must be uint8 (n, H, W, 3), got {frames.dtype} {tuple(frames.shape)}")
    n, H, W, _ = frames.shape
    height, width = int(height), int(width)
    if min(H, W, height, width) < 1:
        raise ValueError("image sizes must be positive")
    if n and frames.stride()[1:] != (3 * W, 3, 1) or (n > 1 and frames.stride(0) < H * W * 3):
        frames = frames.contiguous()
    stride = frames.stride(0) if n > 1 else H * W * 3
    out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=dev)
    if n == 0:
        return out
    ctx = L.Context.get(device)
    L.check(ctx.lib.mq_resize_bilinear(ctx.handle, L.ptr(frames), stride, n, H, W, L.ptr(out), height * width * 3,
                                       height, width, L.stream_ptr(dev)), "mq_resize_bilinear")
    return out
