"""Baseline JPEG frames on the GPU: ``mq_jpeg_encode`` (csrc/jpeg.hip) behind ``JpegEncoder``.

The codec is stated in include/mq_hip.h and restated in NumPy by tests/jpeg_ref.py, which this equals byte for
byte.  Frames stay on the device; only the sizes and then the used bytes of each stream are copied back.  No CPU
fallback.  ``mqhip.io.MjpegAviWriter`` puts the streams into a Motion-JPEG AVI.
"""
from __future__ import annotations

import numpy as np

MAX_DIM = 65535
MAX_RESTART_INTERVAL = 32     # csrc/jpeg.hpp JPEG_MAX_RI
MAX_FRAMES = 65535            # frames per call


def check_args(height, width, quality, restart_interval):
    """The bounds the entry point enforces, raised here with a Python message."""
    if not (1 <= int(height) <= MAX_DIM and 1 <= int(width) <= MAX_DIM):
        raise ValueError(f"height and width must be in [1, {MAX_DIM}], got {height} x {width}")
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must be in [1, 100], got {quality}")
    if not 1 <= int(restart_interval) <= MAX_RESTART_INTERVAL:
        raise ValueError(f"restart_interval must be in [1, {MAX_RESTART_INTERVAL}], got {restart_interval}")


class JpegEncoder:
    """``encode(frames)`` -> ``list[bytes]``, one complete JPEG per frame of a uint8 (N, height, width, 3) BGR
    array (host) or tensor (device)."""

    def __init__(self, height, width, quality=90, restart_interval=16, device=0):
        import torch

        from . import _lib
        check_args(height, width, quality, restart_interval)
        self.H, self.W = int(height), int(width)
        self.quality, self.ri = int(quality), int(restart_interval)
        self.device = device
        self.dev = torch.device("cuda", device)
        self._lib = _lib
        self.ctx = _lib.Context.get(device)
        self.max_bytes = int(self.ctx.lib.mq_jpeg_max_bytes(self.H, self.W, self.ri))
        if not 0 < self.max_bytes < 2 ** 31:
            raise ValueError(f"the worst-case stream of a {self.H} x {self.W} frame at restart_interval {self.ri} "
                             f"exceeds 2^31 - 1 bytes")

    def _frames(self, frames):
        import torch
        if not torch.is_tensor(frames):
            frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint8))
        frames = frames.to(self.dev).contiguous()
        if frames.dtype != torch.uint8 or frames.ndim != 4 or tuple(frames.shape[1:]) != (self.H, self.W, 3):
            raise ValueError(f"frames must be uint8 (N, {self.H}, {self.W}, 3), got {frames.dtype} "
                             f"{tuple(frames.shape)}")
        if frames.shape[0] > MAX_FRAMES:
            raise ValueError(f"at most {MAX_FRAMES} frames per call, got {frames.shape[0]}")
        return frames

    def encode_into(self, frames, out, sizes):
        """The entry point on caller-owned device tensors: ``out`` uint8 (N, out_stride), ``sizes`` int32 (N,).
        An ``out_stride`` below ``max_bytes`` raises ``MqError`` (-2)."""
        L = self._lib
        frames = self._frames(frames)
        n = frames.shape[0]
        L.check(self.ctx.lib.mq_jpeg_encode(
            self.ctx.handle, L.ptr(frames), self.H * self.W * 3, n, self.H, self.W, self.quality, self.ri, L.ptr(out),
            out.shape[1], L.ptr(sizes), L.stream_ptr(self.dev)), "mq_jpeg_encode")
        return out, sizes

    def encode_device(self, frames):
        """``(out, sizes)``: uint8 (N, max_bytes) and int32 (N,) device tensors; frame i's JPEG is
        ``out[i, :sizes[i]]``."""
        import torch
        frames = self._frames(frames)
        n = frames.shape[0]
        out = torch.empty((n, self.max_bytes), dtype=torch.uint8, device=self.dev)
        sizes = torch.zeros((n,), dtype=torch.int32, device=self.dev)
        if n == 0:
            return out, sizes
        return self.encode_into(frames, out, sizes)

    def encode(self, frames):
        out, sizes = self.encode_device(frames)
        sizes = sizes.cpu().numpy()
        return [out[i, :int(s)].cpu().numpy().tobytes() for i, s in enumerate(sizes)]
