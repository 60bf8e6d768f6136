"""Baseline JPEG frames on the GPU: ``mq_jpeg_encode`` (csrc/jpeg.hip) behind ``JpegEncoder``.

The codec is stated in include/mq_hip.h and restated in NumPy by tests/jpeg_ref.py, which this equals byte for
byte.  Frames stay on the device; only the sizes and then the used bytes of each stream are copied back.  No CPU
fallback.  ``mqhip.io.MjpegAviWriter`` puts the streams into a Motion-JPEG AVI.
"""
from __future__ import annotations

import ctypes as _C

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


# ------------------------------------------------------------------------------------------------ decoding


# include/mq_hip.h MQ_JPEG_E_*: what mq_jpeg_parse refuses
PARSE_ERRORS = {-20: "not a JPEG stream", -21: "truncated header", -22: "not baseline (SOF0)", -23: "not 8-bit samples",
                -24: "16-bit or out-of-range quantisation table", -25: "neither grayscale nor YCbCr",
                -26: "sampling other than 4:4:4, 4:2:2, 4:2:0", -27: "not one interleaved scan",
                -28: "a table the stream never defined", -29: "a Huffman table that is no prefix code",
                -30: "no EOI after the scan", -31: "height or width 0"}
# status of a decoded frame
STATUS = {1: "restart markers wrong in count or sequence", 2: "bits that match no Huffman code",
          3: "a run past coefficient 63", 4: "an interval's bits exhausted before its MCUs"}


class JpegError(ValueError):
    """A stream the decoder refuses (``code`` < 0: the parser) or cannot decode (``code`` > 0: the status)."""

    def __init__(self, frame, code):
        what = PARSE_ERRORS.get(code) or STATUS.get(code) or "?"
        super().__init__(f"frame {frame}: jpeg error {code} ({what})")
        self.frame, self.code = frame, code


class _Huff(_C.Structure):
    _fields_ = [("bits", _C.c_uint8 * 16), ("vals", _C.c_uint8 * 256)]


class JpegInfo(_C.Structure):
    """include/mq_hip.h mq_jpeg_info."""
    _fields_ = [("height", _C.c_int32), ("width", _C.c_int32), ("n_comp", _C.c_int32), ("h_luma", _C.c_int32),
                ("v_luma", _C.c_int32), ("restart_interval", _C.c_int32), ("scan_offset", _C.c_int64),
                ("quant", (_C.c_uint8 * 64) * 3), ("dc_sel", _C.c_uint8 * 3), ("ac_sel", _C.c_uint8 * 3),
                ("reserved", _C.c_uint8 * 2), ("dc", _Huff * 2), ("ac", _Huff * 2)]


assert _C.sizeof(JpegInfo) == 1320


def parse_header(data, frame=0):
    """``JpegInfo`` of one stream (host only, no device); ``JpegError`` with the parser's code otherwise."""
    from . import _lib
    data = bytes(data)
    info = JpegInfo()
    rc = _lib.load().mq_jpeg_parse(data, len(data), _C.byref(info))
    if rc:
        raise JpegError(frame, rc)
    return info


class JpegDecoder:
    """``decode(streams)`` -> uint8 (N, H, W, 3) BGR of ``list[bytes]`` baseline JPEG streams (csrc/jpeg_dec.hip).
    Only the compressed bytes cross the bus.  No CPU fallback."""

    def __init__(self, device=0):
        import torch

        from . import _lib
        self.device = device
        self.dev = torch.device("cuda", device)
        self._lib = _lib
        self.ctx = _lib.Context.get(device)

    def decode_into(self, dev_streams, dev_sizes, info, out, status):
        """The entry point on caller-owned device tensors: ``dev_streams`` uint8 (N, stream_stride) whose rows share
        the header ``info`` (rows contiguous; ``stride(0)`` is the stream stride, so a column slice of a wider
        tensor is fine), ``dev_sizes`` int32 (N,) with every size at most the row length, ``out`` uint8 (N, frame_stride >= H * W * 3) or (N, H, W, 3) with
        contiguous rows, ``status`` int32 (N,).  Nothing is copied to the host."""
        import torch
        L = self._lib
        n = int(dev_streams.shape[0])
        if n == 0:
            return out, status
        for name, t, dt in (("dev_streams", dev_streams, torch.uint8), ("dev_sizes", dev_sizes, torch.int32),
                            ("out", out, torch.uint8), ("status", status, torch.int32)):
            if not torch.is_tensor(t) or t.dtype != dt or t.device != self.dev:
                raise ValueError(f"{name} must be a {dt} tensor on {self.dev}")
        if dev_streams.ndim != 2 or dev_streams.stride(1) != 1:
            raise ValueError("dev_streams must be (N, stream_stride) with contiguous rows")
        if out.ndim < 2 or out.shape[0] != n or not out[0].is_contiguous():
            raise ValueError("out must hold N rows of contiguous bytes")     # a row below one frame: -2 from the call
        for name, t in (("dev_sizes", dev_sizes), ("status", status)):
            if tuple(t.shape) != (n,) or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous ({n},) tensor")
        L.check(self.ctx.lib.mq_jpeg_decode(
            self.ctx.handle, L.ptr(dev_streams), dev_streams.stride(0), L.ptr(dev_sizes), n, _C.byref(info),
            L.ptr(out), out.stride(0), L.ptr(status), L.stream_ptr(self.dev)), "mq_jpeg_decode")
        return out, status

    def decode_device(self, streams):
        """uint8 (N, H, W, 3) device tensor.  Frames are grouped by identical header bytes, one call per group;
        ``JpegError`` names the first frame that is refused or does not decode."""
        import torch
        streams = [bytes(s) for s in streams]
        infos = [parse_header(s, i) for i, s in enumerate(streams)]
        if not streams:
            return torch.zeros((0, 0, 0, 3), dtype=torch.uint8, device=self.dev)
        H, W = infos[0].height, infos[0].width
        groups = {}
        for i, (s, info) in enumerate(zip(streams, infos)):
            if (info.height, info.width) != (H, W):
                raise ValueError(f"frame {i} is {info.height} x {info.width}, frame 0 is {H} x {W}")
            groups.setdefault(s[:info.scan_offset], []).append(i)
        out = torch.empty((len(streams), H, W, 3), dtype=torch.uint8, device=self.dev)
        status = np.zeros(len(streams), dtype=np.int32)
        for idx in groups.values():
            stride = (max(len(streams[i]) for i in idx) + 15) // 16 * 16
            host = np.zeros((len(idx), stride), dtype=np.uint8)
            for r, i in enumerate(idx):
                host[r, :len(streams[i])] = np.frombuffer(streams[i], dtype=np.uint8)
            dev = torch.from_numpy(host).to(self.dev)
            sizes = torch.tensor([len(streams[i]) for i in idx], dtype=torch.int32, device=self.dev)
            part = out if len(groups) == 1 else torch.empty((len(idx), H, W, 3), dtype=torch.uint8, device=self.dev)
            st = torch.zeros((len(idx),), dtype=torch.int32, device=self.dev)
            self.decode_into(dev, sizes, infos[idx[0]], part, st)
            if part is not out:
                out[torch.tensor(idx, device=self.dev)] = part
            status[idx] = st.cpu().numpy()
        bad = np.flatnonzero(status)
        if len(bad):
            raise JpegError(int(bad[0]), int(status[bad[0]]))
        return out

    def decode(self, streams):
        return self.decode_device(streams).cpu().numpy()
