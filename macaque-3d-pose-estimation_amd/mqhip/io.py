"""On-disk formats around the hot path.

* ``kp2d.pickle`` / ``kp2d_f.pickle`` / ``kp3d.pickle``: the reference pickles plain
  numpy arrays and dicts of them (step4:151-170, :332-339).  ``load_array_pickle``
  reads them with an allow-list unpickler that can only rebuild numpy arrays,
  dtypes and builtin containers -- nothing else in the file can execute.
* ``calibration.toml`` / ``config.toml``: read with tomli; ``dump_toml`` writes the
  subset of TOML the reference's ``toml.dump`` produces for these files (tables of
  strings, numbers, booleans and nested lists).
* ``alldata.json`` / ``frame_num.npy`` (step1_proc2d.py:364-375): plain JSON / npy.
* ``FrameStore``: the per-camera frame source of step 1 (stands in for imgstore): raw ``frames.npy`` (``format:
  npy``) or a Motion-JPEG ``frames.avi`` decoded on the GPU (``format: mjpeg``, ``convert_frame_store`` writes one).
* ``MjpegAviWriter`` / ``MjpegAviReader``: the Motion-JPEG AVI the overlay stage writes with ``video='avi'``.
"""
from __future__ import annotations

import io
import json
import os
import pickle

import numpy as np

_ALLOWED = {
    ("numpy.core.multiarray", "_reconstruct"),
    ("numpy._core.multiarray", "_reconstruct"),
    ("numpy.core.multiarray", "scalar"),
    ("numpy._core.multiarray", "scalar"),
    ("numpy", "ndarray"),
    ("numpy", "dtype"),
    ("builtins", "list"),
    ("builtins", "dict"),
    ("builtins", "tuple"),
    ("collections", "OrderedDict"),
}


class _ArrayUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if (module, name) in _ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"refusing to load {module}.{name} from a keypoint pickle")


def load_array_pickle(path):
    """Load a pickle holding numpy arrays / dicts / lists only."""
    with open(path, "rb") as f:
        return _ArrayUnpickler(io.BytesIO(f.read())).load()


def dump_pickle(obj, path):
    with open(path, "wb") as f:
        pickle.dump(obj, f)


def load_toml(path):
    try:
        import tomllib as _toml  # py >= 3.11
    except ImportError:  # pragma: no cover - py3.10 image
        import tomli as _toml
    with open(path, "rb") as f:
        return _toml.load(f)


def _val(v):
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    if isinstance(v, (float, np.floating)):
        v = float(v)
        if v != v:
            return "nan"
        if v in (float("inf"), float("-inf")):
            return "inf" if v > 0 else "-inf"
        return repr(v)
    if isinstance(v, str):
        return '"' + v.replace("\\", "\\\\").replace('"', '\\"') + '"'
    if isinstance(v, np.ndarray):
        v = v.tolist()
    if isinstance(v, (list, tuple)):
        return "[ " + ", ".join(_val(x) for x in v) + ",]" if len(v) else "[]"
    raise TypeError(f"cannot write {type(v)} to TOML")


def dump_toml(data: dict, path):
    """Top-level scalars first, then one [table] per dict value (one nesting level)."""
    lines = []
    for k, v in data.items():
        if not isinstance(v, dict):
            lines.append(f"{k} = {_val(v)}")
    for k, v in data.items():
        if isinstance(v, dict):
            lines.append("")
            lines.append(f"[{k}]")
            for kk, vv in v.items():
                if isinstance(vv, dict):
                    raise TypeError("nested tables are not used by these files")
                lines.append(f"{kk} = {_val(vv)}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


# ----------------------------------------------------------------------------- frame stores
class FrameStore:
    """One camera's synchronized frames plus the detector/tracker output for them.

    Stands in for the reference's imgstore (``imgstore.new_for_filename(<raw>/<data>.<cam>/
    metadata.yaml)``, step1_proc2d.py:403-408), which is not installable here and mostly decodes H.264,
    which this build does not handle (its Motion-JPEG store format is what ``format: mjpeg`` mirrors).  Directory
    layout (``write_frame_store`` makes an ``npy`` one, ``convert_frame_store`` an ``mjpeg`` one from it):

      metadata.yaml     imgstore-style metadata (camera id, image size); its presence is what
                        step 1 globs for, exactly like the reference
      frames.npy        uint8 (N, H, W, 3) BGR, memory-mapped (never loaded whole) -- stores of ``format: npy``
      frames.avi        stores of ``format: mjpeg`` instead: the same images as baseline JPEG frames of a
                        Motion-JPEG AVI (and its rollover files); ``frames`` is then an ``MjpegFrames`` that decodes
                        on the GPU (``decoder``: a factory ``(device=)`` of an object with ``JpegDecoder.decode``;
                        tests inject the NumPy decoder) on ``device``, so only compressed bytes cross the disk
                        and the bus
      frame_time.npy    float64 (N,)  -- get_frame_metadata()["frame_time"]
      frame_number.npy  int64 (N,)    -- get_frame_metadata()["frame_number"]
      tracks.json       per stored frame, the tracker rows [x1, y1, x2, y2, track_id, ...] that the
                        out-of-scope Swin detector + BoT-SORT produce (step1_proc2d.py:226-252)
      id_preds.json     optional: per stored frame, per row {"pred_label", "pred_score"} of the
                        ResNet-152 ID classifier (step1_proc2d.py:140-163)
      frame_index.npy   optional int64 (N,): frame i is frames.npy[frame_index[i]] -- synthetic clips
                        reuse a small pool of rendered images so a 300-frame x 8-view clip at the
                        cameras' 2048x1536 stays a few hundred MB on disk
    """

    def __init__(self, directory, decoder=None, device=0):
        self.filename = str(directory)
        meta = os.path.join(directory, "metadata.yaml")
        if not os.path.exists(meta):
            raise FileNotFoundError(meta)
        self.format = _store_format(meta)
        if self.format == "mjpeg":
            self.frames = MjpegFrames(os.path.join(directory, "frames.avi"), decoder=decoder, device=device)
        elif self.format == "npy":
            self.frames = np.load(os.path.join(directory, "frames.npy"), mmap_mode="r")
        else:
            raise ValueError(f"{directory}: unknown store format {self.format!r}")
        self.frame_time = np.load(os.path.join(directory, "frame_time.npy"))
        self.frame_number = np.load(os.path.join(directory, "frame_number.npy"))
        with open(os.path.join(directory, "tracks.json")) as f:
            self.tracks = json.load(f)
        idp = os.path.join(directory, "id_preds.json")
        self.id_preds = None
        if os.path.exists(idp):
            with open(idp) as f:
                self.id_preds = json.load(f)
        fi = os.path.join(directory, "frame_index.npy")
        self.frame_index = np.load(fi) if os.path.exists(fi) else np.arange(len(self.frames))
        if len(self.frame_index) and (self.frame_index.min() < 0 or self.frame_index.max() >= len(self.frames)):
            raise ValueError(f"{directory}: frame_index out of range")
        if not (len(self.frame_index) == len(self.frame_time) == len(self.frame_number) == len(self.tracks)):
            raise ValueError(f"{directory}: frames, times, numbers and tracks differ in length")
        self._pos = {int(n): i for i, n in enumerate(self.frame_number)}

    def get_frame_metadata(self):
        return {"frame_time": self.frame_time, "frame_number": self.frame_number}

    def index_of(self, frame_number):
        return self._pos[int(frame_number)]

    def image(self, frame_number):
        return np.asarray(self.frames[self.frame_index[self.index_of(frame_number)]])

    def tracks_of(self, frame_number):
        return self.tracks[self.index_of(frame_number)]

    def id_preds_of(self, frame_number):
        return None if self.id_preds is None else self.id_preds[self.index_of(frame_number)]


def _store_format(meta_path):
    import yaml
    with open(meta_path) as f:
        meta = yaml.safe_load(f) or {}
    return str((meta.get("__store") or {}).get("format", "npy"))


def _gpu_decoder(device=0):
    from .mjpeg import JpegDecoder
    return JpegDecoder(device=device)


def _gpu_encoder(height, width, quality=90, restart_interval=16, device=0):
    from .mjpeg import JpegEncoder
    return JpegEncoder(height, width, quality=quality, restart_interval=restart_interval, device=device)


class MjpegFrames:
    """The image pool of a ``format: mjpeg`` store: what ``frames.npy``'s memory map is to an ``npy`` store.
    ``shape`` (pool, H, W, 3), ``dtype``, ``len()``; ``frames[i]`` decodes image i to a uint8 (H, W, 3) BGR array
    (a small LRU keeps the last ``cache`` decoded images: step 1 asks for the same image three times);
    ``device_frames(indices)`` decodes a batch and leaves it on the device.  The decoder is made on first use."""

    dtype = np.dtype(np.uint8)

    def __init__(self, path, decoder=None, device=0, cache=8):
        from collections import OrderedDict
        self.readers = [MjpegAviReader(p) for p in mjpeg_avi_files(path)]
        self._at = [(r, i) for r in self.readers for i in range(len(r))]
        H, W = self.readers[0].height, self.readers[0].width
        if any((r.height, r.width) != (H, W) for r in self.readers):
            raise ValueError(f"{path}: the rollover files differ in frame size")
        self.shape = (len(self._at), H, W, 3)
        self.ndim = 4
        self.device = device
        self._factory, self._decoder = decoder or _gpu_decoder, None
        self._cache, self._cache_size = OrderedDict(), max(1, int(cache))

    def __len__(self):
        return self.shape[0]

    def frame_bytes(self, i):
        r, k = self._at[int(i)]
        return r.frame_bytes(k)

    def _dec(self):
        if self._decoder is None:
            self._decoder = self._factory(device=self.device)
        return self._decoder

    def __getitem__(self, i):
        if not isinstance(i, (int, np.integer)):
            raise TypeError("an MjpegFrames is indexed by one integer (use device_frames for a batch)")
        i = int(i)
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        if i in self._cache:
            self._cache.move_to_end(i)
            return self._cache[i]
        img = np.asarray(self._dec().decode([self.frame_bytes(i)]))[0]
        if img.shape != self.shape[1:]:
            raise ValueError(f"frame {i} is {img.shape}, the store is {self.shape[1:]}")
        img.setflags(write=False)
        self._cache[i] = img
        if len(self._cache) > self._cache_size:
            self._cache.popitem(last=False)
        return img

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __array__(self, dtype=None, copy=None):
        out = np.stack([self[i] for i in range(len(self))]) if len(self) else np.zeros(self.shape, np.uint8)
        return out if dtype is None else out.astype(dtype)

    def device_frames(self, indices, device=None):
        """uint8 (len(indices), H, W, 3) on the device: only the compressed bytes are uploaded."""
        if device is not None and device != self.device and self._decoder is not None:
            self._decoder = None
        if device is not None:
            self.device = device
        return self._dec().decode_device([self.frame_bytes(i) for i in indices])


def convert_frame_store(src, dst, quality=90, restart_interval=16, batch=16, encoder=None, device=0,
                        max_bytes=2 ** 31 - 2 ** 20):
    """Write the ``format: mjpeg`` store ``dst`` of the ``npy`` store ``src``: the image pool encoded on the GPU
    (``encoder``: a factory ``(height, width, quality=, restart_interval=, device=)`` of an object with
    ``JpegEncoder.encode``; tests inject the NumPy encoder) into ``dst/frames.avi`` (rollover files past
    ``max_bytes``), the times, numbers, tracker rows, ID predictions and frame index copied.  JPEG is lossy: the
    new store's images are the decoded ones.  Returns (raw bytes, compressed bytes)."""
    import shutil

    import yaml
    store = FrameStore(src)
    if store.format != "npy":
        raise ValueError(f"{src}: not a format: npy store")
    if os.path.exists(os.path.join(dst, "metadata.yaml")):
        raise FileExistsError(os.path.join(dst, "metadata.yaml"))
    os.makedirs(dst, exist_ok=True)
    n, H, W = (int(v) for v in store.frames.shape[:3])
    enc = (encoder or _gpu_encoder)(H, W, quality=quality, restart_interval=restart_interval, device=device)
    writer = MjpegAviWriter(os.path.join(dst, "frames.avi"), H, W, max_bytes=max_bytes)
    total = 0
    for k in range(0, n, max(1, int(batch))):
        for jpg in enc.encode(np.array(store.frames[k:k + max(1, int(batch))])):      # a writable copy of the map
            writer.append(jpg)
            total += len(jpg)
    writer.close()
    for name in ("frame_time.npy", "frame_number.npy", "tracks.json", "id_preds.json", "frame_index.npy"):
        if os.path.exists(os.path.join(src, name)):
            shutil.copyfile(os.path.join(src, name), os.path.join(dst, name))
    with open(os.path.join(src, "metadata.yaml")) as f:
        meta = yaml.safe_load(f) or {}
    meta.setdefault("__store", {})
    meta["__store"].update(format="mjpeg", imgshape=[H, W, 3], quality=int(quality),
                           restart_interval=int(restart_interval))
    with open(os.path.join(dst, "metadata.yaml"), "w") as f:      # last: its presence makes the directory a store
        yaml.safe_dump(meta, f)
    return n * H * W * 3, total


def write_frame_store(directory, frames, frame_time, frame_number, tracks, camera_id, id_preds=None,
                      frame_index=None):
    """Write a FrameStore directory (used by tests and synthetic runs).  With ``frame_index`` the
    ``frames`` are a pool of images and frame i shows ``frames[frame_index[i]]``."""
    import yaml
    os.makedirs(directory, exist_ok=True)
    frames = np.asarray(frames, dtype=np.uint8)
    with open(os.path.join(directory, "metadata.yaml"), "w") as f:
        yaml.safe_dump({"__store": {"camera_id": str(camera_id), "imgshape": list(frames.shape[1:]),
                                    "format": "npy"}}, f)
    np.save(os.path.join(directory, "frames.npy"), frames)
    np.save(os.path.join(directory, "frame_time.npy"), np.asarray(frame_time, dtype=np.float64))
    np.save(os.path.join(directory, "frame_number.npy"), np.asarray(frame_number, dtype=np.int64))
    with open(os.path.join(directory, "tracks.json"), "w") as f:
        json.dump([[list(map(float, r)) for r in t] for t in tracks], f)
    if id_preds is not None:
        with open(os.path.join(directory, "id_preds.json"), "w") as f:
            json.dump(id_preds, f)
    if frame_index is not None:
        np.save(os.path.join(directory, "frame_index.npy"), np.asarray(frame_index, dtype=np.int64))


class FrameStoreWriter:
    """Write a FrameStore directory batch by batch: ``frames.npy`` is created at its final size with
    ``np.lib.format.open_memmap`` and filled by ``append``, so a clip larger than memory streams through.
    The tracker rows are empty.  ``metadata.yaml`` -- the file whose presence makes the directory a store -- is
    written by ``close`` only, after every announced frame has arrived."""

    def __init__(self, directory, n_frames, height, width, camera_id):
        os.makedirs(directory, exist_ok=True)
        self.directory, self.camera_id = str(directory), camera_id
        self.n, self.pos = int(n_frames), 0
        self.shape = (int(height), int(width), 3)
        self.frames = np.lib.format.open_memmap(os.path.join(directory, "frames.npy"), mode="w+", dtype=np.uint8,
                                                shape=(self.n,) + self.shape)
        self.frame_number = np.zeros(self.n, dtype=np.int64)
        self.frame_time = np.zeros(self.n, dtype=np.float64)

    def append(self, frames, frame_number, frame_time):
        frames = np.asarray(frames)
        k = len(frames)
        if frames.dtype != np.uint8 or frames.shape[1:] != self.shape:
            raise ValueError(f"frames must be uint8 (k,) + {self.shape}, got {frames.dtype} {frames.shape}")
        if self.pos + k > self.n or len(frame_number) != k or len(frame_time) != k:
            raise ValueError("more frames than announced, or numbers / times of another length")
        self.frames[self.pos:self.pos + k] = frames
        self.frame_number[self.pos:self.pos + k] = frame_number
        self.frame_time[self.pos:self.pos + k] = frame_time
        self.pos += k

    def close(self):
        import yaml
        if self.pos != self.n:
            raise ValueError(f"{self.directory}: {self.pos} of {self.n} announced frames were written")
        self.frames.flush()
        del self.frames
        d = self.directory
        np.save(os.path.join(d, "frame_time.npy"), self.frame_time)
        np.save(os.path.join(d, "frame_number.npy"), self.frame_number)
        with open(os.path.join(d, "tracks.json"), "w") as f:
            json.dump([[] for _ in range(self.n)], f)
        with open(os.path.join(d, "metadata.yaml"), "w") as f:
            yaml.safe_dump({"__store": {"camera_id": str(self.camera_id), "imgshape": list(self.shape),
                                        "format": "npy"}}, f)


# ----------------------------------------------------------------------------- Motion-JPEG AVI
_AVIF_HASINDEX = 0x10
_AVIIF_KEYFRAME = 0x10
_AVI_MOVI_FOURCC_AT = 220      # RIFF 12 + LIST hdrl 12 + avih 64 + LIST strl 12 + strh 64 + strf 48 + LIST movi 8


def mjpeg_avi_files(path):
    """The files of one recording in order: ``path`` and its rollover files ``<stem>.001.avi``, ..."""
    stem, out, k = os.path.splitext(str(path))[0], [str(path)], 1
    while os.path.exists(f"{stem}.{k:03d}.avi"):
        out.append(f"{stem}.{k:03d}.avi")
        k += 1
    return out


class MjpegAviWriter:
    """Motion-JPEG AVI (AVI 1.0, one ``vids`` / ``MJPG`` stream, ``idx1`` index); every frame is a complete JPEG.

      RIFF 'AVI ' | LIST hdrl ( avih 56 bytes, AVIF_HASINDEX | LIST strl ( strh 56 bytes | strf 40 bytes ) )
                  | LIST movi ( 00dc chunks, padded to even length ) | idx1 (16 bytes per frame: 00dc,
                    AVIIF_KEYFRAME, offset from the movi fourcc, size)

    Sizes and counts are patched by ``close``.  A file that the next frame would take past ``max_bytes`` is closed
    and writing continues in ``<stem>.001.avi``, ``<stem>.002.avi``, ... (AVI 1.0 sizes are 32 bits; OpenDML is not
    written).  Frame numbers / times given to ``append`` are written by ``close`` as ``<stem>.frame_number.npy`` /
    ``<stem>.frame_time.npy`` beside the first file (the frame mapping a frame store keeps)."""

    def __init__(self, path, height, width, fps=24.0, max_bytes=2 ** 31 - 2 ** 20):
        from fractions import Fraction
        path = str(path)
        if not path.endswith(".avi"):
            raise ValueError(f"path must end in .avi, got {path}")
        if not (1 <= int(height) <= 65535 and 1 <= int(width) <= 65535):
            raise ValueError("height and width must be in [1, 65535]")
        if not float(fps) > 0:
            raise ValueError(f"fps must be positive, got {fps}")
        if not _AVI_MOVI_FOURCC_AT + 4 < int(max_bytes) < 2 ** 32:
            raise ValueError("max_bytes must be in (224, 2^32)")
        self.path, self.stem = path, path[:-4]
        self.H, self.W, self.fps, self.max_bytes = int(height), int(width), float(fps), int(max_bytes)
        rate = Fraction(self.fps).limit_denominator(100000)
        self.rate, self.scale = rate.numerator, rate.denominator
        self.paths, self.n_total = [], 0
        self.frame_number, self.frame_time = [], []
        self._f = None
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self._open()

    def _header(self, n_frames, movi_bytes, max_chunk):
        import struct
        avih = struct.pack("<14I", int(round(1e6 * self.scale / self.rate)), 0, 0, _AVIF_HASINDEX, n_frames, 0, 1,
                           max_chunk, self.W, self.H, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, n_frames,
                           max_chunk, 0xFFFFFFFF, 0, 0, 0, min(self.W, 32767), min(self.H, 32767))
        strf = struct.pack("<IiiHH4sIiiII", 40, self.W, self.H, 1, 24, b"MJPG", self.W * self.H * 3, 0, 0, 0, 0)
        chunk = lambda cc, d: cc + struct.pack("<I", len(d)) + d
        strl = b"LIST" + struct.pack("<I", 4 + 64 + 48) + b"strl" + chunk(b"strh", strh) + chunk(b"strf", strf)
        hdrl = b"LIST" + struct.pack("<I", 4 + 64 + len(strl)) + b"hdrl" + chunk(b"avih", avih) + strl
        riff = 4 + len(hdrl) + 8 + 4 + movi_bytes + 8 + 16 * n_frames
        h = b"RIFF" + struct.pack("<I", riff) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"
        assert len(h) == _AVI_MOVI_FOURCC_AT + 4
        return h

    def _open(self):
        k = len(self.paths)
        p = self.path if k == 0 else f"{self.stem}.{k:03d}.avi"
        self.paths.append(p)
        self._f = open(p, "wb")
        self._f.write(self._header(0, 0, 0))
        self._index, self._movi, self._max_chunk = [], 0, 0      # (offset, size) per frame; bytes of chunks

    def _finish(self):
        import struct
        f = self._f
        f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)))
        for off, size in self._index:
            f.write(struct.pack("<4sIII", b"00dc", _AVIIF_KEYFRAME, off, size))
        f.seek(0)
        f.write(self._header(len(self._index), self._movi, self._max_chunk))
        f.close()
        self._f = None

    def append(self, jpeg_bytes, frame_number=None, frame_time=None):
        import struct
        if self._f is None:
            raise ValueError("the writer is closed")
        data = bytes(jpeg_bytes)
        chunk = 8 + len(data) + (len(data) & 1)
        size_after = _AVI_MOVI_FOURCC_AT + 4 + self._movi + chunk + 8 + 16 * (len(self._index) + 1)
        if size_after > self.max_bytes:
            if not self._index:
                raise ValueError(f"a frame of {len(data)} bytes does not fit a file of max_bytes {self.max_bytes}")
            self._finish()
            self._open()
        self._index.append((4 + self._movi, len(data)))
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + (b"\x00" if len(data) & 1 else b""))
        self._movi += chunk
        self._max_chunk = max(self._max_chunk, len(data))
        self.n_total += 1
        if frame_number is not None:
            self.frame_number.append(int(frame_number))
        if frame_time is not None:
            self.frame_time.append(float(frame_time))

    def close(self):
        if self._f is None:
            return
        self._finish()
        for name, vals, dt in (("frame_number", self.frame_number, np.int64), ("frame_time", self.frame_time,
                                                                               np.float64)):
            if vals:
                if len(vals) != self.n_total:
                    raise ValueError(f"{name} was given for {len(vals)} of {self.n_total} frames")
                np.save(f"{self.stem}.{name}.npy", np.asarray(vals, dtype=dt))


class MjpegAviReader:
    """One file an ``MjpegAviWriter`` wrote, through its ``idx1`` index: ``len()``, ``frame_bytes(i)``, ``fps``,
    ``width``, ``height``.  (``mjpeg_avi_files`` lists a recording's rollover files.)"""

    def __init__(self, path):
        import struct
        self.path = str(path)
        with open(self.path, "rb") as f:
            self._data = f.read()
        d = self._data
        if d[:4] != b"RIFF" or d[8:12] != b"AVI ":
            raise ValueError(f"{path}: not a RIFF AVI file")
        if struct.unpack_from("<I", d, 4)[0] + 8 != len(d):
            raise ValueError(f"{path}: RIFF size does not match the file (not closed?)")
        self.chunks = {}
        self._walk(12, len(d))
        for need in ("avih", "strh", "strf", "movi", "idx1"):
            if need not in self.chunks:
                raise ValueError(f"{path}: no {need} chunk")
        avih = struct.unpack_from("<14I", d, self.chunks["avih"][0])
        strh = struct.unpack_from("<4s4sIHHIIIIIIII4h", d, self.chunks["strh"][0])
        strf = struct.unpack_from("<IiiHH4sIiiII", d, self.chunks["strf"][0])
        if strh[0] != b"vids" or strh[1] != b"MJPG" or strf[5] != b"MJPG":
            raise ValueError(f"{path}: not a Motion-JPEG video stream")
        self.avih, self.strh, self.strf = avih, strh, strf
        self.width, self.height = int(strf[1]), int(strf[2])
        self.fps = strh[7] / strh[6]
        off, size = self.chunks["idx1"]
        self.movi_at = self.chunks["movi"][0] - 4          # the movi fourcc
        self.index = [struct.unpack_from("<4sIII", d, off + 16 * i) for i in range(size // 16)]
        if len(self.index) != avih[4] or len(self.index) != strh[9]:
            raise ValueError(f"{path}: idx1 has {len(self.index)} entries, the headers say {avih[4]} / {strh[9]}")

    def _walk(self, pos, end):
        import struct
        d = self._data
        while pos + 8 <= end:
            cc, size = d[pos:pos + 4], struct.unpack_from("<I", d, pos + 4)[0]
            if cc == b"LIST":
                kind = d[pos + 8:pos + 12].decode("latin1")
                self.chunks[kind] = (pos + 12, size - 4)
                if kind != "movi":
                    self._walk(pos + 12, pos + 8 + size)
            else:
                self.chunks.setdefault(cc.decode("latin1"), (pos + 8, size))
            pos += 8 + size + (size & 1)

    def __len__(self):
        return len(self.index)

    def frame_bytes(self, i):
        import struct
        cc, flags, off, size = self.index[i]
        at = self.movi_at + off
        if self._data[at:at + 4] != b"00dc" or struct.unpack_from("<I", self._data, at + 4)[0] != size:
            raise ValueError(f"{self.path}: idx1 entry {i} does not point at a 00dc chunk of its size")
        return self._data[at + 8:at + 8 + size]
