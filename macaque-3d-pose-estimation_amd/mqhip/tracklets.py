"""Step-3 tracklet lift on MI355X (``src/pipeline/step3_crossframematching.py`` of the reference).

The reference lifts a tracklet's 3D trace one (tracklet, frame) cell at a time: ``calc_3dtrace``
(:274-302) and ``get_graph``'s ``calc_p3d`` (:1115-1130) loop in Python over the rows of every camera,
undistort, and solve a pinv DLT of 17 joints; ``count_id_detections`` (:839-870) is a second loop of the
same shape.  Here step 1's rows are packed once into CSR arrays (``pack_rows``) and one launch of
``mq_tracklet_traces`` / ``mq_tracklet_id_votes`` serves every cell of a stage.  No CPU fallback.
"""
from __future__ import annotations

import numpy as np

THR_KP = 0.3    # step3:267
CONF_THR = 0.8  # step3:28 cid_thr
N_CLASS = 6     # step3:841 classnames


class PackedRows:
    """Step 1's rows of every camera as CSR arrays: ``row_start`` int32 (C, F + 1), and per row ``tid`` int32,
    ``kp`` float64 (J, 3), ``cls`` int32, ``score`` float64."""

    def __init__(self, row_start, tid, kp, cls, score):
        self.row_start = np.ascontiguousarray(row_start, dtype=np.int32)
        self.tid = np.ascontiguousarray(tid, dtype=np.int32)
        self.kp = np.ascontiguousarray(kp, dtype=np.float64)
        self.cls = np.ascontiguousarray(cls, dtype=np.int32)
        self.score = np.ascontiguousarray(score, dtype=np.float64)
        self.n_cam, self.n_frame = self.row_start.shape[0], self.row_start.shape[1] - 1
        self.n_kp = self.kp.shape[1]
        assert self.kp.shape == (len(self.tid), self.n_kp, 3)
        assert np.all(np.diff(self.row_start.ravel()) >= 0) and self.row_start[-1, -1] == len(self.tid)

    def digest(self):
        """SHA-256 over the packed arrays (what a fixture records of its inputs)."""
        import hashlib
        h = hashlib.sha256()
        for a in (self.row_start, self.tid, self.kp, self.cls, self.score):
            h.update(a.tobytes())
        return h.hexdigest()


def pack_rows(rows, n_kp=None) -> PackedRows:
    """``rows``: the ``T[c][f]`` lists of alldata.json ([tid, x1, y1, x2, y2, kp, id, id score] per row),
    or one ``step1_proc2d.CameraRows`` per camera, or a ``PackedRows`` (returned as is).  ``n_kp``: the joint
    count, taken from the first row when not given (17 when there is no row)."""
    if isinstance(rows, PackedRows):
        return rows
    if n_kp is None:
        n_kp = 17
        for cam in rows:
            if hasattr(cam, "offsets"):
                if np.ndim(cam.kp) == 3 and len(cam.kp):
                    n_kp = np.shape(cam.kp)[1]
                    break
                continue
            first = next((row for frame in cam for row in frame), None)
            if first is not None:
                n_kp = len(first[5])
                break
    n_cam = len(rows)
    n_frame = max(len(r) for r in rows)
    start = np.zeros((n_cam, n_frame + 1), dtype=np.int64)
    tid, kp, cls, score = [], [], [], []
    base = 0
    for c, cam in enumerate(rows):
        if hasattr(cam, "offsets"):   # CameraRows
            off = np.asarray(cam.offsets, dtype=np.int64)
            start[c, :len(off)] = base + off
            start[c, len(off):] = base + off[-1]
            tid.append(np.asarray(cam.tid, dtype=np.int64))
            kp.append(np.asarray(cam.kp, dtype=np.float64).reshape(-1, n_kp, 3))
            cls.append(np.asarray(cam.assigned, dtype=np.int64))
            score.append(np.asarray(cam.score, dtype=np.float64))
            base += int(off[-1])
            continue
        t, k, a, s = [], [], [], []
        for f in range(n_frame):
            start[c, f] = base + len(t)
            for row in (cam[f] if f < len(cam) else ()):
                t.append(int(row[0]))
                k.append(row[5])
                a.append(int(row[6]))
                s.append(float(row[7]))
        start[c, n_frame] = base + len(t)
        base += len(t)
        tid.append(np.asarray(t, dtype=np.int64))
        kp.append(np.asarray(k, dtype=np.float64).reshape(-1, n_kp, 3))
        cls.append(np.asarray(a, dtype=np.int64))
        score.append(np.asarray(s, dtype=np.float64))
    assert base < 2 ** 31
    return PackedRows(start, np.concatenate(tid), np.concatenate(kp), np.concatenate(cls), np.concatenate(score))


def trk_array(Trk, n_frame, n_cam):
    """{k: (F', C)} (or an array (K, F', C)) -> (keys, int32 (K, n_frame, C)); frames past F' are -1."""
    if isinstance(Trk, dict):
        keys = list(Trk.keys())
        mats = [np.asarray(Trk[k]) for k in keys]
    else:
        mats = list(np.asarray(Trk))
        keys = list(range(len(mats)))
    out = np.full((len(mats), n_frame, n_cam), -1, dtype=np.int32)
    for i, m in enumerate(mats):
        assert m.shape[1] == n_cam, "Trk and the rows disagree on the camera count"
        n = min(n_frame, m.shape[0])
        out[i, :n] = m[:n]
    return keys, out


def interval_cells(trk):
    """Every frame inside each tracklet's interval (first .. last frame with a box in any camera)."""
    cells = []
    for i in range(trk.shape[0]):
        on = np.nonzero((trk[i] >= 0).any(axis=1))[0]
        if len(on):
            f = np.arange(on[0], on[-1] + 1)
            cells.append(np.stack([np.full_like(f, i), f], axis=1))
    return np.concatenate(cells).astype(np.int32) if cells else np.zeros((0, 2), dtype=np.int32)


def lift_camera_rows(cams):
    """The (C, 24) camera rows of the lift: intrinsics of ``cams.proj`` (what the undistortion reads) with
    R, t of ``cams.pmat`` (what the pinv DLT reads) -- the two views step 3 takes of one camparam."""
    rows = np.stack([c.param_row() for c in cams.proj.cameras])
    ext = np.stack([c.param_row() for c in cams.pmat.cameras])
    rows[:, 10:22] = ext[:, 10:22]
    return rows


class TrackletLift:
    """Step 1's rows and the cameras on the device, for the launches of one ``main_proc``."""

    def __init__(self, cams, rows, device=None):
        import torch

        from . import _lib
        self.rows = pack_rows(rows)
        self.device = cams.proj.device if device is None else device
        self._lib = _lib
        self.ctx = _lib.Context.get(self.device)
        self.dev = torch.device("cuda", self.device)
        assert cams.n_cam == self.rows.n_cam, "cameras and rows disagree on the camera count"
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.cams_d = up(lift_camera_rows(cams))
        r = self.rows
        self.start_d, self.tid_d, self.kp_d, self.cls_d, self.score_d = (up(r.row_start), up(r.tid), up(r.kp),
                                                                       up(r.cls), up(r.score))
        self.launches = 0

    def _cells(self, Trk, cells):
        import torch
        r = self.rows
        keys, trk = trk_array(Trk, r.n_frame, r.n_cam)
        full = cells is None
        cells = interval_cells(trk) if full else np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 2)
        assert np.all((cells[:, 0] >= 0) & (cells[:, 0] < len(keys)) & (cells[:, 1] >= 0)
                      & (cells[:, 1] < r.n_frame)), "cell out of range"
        return keys, trk, cells, full, torch.from_numpy(trk).to(self.dev), torch.from_numpy(cells).to(self.dev)

    def traces(self, Trk, cells=None, thr_kp=THR_KP, return_p3d=False):
        """(median, mean) of the lifted joints per cell.  ``cells`` None: every frame inside each tracklet's
        interval, returned as (K, F, 3) arrays in Trk's order (NaN elsewhere); else (N, 3) per given (k, f)."""
        import torch
        L, r = self._lib, self.rows
        keys, trk, cells, full, trk_d, cells_d = self._cells(Trk, cells)
        N = len(cells)
        med = torch.full((N, 3), float("nan"), dtype=torch.float64, device=self.dev)
        avg = torch.full((N, 3), float("nan"), dtype=torch.float64, device=self.dev)
        p3d = torch.full((N, r.n_kp, 3), float("nan"), dtype=torch.float64, device=self.dev) if return_p3d else None
        if N:
            L.check(self.ctx.lib.mq_tracklet_traces(
                self.ctx.handle, L.ptr(self.cams_d), r.n_cam, L.ptr(self.start_d), L.ptr(self.tid_d), L.ptr(self.kp_d),
                len(r.tid), r.n_frame, r.n_kp, L.ptr(trk_d), trk.shape[0], L.ptr(cells_d), N, float(thr_kp),
                L.ptr(p3d), L.ptr(med), L.ptr(avg), L.stream_ptr(self.dev)), "mq_tracklet_traces")
            self.launches += 1
        med, avg = med.cpu().numpy(), avg.cpu().numpy()
        if full:
            M = np.full((len(keys), r.n_frame, 3), np.nan)
            A = np.full((len(keys), r.n_frame, 3), np.nan)
            M[cells[:, 0], cells[:, 1]] = med
            A[cells[:, 0], cells[:, 1]] = avg
            med, avg = M, A
        return (med, avg, p3d.cpu().numpy()) if return_p3d else (med, avg)

    def id_votes(self, Trk, cells=None, conf_thr=CONF_THR, n_class=N_CLASS):
        """count_id_detections' votes int (N, n_class) per cell ((K, F, n_class) with ``cells`` None)."""
        import torch
        L, r = self._lib, self.rows
        keys, trk, cells, full, trk_d, cells_d = self._cells(Trk, cells)
        N = len(cells)
        votes = torch.zeros((N, n_class), dtype=torch.int32, device=self.dev)
        if N:
            L.check(self.ctx.lib.mq_tracklet_id_votes(
                self.ctx.handle, r.n_cam, L.ptr(self.start_d), L.ptr(self.tid_d), L.ptr(self.cls_d),
                L.ptr(self.score_d), len(r.tid), r.n_frame, L.ptr(trk_d), trk.shape[0], L.ptr(cells_d), N,
                float(conf_thr), int(n_class), L.ptr(votes), L.stream_ptr(self.dev)), "mq_tracklet_id_votes")
            self.launches += 1
        votes = votes.cpu().numpy().astype(np.int64)
        if full:
            V = np.zeros((len(keys), r.n_frame, n_class), dtype=np.int64)
            V[cells[:, 0], cells[:, 1]] = votes
            votes = V
        return votes


def traces(cams, rows, Trk, cells=None, thr_kp=THR_KP):
    """``TrackletLift(cams, rows).traces(Trk, cells)``: cams a ``mqhip.association.StepTwoCameras``."""
    return TrackletLift(cams, rows).traces(Trk, cells, thr_kp=thr_kp)


def id_votes(cams, rows, Trk, cells=None, conf_thr=CONF_THR, n_class=N_CLASS):
    return TrackletLift(cams, rows).id_votes(Trk, cells, conf_thr=conf_thr, n_class=n_class)
