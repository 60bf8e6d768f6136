"""Step 3 -- ``src/pipeline/step3_crossframematching.py``: cross-frame matching and the kp2d.pickle writer.

The reference's step 3 builds tracklets from step 2's keyframe records, trims and stitches them with a
min-cost flow and votes IDs (step3_crossframematching.py:36-94, 313-402).  What the 3D lift consumes from it
is ``kp2d.pickle``: (A, F, C, J, 3) per-view keypoints of every individual, zero where an individual is not
seen, written by ``create_kp2dfile`` (step3:872-915).  This module has both ways to that file:

* the association itself, under the reference's names (second half of the file): ``proc`` / ``main_proc``
  and their stages, with the per-cell 3D lift and the ID votes on the GPU (``mqhip.tracklets``:
  ``mq_tracklet_traces`` / ``mq_tracklet_id_votes``) and the combinatorial part on the host;
  ``run_demo.proc(association="match")`` runs it after step 2; ``visualize`` (``proc(save_vid=True)``) is its
  tracking video, drawn, resized and encoded on the GPU;
* the writer fed from a KNOWN track -> individual assignment instead (the benchmark's "association
  bypassed" path, SURVEY 8(d), and ``run_demo.proc``'s default):

* ``load_alldata``: step 1's per-camera ``alldata.json`` rows, the T[i_cam][i_frame] of step 3;
* ``known_assignment``: Trk / Cid (step 3's per-track box ids per camera and individual ids)
  from a {track id -> individual} map (default: track id == individual index);
* ``create_kp2dfile``: step3:872-915 (every matching row of a camera is written, so the last one
  stays; zero fill);
* ``proc_known_assignment``: the three above for a results directory.

The reference hard-codes 4 individuals and 8 cameras (step3:879-880); here both come from the
arguments / the camera list of config.yaml, so the 4-view config 1 also runs.
"""
from __future__ import annotations

import json
import os
import pickle

import numpy as np
import yaml

from mqhip import io as mqio


def camera_ids(config_path):
    with open(config_path, "r") as f:
        return [str(i) for i in yaml.safe_load(f)["camera_id"]]


def load_alldata(result_dir, cam_ids):
    """T[i_cam][i_frame] = list of rows [tid, x1, y1, x2, y2, [[x, y, s] x J], id, id_score]."""
    T = []
    for cam in cam_ids:
        with open(os.path.join(result_dir, cam, "alldata.json")) as f:
            T.append(json.load(f))
    return T


def track_ids(T):
    """Per camera, per frame, the track ids of the alldata rows T[i_cam][i_frame]."""
    return [[[int(row[0]) for row in frame] for frame in cam] for cam in T]


def default_track_map(T, n_animal, ids=None):
    """{track id -> individual} for the smallest ``n_animal`` track ids present in the alldata rows, in
    ascending order (synthetic stores number tracks from 0, the BoT-SORT tracker from 1).  ``ids``: the
    rows' track ids (``track_ids``) in place of the rows."""
    ids = track_ids(T) if ids is None else ids
    tids = sorted({t for cam in ids for frame in cam for t in frame})
    if not tids:  # nothing tracked: every individual stays zero-filled
        return {a: a for a in range(n_animal)}
    return {t: a for a, t in enumerate(tids[:n_animal])}


def known_assignment(T, n_animal, track_to_animal=None, ids=None):
    """Trk[k] (F, C) box id of track k in each camera (-1 = absent) and Cid[k] (F,) its individual,
    for a known {track id -> individual} map shared by all cameras (default: ``default_track_map``, the
    ``n_animal`` smallest track ids present -> 0..n_animal-1).  ``ids`` (``track_ids``) may stand in for
    the rows: a rank of a sharded run holds the rows of its own cameras only."""
    ids = track_ids(T) if ids is None else ids
    n_cam = len(ids)
    n_frame = len(ids[0])
    if track_to_animal is None:
        track_to_animal = default_track_map(None, n_animal, ids)
    Trk, Cid = {}, {}
    for tid, a in track_to_animal.items():
        trk = np.full((n_frame, n_cam), -1, dtype=np.int64)
        for c in range(n_cam):
            for f in range(min(n_frame, len(ids[c]))):
                if int(tid) in ids[c][f]:
                    trk[f, c] = int(tid)
        Trk[tid] = trk
        Cid[tid] = np.full(n_frame, int(a), dtype=np.int64)
    return Trk, Cid


def kp2d_of_camera(rows_c, Trk, Cid, i_cam, n_frame, n_animal=4, n_kp=17):
    """Camera ``i_cam``'s slice kp2d[:, :, i_cam] of create_kp2dfile (step3:872-915) from that camera's rows
    alone: the writer touches camera i_cam only through T[i_cam] and Trk[k][:, i_cam], so the cameras can
    be assembled independently (on different ranks) and stacked, with the same bits."""
    out = np.zeros([n_animal, n_frame, n_kp, 3])
    is_done = np.zeros([n_animal, n_frame], dtype=bool)
    for i_frame in range(n_frame):
        for k in Trk.keys():
            i_animal = Cid[k][i_frame]
            if i_animal < 0:
                continue
            trk = Trk[k][i_frame, :]
            if np.sum(trk >= 0) == 0 or is_done[i_animal, i_frame]:
                continue
            for tt in rows_c[i_frame]:
                if tt[0] == trk[i_cam]:
                    out[i_animal, i_frame, :, :] = np.array(tt[5], dtype=np.float64)
                    is_done[i_animal, i_frame] = True
    return out


def kp2d_of_camera_rows(cr, Trk, Cid, i_cam, n_frame, n_animal=4, n_kp=17):
    """``kp2d_of_camera`` from a camera's rows as arrays (``step1_proc2d.CameraRows``): the same selection --
    per frame and track (Trk order) the last row carrying the track's box id -- on the arrays, bit for bit."""
    out = np.zeros([n_animal, n_frame, n_kp, 3])
    is_done = np.zeros([n_animal, n_frame], dtype=bool)
    tid = cr.tid
    for i_frame in range(min(n_frame, len(cr))):
        a0, n = cr.frame(i_frame)
        if n == 0:
            continue
        ft = tid[a0:a0 + n]
        for k in Trk.keys():
            i_animal = Cid[k][i_frame]
            if i_animal < 0:
                continue
            trk = Trk[k][i_frame, :]
            if np.sum(trk >= 0) == 0 or is_done[i_animal, i_frame]:
                continue
            hit = np.nonzero(ft == trk[i_cam])[0]
            if len(hit):
                out[i_animal, i_frame] = cr.kp[a0 + hit[-1]]
                is_done[i_animal, i_frame] = True
    return out


def assemble_kp2d(T, Trk, Cid, n_animal=4, n_kp=17):
    """create_kp2dfile's (A, F, C, J, 3) array without writing it."""
    n_cam = len(T)
    n_frame = Trk[list(Trk.keys())[0]].shape[0]
    kp2d = np.zeros([n_animal, n_frame, n_cam, n_kp, 3])
    for i_cam in range(n_cam):
        kp2d[:, :, i_cam] = kp2d_of_camera(T[i_cam], Trk, Cid, i_cam, n_frame, n_animal, n_kp)
    return kp2d


def create_kp2dfile(result_dir, T, Trk, Cid, n_animal=4, n_kp=17):
    """step3_crossframematching.py:872-915 -> <result_dir>/kp2d.pickle (A, F, C, J, 3): per individual,
    frame and camera the keypoints of the first track (in Trk's order) mapped to that individual that has a
    box in the camera; among that camera's rows carrying the box id, the last one; zero fill."""
    kp2d = assemble_kp2d(T, Trk, Cid, n_animal, n_kp)
    mqio.dump_pickle(kp2d, os.path.join(result_dir, "kp2d.pickle"))
    return kp2d


def kp2d_from_step1(s1out, cam_ids, n_animal=4, n_kp=17, track_to_animal=None, world=1, group=None, device=None):
    """create_kp2dfile's array from step 1's rows in memory (``step1_proc2d.Step1Output``) instead of the
    alldata.json files, in the camera order of config.yaml.  On a sharded run every rank assembles the
    kp2d slices of the cameras it post-processed (``mqhip.shard.camera_shard``) -- the known assignment
    needs only every camera's track ids, which every rank has -- and one all-gather
    (``mqhip.shard.gather_cameras``) gives every rank the whole array.  Same bits as the file path.
    Returns None when the rows do not cover config.yaml's cameras (the caller then reads the files)."""
    if s1out is None or not s1out.complete or any(c not in s1out.names for c in cam_ids):
        return None
    store_of = [s1out.names.index(c) for c in cam_ids]          # store index of each config camera
    pos = {i: p for p, i in enumerate(store_of)}
    ids = [s1out.ids[i] for i in store_of]
    Trk, Cid = known_assignment(None, n_animal, track_to_animal, ids=ids)
    n_frame = len(ids[0])
    n_st = len(s1out.names)
    own = sorted(s1out.rows)
    part = np.zeros((n_animal, n_frame, len(own), n_kp, 3))
    for j, i in enumerate(own):
        if i in pos:
            part[:, :, j] = kp2d_of_camera_rows(s1out.rows[i], Trk, Cid, pos[i], n_frame, n_animal, n_kp)
    if len(own) == n_st and world == 1 and group is None:
        full = part
    else:
        from mqhip.shard import gather_cameras
        full = gather_cameras(part, n_st, world, group=group, device=device)
    return np.ascontiguousarray(full[:, :, store_of])


def proc_known_assignment(data_name, results_dir_root, config_path, n_animal=4, n_kp=17, track_to_animal=None):
    """alldata.json of every camera -> kp2d.pickle through a known track -> individual map."""
    result_dir = os.path.join(results_dir_root, data_name)
    cams = camera_ids(config_path)
    T = load_alldata(result_dir, cams)
    Trk, Cid = known_assignment(T, n_animal, track_to_animal)
    return create_kp2dfile(result_dir, T, Trk, Cid, n_animal=n_animal, n_kp=n_kp)


# ============================================================================= cross-frame matching
#
# The reference's association (step3:36-94): keyframe records of step 2 -> tracklets -> trimming -> ID
# votes -> stitching by a min-cost path cover -> ID clean-up.  The combinatorial stages run on the host in
# NumPy and keep the reference's constants, order and accidents (DESIGN 8.4 lists them); every 3D quantity
# and every ID vote comes from a *lift*: an object with ``traces(Trk, cells=None) -> (median, mean)`` and
# ``id_votes(Trk, cells=None)`` (``mqhip.tracklets.TrackletLift``: one launch per call).  The stages take
# the lift as an argument; that is the only seam (the host tests inject the oracle's per-cell lift).

const_mindetcnt1 = 12
const_mindetcnt2 = 6
cid_thr = 0.80
ID_CLASSES = (0, 2, 3, 5)        # 'B', 'G', 'R', 'W' of classnames ['B', 'd', 'G', 'R', 'unknown', 'W']
TRIM_RMSE_MM = 150.0
LINK_WINDOW = 120
OUT_COST = 1000 * 100


def _interval(trk, min_cams=1):
    """[first, last] frame where the tracklet has a box in at least ``min_cams`` cameras."""
    on = np.argwhere(np.sum(trk >= 0, axis=1) >= min_cams)
    return [int(np.min(on)), int(np.max(on))]


def _intervals(Trk, min_cams=1):
    return {k: _interval(Trk[k], min_cams) for k in Trk.keys()}


def _frame_mask(n_frame, lo, hi):
    m = np.zeros(n_frame, bool)
    m[lo:hi] = True
    return m


def to_intv(I):
    """Runs of ones of a 0/1 sequence as rows [start, stop) (step3:1487-1502)."""
    v = np.array(I, dtype=int)
    if v[-1] == 1:
        v = np.append(v, 0)
    d = np.diff(np.append(np.array([0]), v))
    return np.array([np.where(d == 1)[0], np.where(d == -1)[0]]).T


def calc_dist_pose(p1, p2):
    """RMS distance over the frames where both traces are finite; NaN when there is none (step3:304-311)."""
    d = np.sum((p1 - p2) ** 2, axis=1)
    d = d[~np.isnan(d)]
    if d.size == 0:
        return np.nan
    return np.sqrt(d.sum() / d.size)


def get_camparam(config_path, calibration_path=None):
    from src.pipeline.step2_crossviewmatching import get_camparam as _get
    return _get(config_path, calibration_path=calibration_path)


def calc_3dpose(kp_2d, config_path="", camparam=None, device=0):
    """step3:254-272: (C, J, 3) raw x, y, score -> (J, 3) by omnidir undistortion and the pinv DLT over the
    cameras with finite x and score >= 0.3 (``mq_omnidir_undistort`` + ``mq_triangulate_pinv``)."""
    from mqhip.association import StepTwoCameras, calc_3dpose_batch
    from mqhip.tracklets import THR_KP
    cams = camparam if isinstance(camparam, StepTwoCameras) else StepTwoCameras(
        get_camparam(config_path) if camparam is None else camparam, device=device)
    return calc_3dpose_batch(cams, np.asarray(kp_2d, dtype=np.float64)[None], thr_kp=THR_KP)[0]


def calc_3dtrace(lift, trk, frames, n_frame=None):
    """step3:274-302: the per-frame nanmedian of the lifted joints of one tracklet on ``frames`` (NaN
    elsewhere and where fewer than two cameras hold a box), as (n_frame, 3)."""
    frames = np.asarray(frames, dtype=np.int64).ravel()
    n_frame = trk.shape[0] if n_frame is None else n_frame
    out = np.full((n_frame, 3), np.nan)
    if len(frames):
        cells = np.stack([np.zeros_like(frames), frames], axis=1)
        out[frames] = lift.traces({0: trk}, cells)[0]
    return out


def connect_keyframe(T, result_keyframe, n_cam, divide_2dtrack=True):
    """step3:669-837 on the loaded rows ``T`` and step 2's keyframe records: the person links between
    consecutive keyframes (Hungarian on the count of shared box ids), and -- where a linked person changes
    box id in a camera, or one box id moves to another person -- fresh box ids from the later keyframe on
    (-10 in the rows / -1 in the records strictly between the two keyframes).
    Returns (T2, result_keyframe2, C); the inputs are left untouched."""
    import copy

    from scipy.optimize import linear_sum_assignment
    n_frame = len(T[0])
    n_kf = len(result_keyframe)
    C = []
    change = {c: [] for c in range(n_cam)}
    for i_kf in range(1, n_kf):
        f_pre, f_crnt = result_keyframe[i_kf - 1]["frame"], result_keyframe[i_kf]["frame"]
        b_pre = [np.asarray(b) for b in result_keyframe[i_kf - 1]["bcomb"]]
        b_crnt = [np.asarray(b) for b in result_keyframe[i_kf]["bcomb"]]
        sim = np.zeros([len(b_pre), len(b_crnt)], float)
        for i, b1 in enumerate(b_pre):
            for j, b2 in enumerate(b_crnt):
                sim[i, j] = np.sum((b1 == b2) & (b1 >= 0) & (b2 >= 0))
        rows, cols = linear_sum_assignment(-sim)
        c = [[rows[i], cols[i]] for i in range(len(rows)) if sim[rows[i], cols[i]] > 0]
        C.append(c)
        link_of_pre = {p: i for i, (p, _) in enumerate(c)}
        link_of_crnt = {q: i for i, (_, q) in enumerate(c)}
        for i_cam in range(n_cam):
            for p, b1 in enumerate(b_pre):
                if b1[i_cam] < 0:
                    continue
                for q, b2 in enumerate(b_crnt):
                    if b2[i_cam] < 0 or p not in link_of_pre or q not in link_of_crnt:
                        continue
                    if link_of_pre[p] == link_of_crnt[q]:
                        if b1[i_cam] != b2[i_cam]:      # one animal, two box ids
                            change[i_cam].append([b1[i_cam], f_pre, f_crnt])
                            change[i_cam].append([b2[i_cam], f_pre, f_crnt])
                    elif b1[i_cam] == b2[i_cam]:        # one box id, two animals
                        change[i_cam].append([b1[i_cam], f_pre, f_crnt])

    last_id = -1
    for cam in T[:n_cam]:
        for rows in cam:
            for tt in rows:
                last_id = max(last_id, tt[0])
    last_id += 1

    T2 = copy.deepcopy(T)
    kf2 = copy.deepcopy(result_keyframe)
    for i_cam in range(n_cam):
        bc = np.reshape(np.unique(np.array(change[i_cam]), axis=0), [-1, 3]).astype(int)
        for i_box in np.unique(bc[:, 0]):
            ids_T = np.ones(n_frame, int) * i_box
            ids_kf = np.ones(n_frame, int) * i_box
            for f0, f1 in bc[bc[:, 0] == i_box, 1:3]:
                ids_kf[f0 + 1:f1] = -1
                ids_kf[f1:] = last_id
                ids_T[f0 + 1:f1] = -10
                ids_T[f1:] = last_id
                last_id += 1
            for i_frame in range(n_frame):
                for i_tt, tt in enumerate(T[i_cam][i_frame]):
                    if tt[0] == i_box:
                        T2[i_cam][i_frame][i_tt][0] = int(ids_T[i_frame])
            for i_kf in range(n_kf):
                i_frame = result_keyframe[i_kf]["frame"]
                for i_person, bb in enumerate(result_keyframe[i_kf]["bcomb"]):
                    if bb[i_cam] == i_box:
                        kf2[i_kf]["bcomb"][i_person][i_cam] = ids_kf[i_frame]
    if divide_2dtrack:
        return T2, kf2, C
    return T, result_keyframe, C


def get_tracklets(T, result_keyframe, n_cam):
    """step3:1166-1259: (Trk, T, n_frame, n_cam, C).  Renumbers the rows (``connect_keyframe``), zeroes the
    ID score of an individual's class detected twice in one image, and chains the linked keyframe people
    into Trk[k] (n_frame, n_cam) box ids; n_frame is the last keyframe's frame, as in the reference."""
    T, kf, C = connect_keyframe(T, result_keyframe, n_cam, divide_2dtrack=True)
    for i_cam in range(n_cam):
        for rows in T[i_cam]:
            cnt = np.zeros(20, int)
            for tt in rows:
                if tt[6] in ID_CLASSES and tt[7] > cid_thr:
                    cnt[tt[6]] += 1
            for i_det in np.argwhere(cnt > 1).ravel():
                for tt in rows:
                    if tt[6] == i_det:
                        tt[7] = 0.0

    n_frame = kf[-1]["frame"]
    crnt_ids = np.arange(len(kf[0]["bcomb"]), dtype=int)
    cnt = 0 if len(crnt_ids) == 0 else int(max(crnt_ids)) + 1
    Trk = {}
    for i_kf in range(1, len(kf)):
        f_pre, f_crnt = kf[i_kf - 1]["frame"], kf[i_kf]["frame"]
        pre_ids = crnt_ids.copy()
        c = C[i_kf - 1]
        for i_box, pid in enumerate(pre_ids):
            pid = int(pid)
            if pid not in Trk:
                Trk[pid] = -np.ones([n_frame, n_cam], dtype=int)
            for p, q in c:
                if p != i_box:
                    continue
                b_pre = np.asarray(kf[i_kf - 1]["bcomb"][p])
                b_crnt = np.asarray(kf[i_kf]["bcomb"][q])
                clash = (b_pre >= 0) & (b_crnt >= 0) & (b_pre != b_crnt)
                use = -np.ones(n_cam, dtype=int)
                use[(b_crnt >= 0) & ~clash] = b_crnt[(b_crnt >= 0) & ~clash]
                use[(b_pre >= 0) & ~clash] = b_pre[(b_pre >= 0) & ~clash]     # the earlier keyframe wins
                Trk[pid][f_pre:f_crnt, :] = use
        crnt_ids = -np.ones(len(kf[i_kf]["bcomb"]), dtype=int)
        for p, q in c:
            crnt_ids[q] = pre_ids[p]
        for i in range(len(crnt_ids)):
            if crnt_ids[i] < 0:
                crnt_ids[i] = cnt
                cnt += 1
    for k in [k for k in Trk if not np.any(Trk[k] >= 0)]:
        Trk.pop(k)
    return Trk, T, n_frame, n_cam, C


def trim_tracklets(Trk, lift, n_frame, log=None):
    """step3:1504-1568: where two tracklets overlap by a few frames (at most a third of either and 12) at
    their ends and their traces agree within 150 mm RMS there, the shorter-first one gives the frames up.
    Trimming only clears cells (a cleared cell lifts to NaN), so the traces of every cell come from one
    launch up front.  ``log`` collects every (k1, k2, rmse) compared with the threshold."""
    import copy
    Intv = _intervals(Trk)
    K = list(Trk.keys())
    order = np.argsort(np.array([Intv[k][1] - Intv[k][0] for k in K]))
    K = np.array(K, dtype=int)[order].tolist()
    Trk2 = copy.deepcopy(Trk)
    pos = {k: i for i, k in enumerate(Trk.keys())}
    trace = lift.traces(Trk)[0][:, :n_frame].copy()
    for k1 in K:
        for k2 in K:
            if k2 == k1:
                continue
            e1 = np.zeros(n_frame, int)
            e2 = np.zeros(n_frame, int)
            e1[Intv[k1][0]:Intv[k1][1] + 1] = 1
            e2[Intv[k2][0]:Intv[k2][1] + 1] = 1
            n_overlap = np.sum(e1 * e2)
            if n_overlap == 0:
                continue
            if n_overlap > np.sum(e1) / 3 or n_overlap > np.sum(e2) / 3 or n_overlap > 12:
                continue
            case_a = Intv[k1][0] > Intv[k2][0] and Intv[k1][1] > Intv[k2][1]
            case_b = Intv[k2][0] > Intv[k1][0] and Intv[k2][1] > Intv[k1][1]
            if not case_a and not case_b:
                continue
            fo = np.argwhere(e1 * e2 == 1).ravel()
            rmse = calc_dist_pose(trace[pos[k1]][fo], trace[pos[k2]][fo])
            if log is not None:
                log.append((int(k1), int(k2), float(rmse)))
            if rmse < TRIM_RMSE_MM:
                if case_a:
                    Intv[k1][0] = Intv[k2][1] + 1
                    Trk2[k1][:Intv[k2][1] + 1, :] = -1
                    trace[pos[k1]][:Intv[k2][1] + 1] = np.nan
                else:
                    Intv[k1][1] = Intv[k2][0] - 1
                    Trk2[k1][Intv[k2][0]:, :] = -1
                    trace[pos[k1]][Intv[k2][0]:] = np.nan
    return Trk2


def count_id_detections(lift, Trk, n_frame):
    """step3:839-870: Trk_cid[k] (n_frame, 4) votes per frame for the four individuals' classes, from every
    row of every camera carrying the tracklet's box id with an ID score above 0.8 (``mq_tracklet_id_votes``,
    one launch for all tracklets)."""
    votes = lift.id_votes(Trk)
    out = {}
    for i, k in enumerate(Trk.keys()):
        v = np.zeros([n_frame, votes.shape[2]], dtype=int)
        n = min(n_frame, votes.shape[1])
        v[:n] = votes[i, :n]
        out[k] = v[:, list(ID_CLASSES)]
    return out


def _window_vote(cnt, min_count):
    """(class, accepted) of a vote count vector: the leader needs more than 80 % and ``min_count`` votes."""
    i_max = int(np.argmax(cnt))
    tot = np.sum(cnt)
    p = 0.0 if tot == 0 else cnt[i_max] / tot
    return i_max, bool(p > 0.8 and cnt[i_max] >= min_count)


def set_id_for_each_frame_of_tracklets(Trk, Trk_cid, n_frame, wsize):
    """step3:1344-1444: per tracklet, a sliding window of ``wsize`` frames labels the frames whose votes are
    decisive; a tracklet with one label takes it everywhere, one with none falls back to its global vote,
    one with several is cut midway between the last vote of the old label and the first of the new."""
    h = int(wsize / 2)
    Intv = _intervals(Trk)
    Cid = {}
    for k in Trk_cid.keys():
        cid0 = Trk_cid[k]
        cid1 = -np.ones(n_frame, dtype=int)
        cid2 = -np.ones(n_frame, dtype=int)
        for i_frame in range(max(Intv[k][0], h), min(Intv[k][1], n_frame - h)):
            i_max, ok = _window_vote(np.sum(cid0[i_frame - h:i_frame + h, :], axis=0), const_mindetcnt1)
            if ok:
                cid1[i_frame] = i_max
        uid = np.unique(cid1[Intv[k][0]:Intv[k][1]])
        n_id = int(np.sum(uid >= 0))
        if n_id == 0:
            i_max, ok = _window_vote(np.sum(cid0, axis=0), const_mindetcnt1)
            if ok:
                cid2[:] = i_max
        elif n_id == 1:
            cid2[:] = uid[uid >= 0]
        else:
            pre_id, pre_frame = -1, 0
            for i_frame in range(n_frame):
                crnt_id = cid1[i_frame]
                if crnt_id < 0:
                    continue
                if crnt_id == pre_id:
                    cid2[pre_frame:i_frame] = crnt_id
                elif pre_id == -1:
                    cid2[0:i_frame] = crnt_id
                elif i_frame - pre_frame > 1:
                    det = np.argwhere(cid0[:, pre_id] > 0).ravel()
                    det = det[(det >= max(1, pre_frame - h)) & (det <= i_frame)]
                    last_pre = int(det.max()) if det.size else pre_frame
                    det = np.argwhere(cid0[:, crnt_id] > 0).ravel()
                    det = det[(det >= pre_frame) & (det <= min(i_frame + h, n_frame))]
                    first_crnt = int(det.min()) if det.size else i_frame
                    if last_pre < first_crnt:
                        mid = int((first_crnt - last_pre) / 2) + last_pre
                    else:
                        mid = int((i_frame - pre_frame) / 2) + pre_frame
                    cid2[pre_frame:mid] = pre_id
                    cid2[mid:i_frame] = crnt_id
                pre_id, pre_frame = crnt_id, i_frame
            cid2[pre_frame:] = pre_id
        Cid[k] = cid2
    return Cid


def div_3dtracklet(Trk, Cid, stitch_info=None):
    """step3:917-983: a tracklet whose frames carry more than one label (-1 included) is replaced by one
    tracklet per run of equal labels; ``stitch_info`` follows the pieces."""
    assigned = [k for k in Trk.keys() if np.sum(Cid[k] >= 0) > 0]
    Intv = _intervals(Trk)
    last_key = max(list(Trk.keys()))
    for k in assigned:
        lo, hi = Intv[k]
        labels = np.unique(Cid[k][lo:hi])
        if labels.shape[0] <= 1:
            continue
        n_frame, n_cam = Trk[k].shape
        inside = _frame_mask(n_frame, lo, hi)
        for lab in labels:
            for a, b in to_intv(np.logical_and(Cid[k] == lab, inside)):
                C = -np.ones(n_frame, dtype=int)
                C[a:b + 1] = lab
                trk = -np.ones([n_frame, n_cam], dtype=int)
                trk[a:b + 1, :] = Trk[k][a:b + 1, :]
                last_key += 1
                Cid[last_key] = C
                Trk[last_key] = trk
                if stitch_info is not None and k in stitch_info:
                    stitch_info[last_key] = [f for f in stitch_info[k] if min(b, f[1]) >= max(a, f[0])]
        Trk.pop(k)
        Cid.pop(k)
    if stitch_info is None:
        return Trk, Cid
    return Trk, Cid, stitch_info


def remove_single_cam_tracklets(Trk):
    """step3:1295-1310: drop the tracklets never seen by two cameras at once."""
    for k in [k for k in Trk.keys() if np.sum(np.sum(np.array(Trk[k]) >= 0, axis=1) > 1) == 0]:
        Trk.pop(k)
    return Trk


def remove_short_tracklets(Trk, Cid, min_frames=24):
    """step3:1280-1293: drop the unlabelled tracklets spanning at most ``min_frames`` frames."""
    drop = []
    for k in Trk.keys():
        if np.sum(Cid[k] >= 0) == 0:
            lo, hi = _interval(Trk[k])
            if hi - lo <= min_frames:
                drop.append(k)
    for k in drop:
        Trk.pop(k)
    return Trk


def get_graph(Trk, Cid, lift, n_frame):
    """step3:1079-1164: candidate links k1 -> k2 as rows [k1, k2, d].  k2 must carry on two of k1's last box
    ids within 120 frames, and overlap neither tracklet by more than half; d is the distance between the
    nanmean joints of k1's last frame and k2's first frame from there on (x 0.01 when both carry the same
    label; no link when the labels differ).  As in the reference, the -1 entries of k1's last row become -2
    in place.  The nanmean of every cell comes from one launch."""
    Intv = _intervals(Trk, min_cams=2)
    pos = {k: i for i, k in enumerate(Trk.keys())}
    mean = lift.traces(Trk)[1]
    G = []
    for k1 in Trk.keys():
        for k2 in Trk.keys():
            if k1 == k2:
                continue
            lo1, hi1 = Intv[k1]
            t_e = Trk[k1][hi1, :]
            t_e[t_e == -1] = -2
            carried = np.sum(Trk[k2][hi1:min(hi1 + LINK_WINDOW, n_frame)] == t_e, axis=0)
            if np.sum(carried > 1) == 0:
                continue
            lo2, hi2 = Intv[k2]
            I1 = _frame_mask(n_frame, lo1, hi1)
            I2 = _frame_mask(n_frame, lo2, hi2)
            n1, n2, n12 = np.sum(I1), np.sum(I2), np.sum(np.logical_and(I1, I2))
            if n12 / n1 > 0.5 or n12 / n2 > 0.5:
                continue
            later = np.argwhere(np.sum(Trk[k2] >= 0, axis=1) > 1)
            later = later[later >= hi1]
            if later.shape[0] == 0:
                continue
            f2 = int(later[0])
            d = np.sqrt(np.sum((mean[pos[k1], hi1] - mean[pos[k2], f2]) ** 2))
            id1, id2 = Cid[k1][hi1], Cid[k2][f2]
            if id1 != -1 and id2 != -1 and id1 != id2:
                continue
            if id1 != -1 and id1 == id2:
                d = d * 0.01
            if np.isnan(d):
                continue
            G.append([k1, k2, d])
    return np.reshape(np.array(G), [-1, 3])


def _min_cost_flow(n_node, edges, supply):
    """Min-cost flow by successive shortest paths (queue-based Bellman-Ford on the residual graph; the
    graphs here have at most 2K+4 nodes).  edges: [u, v, capacity, cost]; supply[u] > 0 sends, < 0 takes.
    Returns (cost, flow per edge) or None when the demands cannot be met."""
    from collections import deque
    S, Tn = n_node, n_node + 1
    head, to, cap, cost = [[] for _ in range(n_node + 2)], [], [], []

    def add(u, v, c, w):
        head[u].append(len(to)); to.append(v); cap.append(c); cost.append(w)
        head[v].append(len(to)); to.append(u); cap.append(0); cost.append(-w)

    for u, v, c, w in edges:
        add(u, v, c, w)
    need = 0
    for u, b in enumerate(supply):
        if b > 0:
            add(S, u, b, 0)
            need += b
        elif b < 0:
            add(u, Tn, -b, 0)
    total = 0
    while need > 0:
        dist = [None] * (n_node + 2)
        prev = [-1] * (n_node + 2)
        dist[S] = 0
        queue, queued = deque([S]), [False] * (n_node + 2)
        while queue:
            u = queue.popleft()
            queued[u] = False
            for e in head[u]:
                if cap[e] > 0 and (dist[to[e]] is None or dist[u] + cost[e] < dist[to[e]]):
                    dist[to[e]] = dist[u] + cost[e]
                    prev[to[e]] = e
                    if not queued[to[e]]:
                        queued[to[e]] = True
                        queue.append(to[e])
        if dist[Tn] is None:
            return None
        v = Tn
        while v != S:       # every augmenting path carries one unit: the arcs into Tn from IN / OUT have capacity 1
            e = prev[v]
            cap[e] -= 1
            cap[e ^ 1] += 1
            v = to[e ^ 1]
        total += dist[Tn]
        need -= 1
    return total, [cap[2 * i + 1] for i in range(len(edges))]


def _flow_network(g):
    """The reference's flow network of the links ``g`` (step3:326-349) as an edge list over node indices:
    IN_i = i, OUT_i = n + i, source = 2n, sink = 2n + 1.  Returns (tracklet keys, edges, links) with
    edges[:n] the IN -> OUT arcs, edges[n:2n] source -> IN, edges[2n:3n] OUT -> sink, edges[3n:] the links."""
    nodes = np.unique(g[:, :2]).astype(int)
    n = nodes.shape[0]
    idx = {int(k): i for i, k in enumerate(nodes)}
    edges = [[i, n + i, 1, 0] for i in range(n)]
    edges += [[2 * n, i, 1, OUT_COST] for i in range(n)]
    edges += [[n + i, 2 * n + 1, 1, OUT_COST] for i in range(n)]
    link = {}
    for k1, k2, d in g:     # a repeated link replaces the earlier one, as DiGraph.add_edge does
        link[(idx[int(k1)], idx[int(k2)])] = int(d * 100.0)
    links = list(link.items())
    edges += [[n + a, b, 1, w] for (a, b), w in links]
    return nodes, edges, links


def flow_sweep(g):
    """[(n_track, cost, accepted, flow per edge)] for every feasible n_track in 1 .. n_node-1: the min-cost
    flow of the reference's network with ``n_track`` units from source to sink; ``accepted`` is False when
    the optimum found sends a second unit through a tracklet (its IN -> OUT arc carries flow)."""
    nodes, edges, _ = _flow_network(g)
    n = nodes.shape[0]
    out = []
    for n_track in range(1, n):
        res = _min_cost_flow(2 * n + 2, edges, [-1] * n + [1] * n + [n_track, -n_track])
        if res is not None:
            out.append((n_track, res[0], not any(res[1][:n]), res[1]))
    return out


def calc_flow(g):
    """step3:313-402 without networkx: the tracklets of ``g``'s links [k1, k2, d] are covered by paths.
    For n_track = 1 .. n_node-1 the reference's network is solved as it stands -- source (supply n_track),
    sink, IN_k (takes 1) -> OUT_k (gives 1) with capacity 1 and cost 0, source -> IN_k and OUT_k -> sink at
    cost 100000, link OUT_k1 -> IN_k2 at cost int(100 d) -- and an n_track whose optimum sends two units
    through a tracklet is *rejected* (not re-solved with that forbidden).  The cheapest accepted optimum
    (the smallest n_track on ties) gives the paths, ordered by their first tracklet."""
    nodes, _, links = _flow_network(g)
    n = nodes.shape[0]
    best, min_cost = None, int(1000 * 100 * 1000)
    for n_track, total, accepted, flow in flow_sweep(g):
        if accepted and total < min_cost:
            min_cost, best = total, flow
    if best is None:
        raise ValueError("calc_flow: no admissible path cover")
    nxt = {a: b for ((a, b), _), f in zip(links, best[3 * n:]) if f}
    P = []
    for i in range(n):
        if best[n + i]:     # source -> IN_i
            path, seen = [int(nodes[i])], {i}
            while i in nxt and nxt[i] not in seen:
                i = nxt[i]
                seen.add(i)
                path.append(int(nodes[i]))
            P.append(path)
    return P


def stitch_tracklets(Trk, Cid, lift, n_frame, record=None):
    """step3:1446-1485: the tracklets of every multi-tracklet path of ``calc_flow`` are merged (the first
    one's array is filled in place where it holds -1) under a new key; stitch_info[key] lists the merged
    intervals."""
    stitch_info = {}
    g = get_graph(Trk, Cid, lift, n_frame)
    if record is not None:
        record["graph"] = g.copy()
    if g.shape[0] == 0:
        return Trk, stitch_info
    paths = calc_flow(g)
    if record is not None:
        record["paths"] = [list(p) for p in paths]
    Intv = _intervals(Trk)
    last_key = max(list(Trk.keys()))
    drop = []
    for path in paths:
        if len(path) < 2:
            continue
        trk1 = Trk[path[0]]
        for k in path:
            hole = trk1 == -1
            trk1[hole] = Trk[k][hole]
        last_key += 1
        Trk[last_key] = trk1
        stitch_info[last_key] = [Intv[k] for k in path]
        drop.extend(path)
    for k in drop:
        Trk.pop(k)
    return Trk, stitch_info


def breakdown_stitched_tracklet(Trk, Cid, stitch_info):
    """step3:216-252: a stitched tracklet goes back to its pieces, each labelled with the stitched one's
    (largest) label."""
    Intv = _intervals(Trk)
    last_key = max(list(Trk.keys()))
    for k in list(stitch_info.keys()):
        if k not in Cid:
            continue
        n_frame, n_cam = Trk[k].shape
        cid = np.max(np.unique(Cid[k][Intv[k][0]:Intv[k][1]]))
        for a, b in stitch_info[k]:
            trk = -np.ones([n_frame, n_cam], dtype=int)
            trk[a:b + 1, :] = Trk[k][a:b + 1, :]
            C = -np.ones(n_frame, dtype=int)
            C[a:b + 1] = cid
            last_key += 1
            Cid[last_key] = C
            Trk[last_key] = trk
        Trk.pop(k)
        Cid.pop(k)
    return Trk, Cid


def clean_id_duplication(Trk, Cid, Trk_cid, n_frame, wsize, fps, n_animal=4):
    """step3:404-637: per individual, where several tracklets carry its label at once, unlabel those
    without a confident vote of their own (window vote, 6 detections), delete those adding no frame of their
    own, and cut or delete the remaining overlapping neighbours at their confident frames.  At the end every
    tracklet is cut to [first, last) of its interval, as in the reference."""
    h = int(wsize / 2)
    Intv = _intervals(Trk)
    k_exclude, k_del = [], []
    for i_sub in range(n_animal):
        K = [k for k in Trk.keys() if np.sum(np.unique(Cid[k]) == i_sub)]
        cnt_overlap = np.zeros(n_frame, int)
        for k in K:
            cnt_overlap[Intv[k][0]:Intv[k][1]] += 1
        if np.sum(cnt_overlap > 1) == 0:
            continue

        confident = {}
        for k in K:
            cid0 = Trk_cid[k]
            c1 = -np.ones(n_frame, dtype=int)
            for i_frame in range(max(Intv[k][0], h), min(Intv[k][1], n_frame - h)):
                i_max, ok = _window_vote(np.sum(cid0[i_frame - h:i_frame + h, :], axis=0), const_mindetcnt2)
                if ok:
                    hit = np.argwhere(cid0[i_frame - h:i_frame + h, i_max])
                    if np.min(hit) <= h and np.max(hit) >= h:
                        c1[i_frame] = i_max
            c1[:Intv[k][0]] = -1
            c1[Intv[k][1]:] = -1
            confident[k] = c1

        order = np.argsort(np.array([Intv[k][1] - Intv[k][0] for k in K]))
        K = np.array(K, dtype=int)[order].tolist()

        for k1 in K:    # overlapping another and no confident frame: unlabel
            e1 = np.zeros(n_frame, int)
            e2 = np.zeros(n_frame, int)
            e1[Intv[k1][0]:Intv[k1][1]] = 1
            for k2 in K:
                if k2 == k1 or k2 in k_exclude:
                    continue
                e2[Intv[k2][0]:Intv[k2][1]] += 1
            if np.sum(e1 * e2) == 0:
                continue
            if not np.any(confident[k1] == i_sub):
                k_exclude.append(k1)

        for k1 in K:    # no frame of its own: delete
            if k1 in k_exclude:
                continue
            e1 = np.zeros(n_frame, int)
            e2 = np.zeros(n_frame, int)
            a, b = Intv[k1]
            e1[a:b] = 1
            for k2 in K:
                if k2 == k1 or k2 in k_exclude:
                    continue
                e2[Intv[k2][0]:Intv[k2][1]] = 1
            if np.sum(e1 > e2) == 0:
                at_edge = a == 0 or b == n_frame - 1
                if np.sum(cnt_overlap[a:b] > 2) != 0 or not at_edge:
                    k_exclude.append(k1)
                    k_del.append(k1)

        K = [k for k in K if k not in k_exclude]
        iv = np.array([Intv[k] for k in K])
        order = np.lexsort([iv[:, 1], iv[:, 0]])
        K = np.array(K, dtype=int)[order].tolist()
        for k1, k2 in zip(K[:-1], K[1:]):   # neighbours in time
            if k1 in k_exclude:
                continue
            if Intv[k1][1] < Intv[k2][0]:
                continue
            f1 = np.argwhere(confident[k1] == i_sub).ravel()
            f2 = np.argwhere(confident[k2] == i_sub).ravel()
            if f1.shape[0] == 0:
                k_exclude.append(k1)
                continue
            if f2.shape[0] == 0:
                k_exclude.append(k2)
                continue
            f1, f2 = int(np.max(f1)), int(np.min(f2))
            if f1 < f2:
                Intv[k1][1], Intv[k2][0] = f1, f2
                confident[k1][f1:] = -1
                confident[k2][:f2] = -1
            elif f2 - Intv[k1][0] >= fps and Intv[k2][1] - f1 >= fps:
                Intv[k1][1], Intv[k2][0] = f2, f1
                confident[k1][f2:] = -1
                confident[k2][:f1] = -1
            elif Intv[k1][1] - Intv[k1][0] > Intv[k2][1] - Intv[k2][0]:
                k_exclude.append(k2)
                k_del.append(k2)
            else:
                k_exclude.append(k1)
                k_del.append(k1)

    for k in k_exclude:
        Cid[k][:] = -1
    for k in Intv.keys():
        Trk[k][:Intv[k][0], :] = -1
        Trk[k][Intv[k][1]:, :] = -1
    for k in Trk.keys():
        if not np.any(np.sum(Trk[k] >= 0, axis=1) > 0):
            k_del.append(k)
    for k in set(k_del):
        Trk.pop(k)
        Cid.pop(k)
        Trk_cid.pop(k)
    return Trk, Cid, Trk_cid


def assign_lastone(Trk, Cid, lift, n_animal=4, min_duration=12, log=None):
    """step3:96-214: an unlabelled tracklet (longest first) takes the one label that is free while all the
    others are taken during its interval -- more than 80 % of such frames, at least 3 -- unless a labelled
    tracklet follows the same trace (RMS below 150 mm over enough shared frames) or already holds that label
    during the interval.  The median traces of every cell come from one launch."""
    Intv = _intervals(Trk)
    unassigned = [k for k in Trk.keys() if np.sum(Cid[k] >= 0) == 0]
    assigned = [k for k in Trk.keys() if np.sum(Cid[k] >= 0) != 0]
    order = np.argsort(np.array([Intv[k][1] - Intv[k][0] for k in unassigned]))[-1::-1]
    unassigned = np.array(unassigned, dtype=int)[order].tolist()
    flag_update = False
    if len(assigned) == 0 or len(unassigned) == 0:
        return Trk, Cid, flag_update
    n_frame = Trk[assigned[0]].shape[0]
    A = np.zeros([n_frame, n_animal])
    for k in assigned:
        a, b = Intv[k]
        for i_c in range(n_animal):
            A[a:b, i_c] += Cid[k][a:b] == i_c
    A = A > 0
    pos = {k: i for i, k in enumerate(Trk.keys())}
    trace = None
    for k in unassigned:
        a, b = Intv[k]
        if b - a <= min_duration:
            continue
        taken = A[a:b, :]
        free = np.logical_not(taken)[np.sum(taken, axis=1) == n_animal - 1, :]
        cnt = np.sum(free, axis=0)
        i_max = int(np.argmax(cnt))
        p = 0.0 if np.sum(cnt) == 0 else cnt[i_max] / np.sum(cnt)
        if not (p > 0.8 and cnt[i_max] >= 3):
            continue
        cid = i_max
        Ik = _frame_mask(n_frame, a, b)
        clash = False
        for k2 in assigned:
            n_overlap = np.sum(np.logical_and(Ik, _frame_mask(n_frame, Intv[k2][0], Intv[k2][1])))
            if n_overlap == 0:
                continue
            thr = 2 if n_overlap > (b - a) / 2 else 12
            if trace is None:
                trace = lift.traces(Trk)[0][:, :n_frame]
            # the unlabelled tracklet's trace is NaN outside [a, b], so only those frames count
            d = np.sum((trace[pos[k]] - trace[pos[k2]]) ** 2, axis=1)
            d = d[np.logical_not(np.isnan(d))]
            if d.shape[0] >= thr:
                rmse = np.sqrt(np.sum(d) / d.shape[0])
                if log is not None:
                    log.append((int(k), int(k2), float(rmse)))
                if rmse < TRIM_RMSE_MM:
                    clash = True
                    break
        if clash:
            continue
        for k2 in assigned:
            ids = np.unique(Cid[k2][Intv[k2][0]:Intv[k2][1]])
            ids = ids[ids >= 0]
            if not (ids.size == 1 and ids[0] == cid):
                continue
            if np.sum(np.logical_and(Ik, _frame_mask(n_frame, Intv[k2][0], Intv[k2][1]))) > 0:
                clash = True
                break
        if clash:
            continue
        flag_update = True
        Cid[k][:] = cid
        assigned.append(k)
    return Trk, Cid, flag_update


def _copy_tracks(D):
    return {int(k): np.array(v) for k, v in D.items()}


def run_stages(T, result_keyframe, n_cam, make_lift, n_animal=4, n_kp=17, fps=24, record=None):
    """``main_proc``'s chain (step3:36-94) on loaded rows and keyframe records.  ``make_lift(T)`` builds the
    lift from the renumbered rows.  Returns (Trk, Cid, T, C, n_frame); ``record`` (a dict) collects the
    intermediates the fixtures store.  Keyframes without a single linked person give empty dicts (the
    reference fails there)."""
    rec = record if record is not None else {}
    wsize = fps * 5
    if len(result_keyframe) == 0:
        raise ValueError("step 3 needs at least one keyframe record (a clip of 14 frames or more)")
    Trk, T, n_frame, n_cam, C = get_tracklets(T, result_keyframe, n_cam)
    rec["trk_tracklets"] = _copy_tracks(Trk)
    if not Trk:
        return {}, {}, T, C, n_frame
    lift = make_lift(T)
    rec["trim_rmse"] = []
    Trk = trim_tracklets(Trk, lift, n_frame, log=rec["trim_rmse"])
    rec["trk_trimmed"] = _copy_tracks(Trk)

    Trk_cid = count_id_detections(lift, Trk, n_frame)
    Cid = set_id_for_each_frame_of_tracklets(Trk, Trk_cid, n_frame, wsize)
    rec["cid_first"] = _copy_tracks(Cid)
    Trk, Cid = div_3dtracklet(Trk, Cid)

    Trk = remove_single_cam_tracklets(Trk)
    Trk = remove_short_tracklets(Trk, Cid, min_frames=0)
    if not Trk:
        return {}, {}, T, C, n_frame

    Trk, stitch_info = stitch_tracklets(Trk, Cid, lift, n_frame, record=rec)

    Trk_cid = count_id_detections(lift, Trk, n_frame)
    Cid = set_id_for_each_frame_of_tracklets(Trk, Trk_cid, n_frame, wsize)
    rec["cid_second"] = _copy_tracks(Cid)
    Trk, Cid, stitch_info = div_3dtracklet(Trk, Cid, stitch_info)

    Trk, Cid = breakdown_stitched_tracklet(Trk, Cid, stitch_info)
    Trk_cid = count_id_detections(lift, Trk, n_frame)
    Trk, Cid, Trk_cid = clean_id_duplication(Trk, Cid, Trk_cid, n_frame, wsize, fps, n_animal=n_animal)

    rec["lastone_rmse"] = []
    for _ in range(n_animal):
        Trk, Cid, updated = assign_lastone(Trk, Cid, lift, n_animal=n_animal, min_duration=12,
                                           log=rec["lastone_rmse"])
        if not updated:
            break
    return Trk, Cid, T, C, n_frame


def main_proc(config_path, result_dir, rmse_thr=200.0, camparam=None, device=0, n_animal=4, n_kp=17):
    """step3:36-94: alldata.json of every camera + match_keyframe.pickle -> kp2d.pickle, track.pickle,
    collar_id.pickle, keyframe_connection.pickle in ``result_dir``; returns (Trk, Cid, T).  ``rmse_thr`` is
    accepted and unused, as in the reference.  The labels are the four ID classes' indices; with
    ``n_animal`` < 4 a label past it has no slot in kp2d and is left out of that file (track.pickle and
    collar_id.pickle keep it).  Needs a HIP device: the lift has no CPU path."""
    from mqhip.association import StepTwoCameras
    from mqhip.tracklets import TrackletLift
    cam_ids = camera_ids(config_path)
    if camparam is None:
        calib = os.path.join(os.path.dirname(config_path), "calibration.toml")
        if not os.path.exists(calib):
            calib = os.path.join(result_dir, "calibration.toml")
        camparam = get_camparam(config_path, calibration_path=calib)
    cams = camparam if isinstance(camparam, StepTwoCameras) else StepTwoCameras(camparam, device=device)
    T = load_alldata(result_dir, cam_ids)
    with open(os.path.join(result_dir, "match_keyframe.pickle"), "rb") as f:
        result_keyframe = pickle.load(f)
    Trk, Cid, T, C, n_frame = run_stages(T, result_keyframe, len(cam_ids),
                                         lambda rows: TrackletLift(cams, rows, device), n_animal=n_animal, n_kp=n_kp)
    mqio.dump_pickle(C, os.path.join(result_dir, "keyframe_connection.pickle"))
    if Trk:
        shown = {k: np.where(Cid[k] < n_animal, Cid[k], -1) for k in Trk} if n_animal < len(ID_CLASSES) else Cid
        create_kp2dfile(result_dir, T, Trk, shown, n_animal=n_animal, n_kp=n_kp)
    else:
        mqio.dump_pickle(np.zeros([n_animal, n_frame, len(cam_ids), n_kp, 3]), os.path.join(result_dir, "kp2d.pickle"))
    mqio.dump_pickle(Trk, os.path.join(result_dir, "track.pickle"))
    mqio.dump_pickle(Cid, os.path.join(result_dir, "collar_id.pickle"))
    return Trk, Cid, T


def _gpu_renderer(cgroup, height, width, skeleton, mrksize, device):
    from mqhip.overlay import OverlayRenderer
    return OverlayRenderer(cgroup, height, width, skeleton=skeleton, mrksize=mrksize, device=device)


def _gpu_encoder(height, width, quality, device):
    from mqhip.mjpeg import JpegEncoder
    return JpegEncoder(height, width, quality=quality, device=device)


def _gpu_resizer(frames, height, width, device=0):
    from mqhip.resize import resize_bilinear
    return resize_bilinear(frames, height, width, device=device)


VIS_MAX_TRACKLETS = 8    # mqhip.overlay.MAX_ANIMALS: tracklets of one frame drawn per render pass


def visualize(vis_cam, config_path, result_dir, raw_data_dir, T=None, vidfile_prefix='', size=(800, 600), step=3,
              fps=24.0, quality=90, batch=16, device=0, camparam=None, renderer=None, encoder=None, resizer=None,
              lift=None, decoder=None):
    """step3:1570-1688: the tracking video of camera ``camera_id[vis_cam]``.  Every ``step``-th frame of
    track.pickle's range, each live tracklet (any box id >= 0 in the frame) lifted from its 2D rows, reprojected
    and drawn as a skeleton in the colour of its voted collar ID (collar_id.pickle; -1 is black) with its key
    written at the upper left (:1658-1670); the picture is then resized to ``size`` = (width, height) (:1685;
    None keeps the camera's size), encoded as JPEG at ``quality`` and appended to the Motion-JPEG AVI
    ``vidfile_prefix + '<camid>.avi'`` at ``fps`` (where the reference writes an mp4 through cv2), with
    ``.frame_number.npy`` / ``.frame_time.npy`` beside it.  Lift, drawing, resize and encoding run on the GPU
    (``mq_tracklet_traces``, ``mq_overlay_render_labelled``, ``mq_resize_bilinear``, ``mq_jpeg_encode``): one lift
    launch per ``batch`` frames, and only the lifted joints (which the renderer takes as host arrays) and the JPEG
    bytes leave the device.

    ``T``: the rows main_proc returned (``proc`` passes them; they carry step 3's renumbered box ids); None reads
    the cameras' alldata.json as the reference does.  A frame with more than 8 live tracklets is drawn in passes
    of 8 in ``Trk``'s key order, a pass's output being the next pass's source, which keeps the painter's order.
    The scores handed to the renderer are 1, as the reference's constant score column (:1652): the renderer's
    "no joint with X != 0 and score > 0" gate could then only drop a tracklet whose 18 lifted X coordinates are
    all exactly 0.0, which the lift cannot return for a cell it triangulated (an absent joint is NaN, and
    NaN != 0), so no tracklet is nulled by it.  A frame number absent from the store is skipped with a warning.
    ``renderer`` / ``encoder`` / ``decoder`` as in ``visualize_result.proc``; ``resizer``: a callable
    ``(frames, height, width, device=)``; ``lift``: a factory ``(rows)`` of an object with
    ``TrackletLift.traces`` (tests inject the NumPy restatements).  Returns the AVI's path, or None (and writes
    nothing) when track.pickle holds no tracklet."""
    cam_ids = camera_ids(config_path)
    with open(config_path, 'r') as f:
        ID = yaml.safe_load(f)['camera_id']
    if camparam is None:
        calib = os.path.join(os.path.dirname(config_path), "calibration.toml")
        if not os.path.exists(calib):
            calib = os.path.join(result_dir, "calibration.toml")
        camparam = get_camparam(config_path, calibration_path=calib)
    from mqhip.association import StepTwoCameras
    cams = camparam if isinstance(camparam, StepTwoCameras) else StepTwoCameras(camparam, device=device)
    if T is None:
        T = load_alldata(result_dir, cam_ids)
    Trk = mqio.load_array_pickle(os.path.join(result_dir, 'track.pickle'))
    Cid = mqio.load_array_pickle(os.path.join(result_dir, 'collar_id.pickle'))
    vid_path = vidfile_prefix + '{:d}.avi'.format(ID[vis_cam])
    keys = list(Trk.keys())
    if not keys:        # the reference takes the frame count from the first tracklet and fails without one
        print('no tracklets:', result_dir)
        return None

    data_name = os.path.basename(os.path.normpath(result_dir)).split('.')[0]
    store = mqio.FrameStore(raw_data_dir + '/' + data_name + '.' + str(ID[vis_cam]), decoder=decoder, device=device)
    frame_num = np.load(result_dir + '/' + str(ID[vis_cam]) + '/frame_num.npy')
    have = set(int(f) for f in store.get_frame_metadata()['frame_number'])
    n_frame = Trk[keys[0]].shape[0]
    rows = []
    for i_frame in range(0, min(n_frame, len(frame_num)), max(1, int(step))):
        fn = int(frame_num[i_frame])
        if fn not in have:
            print(f'[warning] Skipping frame {fn}: not found in the frame store')
            continue
        rows.append((i_frame, fn))

    H, W = (int(v) for v in store.frames.shape[1:3])
    w_out, h_out = (W, H) if size is None else (int(size[0]), int(size[1]))
    draw = (renderer or _gpu_renderer)(cams.proj.subset_cameras([vis_cam]), H, W, "v1", 3, device)
    resize = resizer or _gpu_resizer
    encode = (encoder or _gpu_encoder)(h_out, w_out, quality=quality, device=device)
    tracer = (lift(T) if lift is not None else None)
    if tracer is None:
        from mqhip.tracklets import TrackletLift
        tracer = TrackletLift(cams, T, device)
    writer = mqio.MjpegAviWriter(vid_path, h_out, w_out, fps=fps)
    n_kp = 17
    batch = max(1, int(batch))
    for k0 in range(0, len(rows), batch):
        part = rows[k0:k0 + batch]
        fns = [fn for _, fn in part]
        pos = [store.index_of(fn) for fn in fns]
        pool, src_index = np.unique(store.frame_index[pos], return_inverse=True)
        if store.format == 'mjpeg' and renderer is None:     # decoded on the device: only JPEG bytes are uploaded
            out = store.frames.device_frames([int(p) for p in pool], device)
        else:
            out = np.stack([np.asarray(store.frames[int(p)]) for p in pool])      # each source image once
        src_index = src_index.astype(np.int32)
        live = [[i for i, k in enumerate(keys) if np.any(Trk[k][i_frame] >= 0)] for i_frame, _ in part]
        cells = np.array([[i, i_frame] for (i_frame, _), ks in zip(part, live) for i in ks], dtype=np.int32)
        p3d = tracer.traces(Trk, cells=cells.reshape(-1, 2), return_p3d=True)[2] if len(cells) else None
        first = np.concatenate([[0], np.cumsum([len(ks) for ks in live])])
        B = len(part)
        n_max = max(len(ks) for ks in live)
        for p0 in range(0, max(n_max, 1), VIS_MAX_TRACKLETS):
            A = max(1, min(VIS_MAX_TRACKLETS, n_max - p0))
            kp3d = np.full((B, A, n_kp, 3), np.nan)
            colour = np.full((B, A), -1, dtype=np.int32)
            labels = [[None] * A for _ in range(B)]
            for b, ((i_frame, _), ks) in enumerate(zip(part, live)):
                for a, i in enumerate(ks[p0:p0 + A]):
                    kp3d[b, a] = p3d[first[b] + p0 + a]
                    colour[b, a] = int(Cid[keys[i]][i_frame])
                    labels[b][a] = str(keys[i])
            out = draw.render(out, 0, kp3d, np.ones((B, A, n_kp)), src_index=src_index, colour=colour, labels=labels,
                              label_scale=2.0, label_thickness=5)
            src_index = np.arange(B, dtype=np.int32)
        if (h_out, w_out) != (H, W):
            out = resize(out, h_out, w_out, device=device)
        for jpg, fn, t in zip(encode.encode(out), fns, store.frame_time[pos]):
            writer.append(jpg, fn, t)
    writer.close()
    return vid_path


def proc(data_name, result_dir_root, raw_data_dir, config_path, save_vid=False, save_vid_cam=2, rmse_thr=200.0,
         vidfile_prefix='', n_animal=4, n_kp=17, device=0, **vis_kw):
    """step3:30-34.  ``save_vid``: ``visualize`` for camera ``save_vid_cam`` on the rows main_proc returned;
    ``vis_kw`` are ``visualize``'s keyword options."""
    result_dir = result_dir_root + '/' + data_name
    Trk, Cid, T = main_proc(config_path, result_dir, rmse_thr=rmse_thr, device=device, n_animal=n_animal, n_kp=n_kp,
                            camparam=vis_kw.get('camparam'))
    if save_vid:
        visualize(save_vid_cam, config_path, result_dir, raw_data_dir, T=T, vidfile_prefix=vidfile_prefix,
                  device=device, **vis_kw)
    return Trk, Cid, T
