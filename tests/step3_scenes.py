"""Helpers of the step-3 tests (not a test module): seeded scenes for the cross-frame matching, the
oracle's per-cell lift (the trace provider the host tests inject), and the fixture reader.

A scene is ``mqhip.synth`` cameras / skeletons / step-1 rows, with the rows' box ids renumbered per camera
and a list of events that break what a clean recording would give step 3:

* ``["switch", cam, animal, frame]``   the animal's box id in the camera changes from ``frame`` on;
* ``["swap", cam, a1, a2, frame]``     two animals exchange their box ids in the camera from ``frame`` on;
* ``["noid", animal]``                 the animal's ID scores are 0.5 everywhere (never a confident vote);
* ``["dup", cam, animal, f0, f1]``     in frames [f0, f1) the animal's row is followed by a shifted copy with
                                       the same box id (and the same confident ID);
* ``["kf_drop", i_kf, animal]``        the animal is missing from keyframe ``i_kf``'s record;
* ``["kf_split", i_kf, animal, cams]`` the animal appears in keyframe ``i_kf`` as two people, the first
                                       holding the listed cameras and the second the rest.

The keyframe records (step 2's ``match_keyframe.pickle``) are built from the truth every 12 frames from
frame 1, people seen by fewer than two cameras left out as step 2 does.
"""
import copy
import json
import os
import warnings

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYFRAME_STEP = 12

RECIPES = {
    # a keyframe without animal 1 (break -> stitch -> breakdown), a mid-clip id switch, an unlabelled animal
    "a": {"seed": 21, "n_frame": 205, "n_cam": 8, "n_animal": 4, "p_seen": 0.95, "p_dup": 0.1,
          "events": [["kf_drop", 7, 1], ["switch", 2, 0, 100], ["switch", 5, 2, 55], ["noid", 3],
                     ["dup", 1, 2, 40, 90]]},
    # two animals swap a camera's box ids between keyframes; a split keyframe pair gives overlapping tracklets
    "b": {"seed": 33, "n_frame": 217, "n_cam": 8, "n_animal": 4, "p_seen": 0.95, "p_dup": 0.05,
          "events": [["swap", 3, 0, 1, 80], ["kf_split", 8, 2, [0, 1, 2, 3, 4]], ["kf_split", 9, 2, [0, 1, 2]],
                     ["noid", 1], ["dup", 6, 0, 10, 30], ["kf_drop", 4, 3]]},
}


def build_scene(recipe):
    """(cams, T, keyframes): synthetic cameras, the rows T[c][f] and the keyframe records of a recipe."""
    from mqhip import synth
    A, F, C = recipe["n_animal"], recipe["n_frame"], recipe["n_cam"]
    cams = synth.make_cameras(C)
    skel = synth.make_skeletons(A, F, seed=recipe["seed"])
    T = synth.make_alldata(cams, skel, p_seen=recipe["p_seen"], p_dup=recipe["p_dup"], seed=recipe["seed"] + 1)
    owner = [[[(r[0] if r[0] < 10 else -1) for r in rows] for rows in cam] for cam in T]
    # per-camera numbering: animal a is box 1 + (a + c) % A in camera c, spurious detections 20 + a
    for c in range(C):
        for f in range(F):
            for r in T[c][f]:
                r[0] = 1 + (r[0] + c) % A if r[0] < 10 else 20 + (r[0] - 10)
    fresh = 30
    kf_events = []
    for ev in recipe["events"]:
        kind = ev[0]
        if kind == "switch":
            _, c, a, f0 = ev
            for f in range(f0, F):
                for r, o in zip(T[c][f], owner[c][f]):
                    if o == a:
                        r[0] = fresh
            fresh += 1
        elif kind == "swap":
            _, c, a1, a2, f0 = ev
            id1, id2 = 1 + (a1 + c) % A, 1 + (a2 + c) % A
            for f in range(f0, F):
                for r, o in zip(T[c][f], owner[c][f]):
                    if o == a1 and r[0] == id1:
                        r[0] = id2
                    elif o == a2 and r[0] == id2:
                        r[0] = id1
        elif kind == "noid":
            for c in range(C):
                for f in range(F):
                    for r, o in zip(T[c][f], owner[c][f]):
                        if o == ev[1]:
                            r[7] = 0.5
        elif kind == "dup":
            _, c, a, f0, f1 = ev
            for f in range(f0, f1):
                for i, o in enumerate(list(owner[c][f])):
                    if o == a:
                        r = copy.deepcopy(T[c][f][i])
                        r[5] = [[v[0] + 6.0, v[1] - 4.0, v[2]] for v in r[5]]
                        T[c][f].append(r)
                        owner[c][f].append(a)
        else:
            kf_events.append(ev)

    keyframes = []
    for i_kf, f in enumerate(range(1, F - KEYFRAME_STEP, KEYFRAME_STEP)):
        people = []
        for a in range(A):
            bc = -np.ones(C, dtype=int)
            for c in range(C):
                for r, o in zip(T[c][f], owner[c][f]):
                    if o == a:
                        bc[c] = r[0]
            parts = [bc]
            for ev in kf_events:
                if ev[1] != i_kf or ev[2] != a:
                    continue
                if ev[0] == "kf_drop":
                    parts = []
                elif ev[0] == "kf_split":
                    first = bc.copy()
                    second = bc.copy()
                    keep = np.zeros(C, bool)
                    keep[ev[3]] = True
                    first[~keep] = -1
                    second[keep] = -1
                    parts = [first, second]
            people += [p for p in parts if np.sum(p >= 0) >= 2]
        keyframes.append({"frame": f, "bcomb": people, "pose3d": [None] * len(people)})
    return cams, T, keyframes


class OracleLift:
    """The trace provider of the host tests: per cell the reference's Python gather (the last row carrying the
    box id wins) and ``oracle.association.calc_3dpose`` at score threshold 0.3, reduced by np.nanmedian /
    np.nanmean; the votes by count_id_detections' loop.  Same interface as ``mqhip.tracklets.TrackletLift``."""

    def __init__(self, camparam, T, n_kp=17, n_class=6, conf_thr=0.8):
        self.camparam, self.T = camparam, T
        self.n_cam, self.n_frame, self.n_kp = len(T), len(T[0]), n_kp
        self.n_class, self.conf_thr = n_class, conf_thr
        self._cache = {}
        self.cells_lifted = 0

    def _cells(self, Trk, cells):
        from mqhip.tracklets import interval_cells, trk_array
        keys, trk = trk_array(Trk, self.n_frame, self.n_cam)
        full = cells is None
        cells = interval_cells(trk) if full else np.asarray(cells, dtype=np.int64).reshape(-1, 2)
        return keys, trk, cells, full

    def p3d(self, ids, f):
        from oracle.association import calc_3dpose
        key = (tuple(int(i) for i in ids), int(f))
        if key not in self._cache:
            p2d = np.full((self.n_cam, self.n_kp, 3), np.nan)
            for c in range(self.n_cam):
                for tt in self.T[c][f]:
                    if ids[c] >= 0 and tt[0] == ids[c]:
                        p2d[c] = np.array(tt[5], dtype=np.float64)
            self._cache[key] = calc_3dpose(p2d, self.camparam, thr_kp=0.3)
            self.cells_lifted += 1
        return self._cache[key]

    def traces(self, Trk, cells=None, return_p3d=False):
        keys, trk, cells, full = self._cells(Trk, cells)
        med = np.full((len(cells), 3), np.nan)
        avg = np.full((len(cells), 3), np.nan)
        p3 = np.full((len(cells), self.n_kp, 3), np.nan)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for n, (k, f) in enumerate(cells):
                p = self.p3d(trk[k, f], f)
                avg[n] = np.nanmean(p, axis=0)
                if np.sum(trk[k, f] >= 0) >= 2:
                    med[n] = np.nanmedian(p, axis=0)
                    p3[n] = p
        if full:
            M = np.full((len(keys), self.n_frame, 3), np.nan)
            Av = np.full((len(keys), self.n_frame, 3), np.nan)
            M[cells[:, 0], cells[:, 1]] = med
            Av[cells[:, 0], cells[:, 1]] = avg
            med, avg = M, Av
        return (med, avg, p3) if return_p3d else (med, avg)

    def id_votes(self, Trk, cells=None):
        keys, trk, cells, full = self._cells(Trk, cells)
        votes = np.zeros((len(cells), self.n_class), dtype=np.int64)
        for n, (k, f) in enumerate(cells):
            for c in range(self.n_cam):
                for tt in self.T[c][f]:
                    if trk[k, f, c] >= 0 and tt[0] == trk[k, f, c] and tt[7] > self.conf_thr \
                            and 0 <= int(tt[6]) < self.n_class:
                        votes[n, int(tt[6])] += 1
        if full:
            V = np.zeros((len(keys), self.n_frame, self.n_class), dtype=np.int64)
            V[cells[:, 0], cells[:, 1]] = votes
            votes = V
        return votes


# ----------------------------------------------------------------------------- fixtures

def pack_tracks(D):
    """{k: array} -> (keys int64 (K,), stacked int16 array); every box / label id fits int16."""
    keys = np.array(list(D.keys()), dtype=np.int64)
    vals = np.stack([np.asarray(D[k]) for k in D.keys()]) if len(keys) else np.zeros((0,), dtype=np.int16)
    assert np.all(np.abs(vals) < 2 ** 15)
    return keys, vals.astype(np.int16)


def unpack_tracks(keys, vals):
    return {int(k): np.asarray(v, dtype=int) for k, v in zip(keys, vals)}


def pack_lists(L):
    """A list of int lists -> (flat, lengths)."""
    return (np.array([x for l in L for x in l], dtype=np.int64).reshape(-1),
            np.array([len(l) for l in L], dtype=np.int64))


def unpack_lists(flat, lengths):
    out, i = [], 0
    for n in lengths:
        out.append([int(x) for x in flat[i:i + n]])
        i += n
    return out


def load_fixture(name):
    """The recorded reference run of scene ``name``: recipe, input digest, final and intermediate results."""
    z = np.load(os.path.join(GOLDEN, f"step3_scene_{name}.npz"))
    fx = {"recipe": json.loads(str(z["recipe"])), "digest": str(z["digest"])}
    for key in ("trk_final", "cid_final", "trk_tracklets", "trk_trimmed", "cid_first", "cid_second"):
        fx[key] = unpack_tracks(z[key + "_keys"], z[key + "_vals"])
    fx["connection"] = [[[int(p), int(q)] for p, q in np.asarray(unpack_lists(z["conn_flat"], z["conn_len"])[i],
                                                                 dtype=int).reshape(-1, 2)]
                        for i in range(len(z["conn_len"]))]
    fx["trim_rmse"] = z["trim_rmse"]
    fx["graph"] = z["graph"]
    fx["paths"] = unpack_lists(z["paths_flat"], z["paths_len"])
    return fx


def scene_digest(T, keyframes):
    """SHA-256 of the packed rows and the keyframe records."""
    import hashlib

    from mqhip.tracklets import pack_rows
    h = hashlib.sha256(pack_rows(T).digest().encode())
    for kf in keyframes:
        h.update(np.int64(kf["frame"]).tobytes())
        for p in kf["bcomb"]:
            h.update(np.asarray(p, dtype=np.int64).tobytes())
    return h.hexdigest()
