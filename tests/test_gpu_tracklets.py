"""GPU: mq_tracklet_traces / mq_tracklet_id_votes (csrc/tracklet.hip) against NumPy built from the oracle's
per-cell lift (``step3_scenes.OracleLift``: the reference's row gather, ``oracle.association.calc_3dpose`` at
score threshold 0.3, np.nanmedian / np.nanmean, count_id_detections' loop).

p3d, median and mean are held to the bound tests/test_gpu_geometry.py holds mq_triangulate_pinv to (1e-6 mm
absolute), the NaN pattern is identical, the votes are equal."""
import copy

import numpy as np
import pytest

from conftest import gpu_available
from step3_scenes import OracleLift

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

ATOL = 1e-6


def _rows(n_cam, n_animal, n_frame, seed):
    from mqhip import synth
    cams = synth.make_cameras(n_cam)
    skel = synth.make_skeletons(n_animal, n_frame, seed=seed)
    T = synth.make_alldata(cams, skel, p_seen=0.9, p_dup=0.1, seed=seed + 1)
    return cams, T


def _compare(cams, T, trk, n_kp=17):
    from mqhip import synth
    from mqhip.association import StepTwoCameras
    from mqhip.tracklets import TrackletLift
    camparam = synth.camparam_from_cams(cams)
    K, F, C = trk.shape
    cells = np.stack(np.meshgrid(np.arange(K), np.arange(F), indexing="ij"), axis=-1).reshape(-1, 2)
    ref = OracleLift(camparam, T, n_kp=n_kp)
    r_med, r_avg, r_p3d = ref.traces(trk, cells, return_p3d=True)
    r_votes = ref.id_votes(trk, cells)
    lift = TrackletLift(StepTwoCameras(camparam), T)
    med, avg, p3d = lift.traces(trk, cells, return_p3d=True)
    votes = lift.id_votes(trk, cells)
    assert lift.launches == 2
    for got, want in ((p3d, r_p3d), (med, r_med), (avg, r_avg)):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_allclose(got, want, rtol=0, atol=ATOL, equal_nan=True)
    np.testing.assert_array_equal(votes, r_votes)
    # the default cells: every frame inside each tracklet's interval, as (K, F, 3)
    m2, a2 = lift.traces({10 + k: trk[k] for k in range(K)})
    inside = np.zeros((K, F), bool)
    for k in range(K):
        on = np.nonzero((trk[k] >= 0).any(axis=1))[0]
        if len(on):
            inside[k, on[0]:on[-1] + 1] = True
    np.testing.assert_array_equal(m2[inside], med.reshape(K, F, 3)[inside])
    np.testing.assert_array_equal(a2[inside], avg.reshape(K, F, 3)[inside])
    assert np.isnan(m2[~inside]).all() and np.isnan(a2[~inside]).all()
    return ref, cells, r_med, r_avg, r_p3d, r_votes


def test_traces_and_votes_8_cameras_17_joints():
    n_cam, F, K = 8, 40, 5
    cams, T = _rows(n_cam, 4, F, seed=41)
    seen = lambda c, f, a: [i for i, tt in enumerate(T[c][f]) if tt[0] == a]
    trk = np.full((K, F, n_cam), -1, dtype=int)
    for a in range(4):
        trk[a] = a                              # track id == individual in these rows; unseen cameras find no row
    # -- a duplicate row with the same id: the last one wins for the pose, both count for the votes
    f_dup = next(f for f in range(F) if seen(0, f, 0))
    dup = copy.deepcopy(T[0][f_dup][seen(0, f_dup, 0)[0]])
    dup[5] = [[v[0] + 9.0, v[1] - 7.0, v[2]] for v in dup[5]]
    T[0][f_dup].append(dup)
    # -- a frame with no rows in one camera, and one with no rows at all
    T[2][7] = []
    for c in range(n_cam):
        T[c][30] = []
    # -- a joint with NaN x in all but one camera
    f_nan = 10
    first = True
    for c in range(n_cam):
        for i in seen(c, f_nan, 1):
            if not first:
                T[c][f_nan][i][5][4][0] = float("nan")
                T[c][f_nan][i][5][4][1] = float("nan")
            first = False
    # -- cells whose finite joints number 0, 1, 2 (even) and 3 (odd): only the first n joints stay
    for n_keep, f in ((0, 20), (1, 21), (2, 22), (3, 23)):
        for c in range(n_cam):
            for i in seen(c, f, 2):
                for j in range(n_keep, 17):
                    T[c][f][i][5][j][0] = float("nan")
                    T[c][f][i][5][j][1] = float("nan")
                for j in range(n_keep):
                    T[c][f][i][5][j][2] = 0.9
    # -- a trk entry of -2, a row id of -10 (met by a positive entry, and by an entry of -10: no match either way)
    trk[3, 15, 2] = -2
    T[4][12][0][0] = -10
    # -- tracklet 4: 0, 1 and 2 present cameras, then more, on individual 0's rows
    trk[4, 2, 0] = 0
    trk[4, 3, [0, 1]] = 0
    trk[4, 4:12, :] = 0
    trk[4, 12, :] = 0
    trk[4, 12, 4] = -10
    ref, cells, med, avg, p3d, votes = _compare(cams, T, trk)
    # the crafted cases are what they claim to be, on the NumPy side
    at = lambda k, f: k * F + f
    for n_keep, f in ((0, 20), (1, 21), (2, 22), (3, 23)):
        assert np.isfinite(p3d[at(2, f), :, 0]).sum() == n_keep
    assert np.isnan(med[at(2, 20)]).all() and np.isfinite(med[at(2, 21)]).all()
    assert np.isnan(med[at(4, 0)]).all() and np.isnan(med[at(4, 2)]).all()     # 0 and 1 present cameras
    assert np.isnan(avg[at(4, 2)]).all()
    assert np.isnan(med[at(0, 30)]).all()                                      # no rows at all
    assert votes[at(0, f_dup)].sum() >= 2 and votes.sum() > 100
    shifted = OracleLift(ref.camparam, T).p3d(trk[0, f_dup], f_dup)
    T[0][f_dup].pop()
    assert not np.allclose(OracleLift(ref.camparam, T).p3d(trk[0, f_dup], f_dup), shifted, atol=1e-3, equal_nan=True)


def test_traces_and_votes_2_cameras():
    cams, T = _rows(2, 2, 6, seed=43)
    trk = np.full((2, 6, 2), -1, dtype=int)
    trk[0], trk[1] = 0, 1
    trk[1, 4, 1] = -1
    _compare(cams, T, trk)


def test_traces_and_votes_1_joint():
    cams, T = _rows(8, 2, 6, seed=45)
    for cam in T:
        for rows in cam:
            for tt in rows:
                tt[5] = tt[5][:1]
    trk = np.full((2, 6, 8), -1, dtype=int)
    trk[0], trk[1] = 0, 1
    _compare(cams, T, trk, n_kp=1)
