"""GPU: more than one candidate per (instance, joint) -- the top-K heatmap peaks (mq_decode_udp_topk), the
n_possible > 1 Viterbi filter (mq_viterbi_filter_multi) and CameraGroup.triangulate_possible
(mq_triangulate_possible) against tests/cand_ref.py and the oracle."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

INPUT_SIZE = (192, 256)


# ------------------------------------------------------------------ decode
def _blob_heatmaps(n, J, h, w, seed):
    """_peaky_heatmaps of test_gpu_pose.py with two or three blobs of different heights per map."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    hm = rng.normal(0, 0.02, (n, J, h, w)).astype(np.float32)
    for i in range(n):
        for k in range(J):
            for amp in rng.permutation([1.0, 0.7, 0.45])[:rng.integers(2, 4)]:
                cx, cy = rng.uniform(-2, w + 1), rng.uniform(-2, h + 1)
                hm[i, k] += (amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * 2.0 ** 2))).astype(np.float32)
    return hm


_DECODE_CASES = {}


def _decode_case(name):
    """Inputs and the GPU single-candidate decode of a case, built once."""
    if name in _DECODE_CASES:
        return _DECODE_CASES[name]
    import torch
    from mqhip.pose import decode_heatmaps
    if name == "64x48":
        n, J, h, w = 4, 17, 64, 48
        hm = _blob_heatmaps(n, J, h, w, seed=11)
        hm[0, 3] = -np.abs(hm[0, 3])   # max <= 0 -> loc -1 + wrap-around reads in slot 0, no peaks
        hm[1, 0] = -np.abs(hm[1, 0])
        yy, xx = np.mgrid[0:h, 0:w]    # one clean blob: fewer peaks than slots
        hm[2, 5] = np.exp(-((xx - 20.3) ** 2 + (yy - 41.6) ** 2) / 8.0).astype(np.float32)
    else:
        n, J, h, w = 2, 3, 20, 12
        hm = _blob_heatmaps(n, J, h, w, seed=12)
    rng = np.random.default_rng(1)
    center = rng.uniform(100, 1500, (n, 2)).astype(np.float32)
    scale = rng.uniform(50, 400, (n, 2)).astype(np.float32)
    dev = [torch.from_numpy(a).cuda() for a in (hm, center, scale)]
    one = [t.cpu().numpy() for t in decode_heatmaps(*dev)]
    _DECODE_CASES[name] = (hm, center, scale, dev, one)
    return _DECODE_CASES[name]


@pytest.mark.parametrize("min_score", [0.0, 0.1])
@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("case", ["64x48", "20x12"])
def test_decode_topk(case, K, min_score):
    from cand_ref import topk_peaks_batch
    from mqhip.pose import decode_heatmaps_topk
    from oracle.decode import get_heatmap_maximum, refine_keypoints_dark_udp, to_image_space
    hm, center, scale, dev, one = _decode_case(case)
    n, J, h, w = hm.shape
    kp, score, peak, kp_hm = [t.cpu().numpy() for t in decode_heatmaps_topk(*dev, K, min_score=min_score)]
    assert kp.shape == (n, J, K, 2) and score.shape == (n, J, K) and peak.shape == (n, J, K)
    # the peak rule
    rpeak, rscore = topk_peaks_batch(hm, K, 3, min_score)
    np.testing.assert_array_equal(peak, rpeak)
    np.testing.assert_array_equal(score, rscore)
    if case == "64x48":
        assert (peak[0, 3, 1:] == -1).all() and (peak[1, 0, 1:] == -1).all() and (peak[2, 5, 1:] == -1).all()
        if K >= 3:
            assert (peak[:, :, 1] >= 0).sum() > n * J // 2      # the second blobs are found
    # slot 0 is mq_decode_udp, bit for bit
    for got, ref in zip((kp, score, peak, kp_hm), one):
        np.testing.assert_array_equal(got[:, :, 0], ref)
    # empty slots
    empty = peak < 0
    assert not empty[:, :, 0].any()
    assert np.isnan(kp[empty]).all() and np.isnan(kp_hm[empty]).all() and (score[empty] == 0).all()
    assert np.isfinite(kp[~empty]).all()
    # slots >= 1: the oracle's DARK-UDP step from the same peak locations (candidates on its instance axis).
    # Compared where the oracle's own step is defined to better than the tolerance, which is where the peak
    # is a blob (min_score 0.1: the blobs are >= 0.45 high, the noise peaks 5 sigma lower).  A noise peak
    # sits on the log map's clipped plateau log(1e-3): its Hessian is exactly 0, the step is the derivative
    # times 1 / eps = 8.4e6, and changing the log map by one float32 ulp moves the oracle's own result by up
    # to 7.6 px there (against <= 1e-5 px at every peak above 0.1), so at min_score 0 those slots are checked
    # for the peak, the score and finiteness only.  (Measured once at min_score 0: slots 1-2 of K = 3 within
    # 7.7e-5 of the oracle, slot 3 of K = 4 -- noise peaks -- 2.2e-3 off.)
    if min_score == 0.0:
        return
    for i in range(n):
        locs = np.zeros((K, J, 2), dtype=np.float32)
        locs[0] = get_heatmap_maximum(hm[i].copy())[0]
        for k in range(1, K):
            ok = peak[i, :, k] >= 0
            locs[k, ok, 0] = peak[i, ok, k] % w
            locs[k, ok, 1] = peak[i, ok, k] // w
        ref = refine_keypoints_dark_udp(locs.copy(), hm[i].copy())          # (K, J, 2)
        ref_in = ref / np.array([w - 1, h - 1]) * np.array(INPUT_SIZE)
        ref_img = to_image_space(ref_in, center[i], scale[i], INPUT_SIZE)
        for k in range(1, K):
            ok = peak[i, :, k] >= 0
            d_hm = np.abs(kp_hm[i, ok, k] - ref[k, ok])
            d_img = np.abs(kp[i, ok, k] - ref_img[k, ok])
            if ok.any():
                print(f"{case} K={K} min_score={min_score} inst {i} slot {k}: max|d kp_hm|={d_hm.max():.3e} "
                      f"max|d kp_img|={d_img.max():.3e}")
            np.testing.assert_allclose(kp_hm[i, ok, k], ref[k, ok], rtol=0, atol=2e-4)
            np.testing.assert_allclose(kp[i, ok, k], ref_img[k, ok], rtol=0, atol=2e-2)


def test_decode_slot0_edge_maps():
    """NaN pixels and an all-equal map through the argmax reduction that both decodes share: slot 0 stays the
    single-candidate result bit for bit (NaN in the same places), the argmax is np.argmax's."""
    import torch
    from cand_ref import topk_peaks
    from mqhip.pose import decode_heatmaps, decode_heatmaps_topk
    rng = np.random.default_rng(21)
    hm = rng.normal(0, 0.02, (1, 3, 20, 12)).astype(np.float32)
    hm[0, 0, 7, 5] = hm[0, 0, 11, 2] = np.nan       # the first NaN is the argmax: 7 * 12 + 5
    hm[0, 1] = 0.25                                   # every pixel ties: index 0
    center = rng.uniform(100, 1500, (1, 2)).astype(np.float32)
    scale = rng.uniform(50, 400, (1, 2)).astype(np.float32)
    dev = [torch.from_numpy(a).cuda() for a in (hm, center, scale)]
    one = [t.cpu().numpy() for t in decode_heatmaps(*dev)]
    want = [int(np.argmax(hm[0, j].reshape(-1))) for j in range(3)]
    assert want[:2] == [89, 0]
    np.testing.assert_array_equal(one[2][0], want)
    for K in (1, 2, 3, 4):
        kp, score, peak, kp_hm = [t.cpu().numpy() for t in decode_heatmaps_topk(*dev, K)]
        for got, ref in zip((kp, score, peak, kp_hm), one):
            np.testing.assert_array_equal(got[:, :, 0], ref)
        np.testing.assert_array_equal(peak[0, :, 0], want)
        for j in range(3):
            rpeak, rscore = topk_peaks(hm[0, j], K)
            np.testing.assert_array_equal(peak[0, j], rpeak)
            np.testing.assert_array_equal(score[0, j], rscore)
        assert (peak[0, :2, 1:] == -1).all() and (score[0, :2, 1:] == 0).all()   # NaN maximum / one plateau
        assert np.isnan(score[0, 0, 0]) and score[0, 1, 0] == np.float32(0.25)


def test_decode_topk_model_api_default_unchanged():
    import torch
    from mqhip.pose import VitPoseHip
    from mqhip.weights import VIT_TINY, make_random_weights
    hm, center, scale, dev, one = _decode_case("64x48")
    model = VitPoseHip(VIT_TINY, make_random_weights(VIT_TINY, seed=0, device="cuda"), graph=False)
    out = model.decode(*dev)
    assert out[0].shape == (4, 17, 2)
    for got, ref in zip(out, one):
        np.testing.assert_array_equal(got.cpu().numpy(), ref)
    out3 = model.decode(*dev, n_candidates=3)
    assert out3[0].shape == (4, 17, 3, 2) and out3[2].dtype == torch.int32
    np.testing.assert_array_equal(out3[0][:, :, 0].cpu().numpy(), one[0])
    with pytest.raises(ValueError):
        model.decode(*dev, n_candidates=5)


# ------------------------------------------------------------------ Viterbi
def _cfg(n_back, thr=0.3, off=25):
    return {"filter": {"score_threshold": thr, "n_back": n_back, "offset_threshold": off, "multiprocessing": False}}


_VIT_INPUT = {}


def _viterbi_input(K):
    """(1, 40, 2, 5, K, 3): synth.make_kp2d in slot 0 plus decoys, with the hand-made cases."""
    if K in _VIT_INPUT:
        return _VIT_INPUT[K]
    from mqhip import synth
    cams = synth.make_cameras(8)[:2]
    skel = synth.make_skeletons(1, 40)
    base = synth.make_kp2d(cams, skel, drop=0.2, seed=5)[:, :, :, :5]        # (1, 40, 2, 5, 3)
    rng = np.random.default_rng(7)
    kp = np.zeros(base.shape[:4] + (K, 3))
    kp[..., 0, :] = base
    for k in range(1, K):
        kp[..., k, :2] = base[..., :2] + rng.normal(0, 80, base[..., :2].shape)
        kp[..., k, 2] = rng.uniform(0.2, 0.9, base.shape[:4])
        kp[..., k, :][rng.uniform(0, 1, base.shape[:4]) < 0.3] = 0.0
    kp[0, 3, 1, 1, K - 1, :2] = np.nan                                       # NaN coordinates, valid score
    # below the threshold in slot 0, a valid one in slot 1
    kp[0, 5, 0, 0, 0] = [300, 200, 0.1]
    kp[0, 5, 0, 0, 1] = [310, 205, 0.8]
    # gaps 4, 4 (and so 8): the second and the third are dropped
    kp[0, 7, 0, 1, :, :] = 0
    for k in range(min(K, 3)):
        kp[0, 7, 0, 1, k] = [400 + 4 * k, 250, 0.9 - 0.1 * k]
    # five frames with nothing valid
    kp[0, 10:15, 1, 2] = 0
    # a 400 px jump
    kp[0, 20, 1, 3, 0, :2] += 400
    kp[0, 20, 1, 3, 0, 2] = 0.9
    # an exact tie: one point, then two equal candidates left and right of it
    # (in the last two frames, so that no later frame breaks it)
    kp[0, 36:40, 0, 4] = 0
    kp[0, 38, 0, 4, 0] = [100, 50, 0.7]
    kp[0, 39, 0, 4, 0] = [90, 50, 0.6]
    kp[0, 39, 0, 4, 1] = [110, 50, 0.6]
    _VIT_INPUT[K] = kp
    return kp


def _oracle_viterbi(kp, n_back):
    """oracle.viterbi.filter_pose_viterbi per (animal, camera) on (A, F, C, J, K, 3) -> (A, F, C, J, 3)."""
    from oracle.viterbi import filter_pose_viterbi
    A, F, C, J, K, _ = kp.shape
    out = np.zeros((A, F, C, J, 3))
    for a in range(A):
        for c in range(C):
            pts, sc = filter_pose_viterbi(_cfg(n_back), np.array(kp[a, :, c], dtype=np.float64, copy=True), [])
            out[a, :, c, :, :2] = pts
            out[a, :, c, :, 2] = sc
    return out


@pytest.mark.parametrize("n_back", [1, 2, 3])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_viterbi_multi_matches_oracle(K, n_back):
    from mqhip.geometry import viterbi_filter
    kp = _viterbi_input(K)
    for F in (40, 1, 2):
        sub = np.ascontiguousarray(kp[:, :F])
        got = viterbi_filter(sub, n_back=n_back)
        assert got.shape == sub.shape[:4] + (3,)
        ref = _oracle_viterbi(sub, n_back)
        np.testing.assert_array_equal(got[..., :2], ref[..., :2])
        np.testing.assert_array_equal(got[..., 2], ref[..., 2])
    # the tie: (90, 50) and (110, 50) are equally far from (100, 50); the first wins
    full = viterbi_filter(kp, n_back=n_back)
    np.testing.assert_array_equal(full[0, 39, 0, 4], [90, 50, 0.6])


@pytest.mark.parametrize("n_back", [1, 3])
def test_viterbi_multi_k1_equals_single(n_back):
    from mqhip import synth
    from mqhip.geometry import viterbi_filter
    cams = synth.make_cameras(8)
    kp2d = synth.make_kp2d(cams, synth.make_skeletons(2, 40), drop=0.3, seed=5)
    kp2d[0, 10:14, 2, 3] = 0
    kp2d[1, 20, 4, 5, :2] += 400
    one = viterbi_filter(kp2d, n_back=n_back)
    np.testing.assert_array_equal(viterbi_filter(kp2d[:, :, :, :, None], n_back=n_back), one)


def test_step4_filter_2d_accepts_candidates():
    from mqhip import synth
    from src.pipeline.step4_aniposefiltering import filter_2d
    cams = synth.make_cameras(8)[:3]
    kp2d = synth.make_kp2d(cams, synth.make_skeletons(2, 20), drop=0.3, seed=6)
    ref = filter_2d(kp2d)
    got = filter_2d(kp2d[:, :, :, :, None])
    assert got.shape == ref.shape == (20, 17, 2, 3, 3)
    np.testing.assert_array_equal(got, ref)
    kp2 = np.concatenate([kp2d[:, :, :, :, None], np.zeros_like(kp2d)[:, :, :, :, None]], axis=4)
    assert filter_2d(kp2).shape == ref.shape


def test_filter_pose_wrapper_three_candidates():
    from oracle.viterbi import filter_pose_viterbi as oracle_fpv
    from src.third_party.anipose.filter_pose import filter_pose_viterbi
    kp = _viterbi_input(3)
    mine = np.array(kp[0, :, 0], dtype=np.float64, copy=True)       # (F, J, 3, 3)
    theirs = mine.copy()
    pts, sc = filter_pose_viterbi(_cfg(3), mine, [])
    rpts, rsc = oracle_fpv(_cfg(3), theirs, [])
    np.testing.assert_array_equal(pts, rpts)
    np.testing.assert_array_equal(sc, rsc)
    np.testing.assert_array_equal(mine, theirs)                      # the NaNs written into the input
    assert np.isnan(mine[5, 0, 0, 0])
    with pytest.raises(ValueError):
        filter_pose_viterbi(_cfg(3), np.zeros((4, 2, 5, 3)), [])


def _decoy_track(seed, F=60):
    """A sigma = 3 px random walk with scores U(0.5, 0.8); in 20 % of the frames (never the first three) a
    decoy 150-300 px away scores 0.1 higher and sits in slot 0, the true point in slot 1."""
    rng = np.random.default_rng(seed)
    truth = np.array([500.0, 400.0]) + np.cumsum(rng.normal(0, 3.0, (F, 2)), axis=0)
    sc = rng.uniform(0.5, 0.8, F)
    kp = np.zeros((1, F, 1, 1, 2, 3))
    kp[0, :, 0, 0, 0, :2] = truth
    kp[0, :, 0, 0, 0, 2] = sc
    bad = rng.uniform(0, 1, F) < 0.2
    bad[:3] = False
    for f in np.flatnonzero(bad):
        ang = rng.uniform(0, 2 * np.pi)
        r = rng.uniform(150, 300)
        kp[0, f, 0, 0, 1] = kp[0, f, 0, 0, 0]
        kp[0, f, 0, 0, 0, :2] = truth[f] + r * np.array([np.cos(ang), np.sin(ang)])
        kp[0, f, 0, 0, 0, 2] = sc[f] + 0.1
    return kp, truth, bad


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_viterbi_candidates_recover_the_track(seed):
    from mqhip.geometry import viterbi_filter
    kp, truth, bad = _decoy_track(seed)
    assert bad.sum() >= 5
    got = viterbi_filter(kp)[0, :, 0, 0, :2]
    d2 = np.linalg.norm(got - truth, axis=1)
    one = viterbi_filter(np.ascontiguousarray(kp[:, :, :, :, 0]))[0, :, 0, 0, :2]
    d1 = np.linalg.norm(one - truth, axis=1)
    print(f"seed {seed}: within 1 px, two candidates {np.mean(d2 <= 1):.3f}, slot 0 alone {np.mean(d1 <= 1):.3f}")
    assert (d2 <= 1.0).all()
    assert not (d1 <= 1.0).all()


# ------------------------------------------------------------------ triangulate_possible
_TRI = {}


def _tri_scene(C, P, N):
    """True projections (0.2 px noise) in a random slot, decoys N(0, 60 px) elsewhere, 15 % of all slots NaN,
    point 0 seen by no camera, point 1 by one."""
    key = (C, P, N)
    if key in _TRI:
        return _TRI[key]
    from mqhip import synth
    from mqhip.geometry import CameraGroup
    from oracle.geometry import CameraGroupOracle
    cams = synth.make_cameras(8)[:C]
    g, o = CameraGroup.from_dicts(cams), CameraGroupOracle(cams)
    X = synth.make_skeletons(1, (N + 16) // 17).reshape(-1, 3)[:N]
    rng = np.random.default_rng(100 * C + 10 * P + N)
    uv = o.project(X)                                                        # (C, N, 2)
    pts = uv[:, :, None, :] + rng.normal(0, 60, (C, N, P, 2))
    slot = rng.integers(0, P, (C, N))
    ci, ni = np.meshgrid(np.arange(C), np.arange(N), indexing="ij")
    pts[ci, ni, slot] = uv + rng.normal(0, 0.2, uv.shape)
    pts[rng.uniform(0, 1, (C, N, P)) < 0.15] = np.nan
    pts[:, 0] = np.nan
    pts[1:, 1] = np.nan
    pts[0, 1, 0] = uv[0, 1]
    _TRI[key] = (g, o, pts)
    return _TRI[key]


@pytest.mark.parametrize("min_cams", [2, 3])
@pytest.mark.parametrize("C,P,N", [(4, 2, 51), (4, 3, 34), (5, 2, 17)])
def test_triangulate_possible_matches_oracle(C, P, N, min_cams):
    g, o, pts = _tri_scene(C, P, N)
    p3, picked, p2, err = g.triangulate_possible(pts, min_cams=min_cams)
    r3, rpicked, r2, rerr = o.triangulate_possible(pts, min_cams=min_cams)
    assert picked.shape == (C, N, P) and picked.dtype == bool
    np.testing.assert_array_equal(picked, rpicked)
    np.testing.assert_array_equal(p2, r2)
    assert np.array_equal(np.isnan(p3), np.isnan(r3))
    np.testing.assert_allclose(p3, r3, rtol=0, atol=1e-6, equal_nan=True)
    np.testing.assert_allclose(err, rerr, rtol=1e-9, atol=1e-9)
    assert np.isnan(p3[0]).all() and np.isnan(p3[1]).all() and not picked[:, :2].any()
    assert np.isfinite(p3[2:]).mean() > 0.8 and (picked.sum(axis=2) <= 1).all()


def test_triangulate_possible_p1_equals_ransac():
    from mqhip import synth
    from mqhip.geometry import CameraGroup
    cams = synth.make_cameras(8)
    g = CameraGroup.from_dicts(cams)
    kp2d = synth.make_kp2d(cams, synth.make_skeletons(2, 6), seed=3)
    A, F, C, J, _ = kp2d.shape
    p = kp2d.transpose(2, 0, 1, 3, 4).reshape(C, A * F * J, 3).copy()
    pts = p[..., :2].copy()
    pts[p[..., 2] < 0.5] = np.nan
    pts[:, 0] = np.nan
    pts[1:, 1] = np.nan
    for min_cams in (2, 3):
        a = g.triangulate_ransac(pts, min_cams=min_cams)
        b = g.triangulate_possible(pts[:, :, None], min_cams=min_cams)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


def _nine_camera_scene():
    """C = 9 (the MAXC = 16 kernel instances), N = 12, P = 2, the points of _tri_scene: each is seen by camera 8
    and three of cameras 0..7, point 0 by none.  Returns g, o, the true-slot points (9, 12, 2) and all
    candidates (9, 12, 2, 2)."""
    key = "nine"
    if key in _TRI:
        return _TRI[key]
    from mqhip import synth
    from mqhip.geometry import CameraGroup
    from oracle.geometry import CameraGroupOracle
    C, N, P = 9, 12, 2
    cams = synth.make_cameras(C)
    g, o = CameraGroup.from_dicts(cams), CameraGroupOracle(cams)
    X = synth.make_skeletons(1, 1).reshape(-1, 3)[:N]
    rng = np.random.default_rng(100 * C + 10 * P + N)
    uv = o.project(X)                                                        # (C, N, 2)
    true = uv + rng.normal(0, 0.2, uv.shape)
    pts = uv[:, :, None, :] + rng.normal(0, 60, (C, N, P, 2))
    slot = rng.integers(0, P, (C, N))
    ci, ni = np.meshgrid(np.arange(C), np.arange(N), indexing="ij")
    pts[ci, ni, slot] = true
    seen = np.zeros((C, N), dtype=bool)
    seen[8] = True
    for n in range(N):
        seen[rng.choice(8, 3, replace=False), n] = True
    seen[:, 0] = False
    pts[~seen] = np.nan
    true[~seen] = np.nan
    _TRI[key] = (g, o, true, pts)
    return _TRI[key]


def test_ransac_nine_cameras():
    g, o, pts, _ = _nine_camera_scene()
    for min_cams in (2, 3):
        p3, picked, p2, err = g.triangulate_ransac(pts, min_cams=min_cams)
        r3, rpicked, r2, rerr = o.triangulate_ransac(pts, min_cams=min_cams)
        np.testing.assert_array_equal(picked, rpicked)
        assert np.array_equal(np.isnan(p3), np.isnan(r3))
        np.testing.assert_allclose(p3, r3, rtol=0, atol=1e-6, equal_nan=True)
        np.testing.assert_allclose(err, rerr, rtol=1e-9, atol=1e-9)
        np.testing.assert_array_equal(p2, r2)
        assert np.isnan(r3[0]).all() and np.isfinite(r3[1:]).all() and rpicked[8, 1:].all()   # the scene


def test_possible_nine_cameras():
    g, o, one, pts = _nine_camera_scene()
    C, N, P = pts.shape[:3]
    for min_cams in (2, 3):
        a = g.triangulate_ransac(one, min_cams=min_cams)
        b = g.triangulate_possible(one[:, :, None], min_cams=min_cams)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        p3, picked, p2, err = g.triangulate_possible(pts, min_cams=min_cams)
        r3, rpicked, r2, rerr = o.triangulate_possible(pts, min_cams=min_cams)
        assert picked.shape == (C, N, P) and picked.dtype == bool
        np.testing.assert_array_equal(picked, rpicked)
        np.testing.assert_array_equal(p2, r2)
        assert np.array_equal(np.isnan(p3), np.isnan(r3))
        np.testing.assert_allclose(p3, r3, rtol=0, atol=1e-6, equal_nan=True)
        np.testing.assert_allclose(err, rerr, rtol=1e-9, atol=1e-9)
        assert np.isnan(p3[0]).all() and not picked[:, 0].any() and (picked.sum(axis=2) <= 1).all()


def test_triangulate_possible_limits():
    from mqhip import synth
    from mqhip.geometry import CameraGroup
    g = CameraGroup.from_dicts(synth.make_cameras(8))
    with pytest.raises(ValueError):
        g.triangulate_possible(np.zeros((8, 3, 4, 2)))          # 5^8 combinations per point
    with pytest.raises(ValueError):
        g.triangulate_possible(np.zeros((8, 3, 5, 2)))
    with pytest.raises(NotImplementedError):
        g.triangulate_possible(np.zeros((8, 3, 2, 2)), undistort=False)


# ------------------------------------------------------------------ heatmaps -> candidates -> Viterbi
def test_chain_heatmap_candidates_through_viterbi():
    import torch
    from mqhip.geometry import viterbi_filter
    from mqhip.pose import decode_heatmaps_topk
    F, J, h, w = 30, 2, 64, 48
    yy, xx = np.mgrid[0:h, 0:w]

    def blob(cx, cy, amp):
        return (amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 8.0)).astype(np.float32)

    true_c = np.zeros((F, J, 2))
    decoy_c = np.zeros((F, J, 2))
    hm = np.zeros((F, J, h, w), dtype=np.float32)
    decoy_frame = np.arange(F) % 5 == 4
    for f in range(F):
        for j in range(J):
            true_c[f, j] = (8 + f, 12 + 10 * j) if j == 0 else (40 - f, 22)
            decoy_c[f, j] = true_c[f, j] + (0, 20)
            hm[f, j] = blob(*true_c[f, j], 0.7)
            if decoy_frame[f]:
                hm[f, j] += blob(*decoy_c[f, j], 0.8)
    # image pixel = 4 x heatmap pixel
    center = np.tile(np.array([[94.0, 126.0]], dtype=np.float32), (F, 1))
    scale = np.tile(np.array([[188.0, 252.0]], dtype=np.float32), (F, 1))
    kp, score, peak, _ = decode_heatmaps_topk(torch.from_numpy(hm).cuda(), torch.from_numpy(center).cuda(),
                                              torch.from_numpy(scale).cuda(), 2)
    kp, score = kp.cpu().numpy(), score.cpu().numpy()
    cand = np.concatenate([kp, score[..., None].astype(np.float64)], axis=-1)      # (F, J, 2, 3)
    out = viterbi_filter(np.ascontiguousarray(cand[None, :, None]))[0, :, 0]        # (F, J, 3)
    d_true = np.linalg.norm(out[..., :2] - 4 * true_c, axis=-1)
    d_decoy = np.linalg.norm(out[..., :2] - 4 * decoy_c, axis=-1)
    assert (d_true < d_decoy).all()
    s0_true = np.linalg.norm(kp[:, :, 0] - 4 * true_c, axis=-1)
    s0_decoy = np.linalg.norm(kp[:, :, 0] - 4 * decoy_c, axis=-1)
    np.testing.assert_array_equal(s0_decoy < s0_true, np.repeat(decoy_frame[:, None], J, axis=1))
