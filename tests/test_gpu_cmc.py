"""GPU: camera-motion compensation (csrc/cmc.hip, mqhip.cmc) against the numpy restatement tests/cmc_ref.py and
known answers.  delta_dog = 4 x the restatement's own float32-vs-float64 DoG deviation (3.6e-4 on the standard
small image); e_ref = 0.26 px is the restatement's corner error on the standard pair."""
import numpy as np
import pytest

from conftest import gpu_available

import cmc_ref as R
from test_cmc_ref import ransac_case

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]


@pytest.fixture(scope="module")
def std():
    """Standard pair, its small image, the restatement's pyramid / keypoints / descriptors on it."""
    f0, f1, truth = R.standard_pair()
    small = R.preprocess(f0)
    mask = R.make_mask(*small.shape, None)
    pyr = R.build_pyramid(small)
    det = R.sift_detect(small, -1, mask, pyr)
    return dict(f0=f0, f1=f1, truth=truth, small=small, mask=mask, pyr=pyr, det=det,
                delta_dog=4 * R.dog_precision(small))


def test_preprocess_bit_exact(std):
    from mqhip import cmc
    np.testing.assert_array_equal(cmc.preprocess(std["f0"][None])[0], std["small"])
    rng = np.random.default_rng(0)
    for shape in ((37, 53, 3), (35, 55, 3)):      # odd sizes; 35 / 55 put the last tap on the clamped edge
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        np.testing.assert_array_equal(cmc.preprocess(img[None])[0], R.preprocess(img))


def test_dog_pyramid_within_delta(std):
    from mqhip import cmc
    _, dogs = cmc.sift_detect(std["small"][None], -1, with_dog=True)
    ref = std["pyr"][1]
    assert [d.shape for d in dogs[0]] == [d.shape for d in ref]
    err = max(float(np.abs(a - b).max()) for a, b in zip(dogs[0], ref))
    print("dog max |diff|", err, "delta_dog", std["delta_dog"])
    assert err <= std["delta_dog"]


def _match_sets(a, b, tol_px):
    """Greedy pairing of keypoint rows of the same octave / layer whose positions and angles agree."""
    used, pairs = set(), []
    for i, p in enumerate(a):
        for j, q in enumerate(b):
            dang = abs((p[3] - q[3] + 180) % 360 - 180)
            if j not in used and p[4] == q[4] and p[5] == q[5] and abs(p[0] - q[0]) <= tol_px \
                    and abs(p[1] - q[1]) <= tol_px and dang <= 0.05:
                used.add(j)
                pairs.append((i, j))
                break
    return pairs


def test_keypoints_six_blobs():
    from mqhip import cmc
    img, _ = R.six_blob_image()
    ref = R.sift_detect(img, 0)["kps"]
    got = cmc.sift_detect(img[None], 0)[0]
    lr = np.unique(ref[:, [4, 5, 1, 0]], axis=0)
    lg = np.unique(got[:, [4, 5, 1, 0]], axis=0)
    assert lr.shape == lg.shape == (6, 4)
    np.testing.assert_array_equal(lr[:, :2], lg[:, :2])          # same octave and layer
    assert np.abs(lr[:, 2:] - lg[:, 2:]).max() < 1e-3


def test_keypoints_standard_image(std):
    """Shared keypoints agree to 0.01 px / 0.05 deg; a keypoint on one side only is fragile (< 16 delta_dog).

    The precondition that at most 5 % of the restatement's keypoints on the chosen frame be fragile does not hold
    for this family of frames: measured on the CPU 20.3 % at seed 7 (71 of 350) and 9.3 % - 20 % over seeds
    1 .. 15 (lowest: seed 8), the 26-neighbour gap and the 0.5 px refinement-offset limit alone exceeding 5 %
    (blobs of sigma 1.2 - 4.5 small-image px are smooth at the pixel scale, so an extremum sits between two
    pixels of nearly equal DoG value as often as not).  The seed and the 16 delta_dog cap stay as set; so that
    the fragile share cannot excuse more than the 5 % it was meant to, the one-sided keypoints are also held to
    5 % of the total here."""
    from mqhip import cmc
    ref, margin = std["det"]["kps"], std["det"]["margin"]
    got = cmc.sift_detect(std["small"][None], -1, std["mask"][None])[0]
    pairs = _match_sets(ref, got, 0.01)
    only_ref = sorted(set(range(len(ref))) - {i for i, _ in pairs})
    only_gpu = sorted(set(range(len(got))) - {j for _, j in pairs})
    print("ref", len(ref), "gpu", len(got), "shared", len(pairs), "only ref", only_ref, "only gpu", only_gpu)
    lim = 16 * std["delta_dog"]
    assert all(margin[i] < lim for i in only_ref)
    assert len(only_ref) + len(only_gpu) <= 0.05 * len(ref)
    # a GPU-only keypoint must sit on a fragile decision of the restatement: a fragile keypoint or rejected
    # candidate of it
    n_fragile = int((margin < lim).sum()) + int((std["det"]["rejected"] < lim).sum())
    assert len(only_gpu) <= n_fragile
    if not only_ref and not only_gpu:
        np.testing.assert_array_equal(ref[:, 4:6], got[:, 4:6])  # then the order is the same too
    # the mask: nothing in the 2 % border
    px, py = np.rint(got[:, 0]).astype(int), np.rint(got[:, 1]).astype(int)
    assert (std["mask"][py, px] != 0).all()


def test_descriptors_within_one_unit(std):
    from mqhip import cmc
    kps = std["det"]["kps"]
    ref = R.sift_describe(std["small"], kps, -1, std["pyr"])
    got = cmc.sift_describe(std["small"][None], [kps], -1)[0]
    d = np.abs(ref.astype(int) - got.astype(int))
    print("descriptor max |diff|", d.max(), "entries differing", int((d > 0).sum()), "of", d.size)
    assert d.max() <= 1


def test_matcher_equals_restatement():
    from mqhip import cmc
    rng = np.random.default_rng(1)
    q = rng.integers(0, 256, (300, 128), dtype=np.uint8)
    t = rng.integers(0, 256, (257, 128), dtype=np.uint8)
    t[200] = t[17]                       # a tie for every query: index 17 must come before 200
    q[5] = t[17]
    for qq, tt in ((q, t), (q[:1], t[:2]), (q[:0], t), (q[:3], t[:0]), (q[:2], t[:1])):
        gi, gd = cmc.match_knn2(qq, tt)
        ri, rd = R.match_knn2(qq, tt)
        np.testing.assert_array_equal(gi, ri)
        np.testing.assert_array_equal(gd, rd)
    gi, gd = cmc.match_knn2(q, t)
    assert gi[5].tolist() == [17, 200] and gd[5].tolist() == [0, 0]


@pytest.mark.parametrize("n_in,n_out", [(40, 15), (100, 15), (5, 0), (4, 0)])
def test_ransac_equals_restatement(n_in, n_out):
    from mqhip import cmc
    src, dst, mask, W = ransac_case(n_in, n_out)
    ref = R.affine_partial_ransac(src, dst)
    got = cmc.affine_partial_ransac(src, dst)
    assert got["hyp"] == ref["hyp"] and got["n_inliers"] == ref["n_inliers"]
    np.testing.assert_array_equal(got["mask"], ref["mask"])
    assert np.abs(got["warp"] - ref["warp"]).max() <= 1e-9
    if n_in > 4:
        assert np.abs(got["warp"] - W).max() <= 1e-9
    else:
        np.testing.assert_array_equal(got["warp"], np.eye(2, 3))


E_REF = 0.26   # tests/test_cmc_ref.py::test_end_to_end_standard_pair


def test_end_to_end_and_determinism(std):
    from mqhip.cmc import SiftCmc
    c = SiftCmc(1536, 2048)
    np.testing.assert_array_equal(c.apply(std["f0"]), np.eye(2, 3))       # first call
    w = c.apply(std["f1"])
    err = R.corner_error(w, std["truth"])
    print("corner error", err, c.stats[0])
    assert err <= 3 * E_REF and err < 10.0
    c2 = SiftCmc(1536, 2048)
    c2.apply(std["f0"])
    np.testing.assert_array_equal(c2.apply(std["f1"]), w)                  # bit-identical warp
    assert c2.stats == c.stats
    c2.reset()
    np.testing.assert_array_equal(c2.apply(std["f1"]), np.eye(2, 3))       # after reset: no previous frame


def test_stage_determinism(std):
    from mqhip import cmc
    a = cmc.sift_detect(std["small"][None], -1, std["mask"][None])[0]
    b = cmc.sift_detect(std["small"][None], -1, std["mask"][None])[0]
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(cmc.sift_describe(std["small"][None], [a], -1)[0],
                                  cmc.sift_describe(std["small"][None], [a], -1)[0])


def test_flat_image_is_identity():
    from mqhip.cmc import SiftCmc
    flat = np.full((480, 640, 3), 117, np.uint8)
    c = SiftCmc(480, 640)
    c.apply(flat)
    np.testing.assert_array_equal(c.apply(flat), np.eye(2, 3))
    assert c.stats[0]["n_kp"] == 0


def _pan_frames(n, step=(90.0, -40.0), height=1536, width=2048):
    blobs = R.blob_field()
    return [R.render_blobs(blobs, height, width, warp=np.array([[1, 0, -k * step[0]], [0, 1, -k * step[1]]], float))
            for k in range(n)]


@pytest.fixture(scope="module")
def pan():
    return _pan_frames(8)


def test_batched_slots_equal_single_runs(std, pan):
    from mqhip.cmc import SiftCmc
    first = [std["f0"], pan[0], pan[3]]
    second = [std["f1"], pan[1], pan[5]]
    dets = [None, np.array([[300.0, 300, 700, 800]]), np.array([[100.0, 200, 400, 500], [900, 900, 1200, 1300]])]
    cb = SiftCmc(1536, 2048, n_slots=3)
    cb.apply_batch(np.stack(first), dets)
    wb = cb.apply_batch(np.stack(second), dets)
    for i in range(3):
        c = SiftCmc(1536, 2048)
        c.apply(first[i], dets[i])
        np.testing.assert_array_equal(c.apply(second[i], dets[i]), wb[i])
        assert c.stats[0] == cb.stats[i]
    assert np.abs(wb[1][:, 2] - [-90, 40]).max() < 1.0 and np.abs(wb[2][:, 2] - [-180, 80]).max() < 1.0


def test_mask_excludes_boxes(std):
    from mqhip import cmc
    dets = np.array([[400.0, 300.0, 900.0, 800.0], [1200.0, 100.0, 1800.0, 600.0]])
    mask = R.make_mask(*std["small"].shape, dets)
    got = cmc.sift_detect(std["small"][None], -1, mask[None])[0]
    px, py = np.rint(got[:, 0]).astype(int), np.rint(got[:, 1]).astype(int)
    assert len(got) > 50 and (mask[py, px] != 0).all()
    inside = (got[:, 0] >= 40.5) & (got[:, 0] < 89.5) & (got[:, 1] >= 30.5) & (got[:, 1] < 79.5)
    assert not inside.any()
    # through SiftCmc: the boxes reach the mask kernel (fewer keypoints than without)
    from mqhip.cmc import SiftCmc
    c = SiftCmc(1536, 2048)
    c.apply(std["f0"], dets)
    assert c.stats[0]["n_kp"] == len(got)


def test_tracker_keeps_ids_under_a_pan(pan):
    """Three boxes fixed in the world, the camera panning (90, -40) px per frame, step 1's BOTSORT_CFG: with the
    SIFT warp the ids [1, 2, 3] hold on all 8 frames; with the identity warp they are lost."""
    from mqhip.cmc import SiftCmc
    from mqhip.tracker import BotSort, make_cmc
    from src.pipeline.step1_proc2d import BOTSORT_CFG
    world = np.array([[900.0, 500, 1000, 620], [1300, 300, 1390, 400], [1000, 900, 1110, 1000]])

    def dets(k):
        b = world - np.array([90.0 * k, -40.0 * k, 90.0 * k, -40.0 * k])
        return np.hstack([b, np.full((3, 1), 0.95), np.zeros((3, 1))])

    tr = BotSort(**BOTSORT_CFG, cmc=SiftCmc(1536, 2048))
    ident = BotSort(**BOTSORT_CFG)
    for k in range(8):
        rows = tr.update(dets(k), pan[k])
        assert sorted(rows[:, 4].astype(int).tolist()) == [1, 2, 3], (k, rows)
        r0 = ident.update(dets(k), pan[k])
        assert len(r0) == 3 if k == 0 else len(r0) < 3, (k, r0)   # rows on the first frame, then the tracks are lost
    with pytest.raises(ValueError):
        make_cmc("orb", 1536, 2048)


def test_track_stores_with_sift(pan):
    import torch
    from src.pipeline import step1_proc2d as s1
    world = np.array([[900.0, 500, 1000, 620], [1300, 300, 1390, 400]])

    class Store:
        def get_frame_metadata(self):
            return dict(frame_time=np.arange(3) / 24.0, frame_number=np.arange(3))

        def image(self, fn):
            return pan[fn]

    class Det:
        dev = torch.device("cuda:0")
        k = 0

        def forward(self, fr):
            b = world - np.array([90.0 * self.k, -40.0 * self.k, 90.0 * self.k, -40.0 * self.k])
            self.k += 1
            return (torch.tensor(b[None], dtype=torch.float32), torch.full((1, 2), 0.95), torch.tensor([2]))

    T = np.arange(3) / 24.0
    rows = s1.track_stores(Det(), [Store()], T, cmc="sift")[0]
    assert sorted(rows) == [0, 1, 2]
    for fn in range(3):
        assert sorted(rows[fn][:, 4].astype(int).tolist()) == [1, 2]
    rows0 = s1.track_stores(Det(), [Store()], T)[0]
    assert len(rows0[1]) == 0                       # the identity path loses them
