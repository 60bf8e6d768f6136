"""CPU: the numpy restatement of boxmot's SIFT camera-motion compensation (tests/cmc_ref.py), pinned by known
answers.  Figures measured with it on the standard pair (blob field seed 7; rotation 0.5 deg, scale 1.01,
t = (93, -41) px): 350 / 322 keypoints (first / second frame, the second under the border mask too), 254 good
matches, all inliers, corner error e_ref = 0.26 px; DoG float32-vs-float64 deviation 8.9e-5, so
delta_dog = 4 x that = 3.6e-4."""
import numpy as np
import pytest

import cmc_ref as R


def test_preprocess_constant_ramp_and_size():
    img = np.full((60, 80, 3), 100, np.uint8)
    assert (R.preprocess(img) == 100).all()
    f0, _, _ = R.standard_pair()
    assert R.preprocess(f0).shape == (154, 205)          # 205 x 154 for 2048 x 1536
    # horizontal integer ramp: dst x reads (src 10 x + 4, 10 x + 5) with equal weights -> rint-half-up of the mean
    ramp = np.repeat(np.arange(200, dtype=np.uint8)[None, :, None], 50, 0).repeat(3, 2)
    out = R.preprocess(ramp)
    assert out.shape == (5, 20)
    gray = R.bgr_to_gray(ramp)[0].astype(np.int64)
    want = (gray[4::10] + gray[5::10] + 1) >> 1
    np.testing.assert_array_equal(out, np.broadcast_to(want, out.shape))
    # gray rule
    px = np.array([[[10, 200, 30]]], np.uint8)
    assert R.bgr_to_gray(px)[0, 0] == (10 * 1868 + 200 * 9617 + 30 * 4899 + 8192) >> 14


def test_detector_six_blobs():
    """One extremum per blob at the blob centre.  A circular blob has a 4-fold symmetric orientation
    histogram, so its orientation peaks come in fours: the locations are compared, not the angles."""
    img, centres = R.six_blob_image()
    d = R.sift_detect(img, 0)
    loc = np.unique(d["kps"][:, [0, 1, 4, 5]], axis=0)
    assert len(loc) == 6
    want = np.array(sorted(centres), np.float64)
    got = np.array(sorted(map(tuple, loc[:, :2])), np.float64)
    assert np.abs(got - want).max() < 1e-3
    geom = d["margin"][d["kind"] != "ori"]
    assert len(geom) == 0 or geom.min() > 1e-2            # the non-orientation decisions are far from their limits


@pytest.mark.parametrize("deg", [0, 90])
def test_orientation_of_windowed_ramp(deg):
    yy, xx = np.mgrid[0:128, 0:128].astype(np.float64) - 64
    t = np.deg2rad(deg)
    # SIFT's gradient has dy = I(y-1) - I(y+1): an image rising towards smaller y has orientation 90 deg
    ramp = xx * np.cos(t) - yy * np.sin(t)
    img = np.clip(np.rint(128 + 3.0 * ramp * np.exp(-(xx ** 2 + yy ** 2) / (2 * 12.0 ** 2))), 0, 255).astype(np.uint8)
    gauss, _ = R.build_pyramid(img, 0)
    hist, _ = R._orientation_hist(gauss[0][2], 64, 64, 12, np.float32(4.0))
    j = int(np.argmax(hist))
    assert j == deg // 10
    hl, hr, hj = hist[(j - 1) % 36], hist[(j + 1) % 36], hist[j]
    b = j + 0.5 * (hl - hr) / (hl - 2 * hj + hr)
    assert abs(b - deg / 10) < 0.05                       # the centre of its 10 degree bin


def test_ratio_test_in_integers():
    # 100 d1^2 < 81 d2^2: d2^2 = 10000 puts the boundary at d1^2 = 8100
    assert R.ratio_ok(8099, 10000) and not R.ratio_ok(8100, 10000) and not R.ratio_ok(8101, 10000)
    assert not R.ratio_ok(0, 0) and R.ratio_ok(0, 1)
    big = 128 * 255 * 255
    assert R.ratio_ok(int(big * 0.81) - 1, big) and not R.ratio_ok(int(np.ceil(big * 0.81)), big)


def ransac_case(n_in, n_out, seed=0):
    rng = np.random.default_rng(seed)
    src = rng.uniform(0, 200, (n_in + n_out, 2))
    W = R.similarity(7.0, 1.05, (12.5, -30.25))
    dst = src @ W[:, :2].T + W[:, 2]
    dst[n_in:] += rng.uniform(30, 80, (n_out, 2)) * rng.choice([-1, 1], (n_out, 2))
    perm = rng.permutation(n_in + n_out)
    mask = np.arange(n_in + n_out) < n_in
    return src[perm], dst[perm], mask[perm], W


@pytest.mark.parametrize("n_in,n_out", [(40, 15), (100, 15)])
def test_ransac_recovers_similarity(n_in, n_out):
    src, dst, mask, W = ransac_case(n_in, n_out)
    n = n_in + n_out
    assert (n * (n - 1) // 2 <= R.MAX_HYP) == (n_in == 40)   # every pair / the hashed pairs
    res = R.affine_partial_ransac(src, dst)
    np.testing.assert_array_equal(res["mask"], mask)
    assert res["n_inliers"] == n_in
    assert np.abs(res["warp"] - W).max() < 1e-9


def test_ransac_identity_boundary():
    src, dst, _, W = ransac_case(5, 0)
    assert np.abs(R.affine_partial_ransac(src, dst)["warp"] - W).max() < 1e-9
    r4 = R.affine_partial_ransac(src[:4], dst[:4])
    np.testing.assert_array_equal(r4["warp"], np.eye(2, 3))
    assert r4["hyp"] == -1


def test_knn2_ties_take_the_lower_index():
    t = np.zeros((4, 128), np.uint8)
    t[1, 0] = t[2, 0] = 3
    t[3, 0] = 1
    idx, dist = R.match_knn2(np.zeros((1, 128), np.uint8) + np.eye(1, 128, dtype=np.uint8) * 3, t)
    assert idx.tolist() == [[1, 2]] and dist.tolist() == [[0, 0]]
    idx, dist = R.match_knn2(np.zeros((1, 128), np.uint8), t[:1])
    assert idx.tolist() == [[0, -1]] and dist.tolist() == [[0, -1]]


def test_end_to_end_standard_pair():
    f0, f1, truth = R.standard_pair()
    c = R.SiftCmcRef()
    np.testing.assert_array_equal(c.apply(f0), np.eye(2, 3))   # first call: the identity
    w = c.apply(f1)
    e_ref = R.corner_error(w, truth)
    print("e_ref", e_ref, c.stats)
    assert e_ref < 10.0                                   # one small-image pixel
    assert c.stats["n_good"] > 4 and c.stats["n_inliers"] > 4


def test_flat_image_gives_identity():
    flat = np.full((1536, 2048, 3), 117, np.uint8)
    c = R.SiftCmcRef()
    c.apply(flat)
    np.testing.assert_array_equal(c.apply(flat), np.eye(2, 3))
    assert c.stats["n_good"] < 5


def test_mask_border_and_boxes():
    m = R.make_mask(154, 205, np.array([[400.0, 300.0, 900.0, 800.0, 0.9, 0]]))
    assert m[:3].max() == 0 and m[150:].max() == 0 and m[:, :4].max() == 0 and m[:, 200:].max() == 0
    assert m[30:80, 40:90].max() == 0 and m[29, 40] == 255 and m[80, 40] == 255 and m[50, 39] == 255 and m[50, 90] == 255
