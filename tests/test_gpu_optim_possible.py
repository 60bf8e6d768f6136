"""GPU optim_points_possible (mq_optim_points_possible, csrc/optim_possible.hip) against scipy on identical inputs,
and CameraGroup.triangulate_optim.

The problems are tests/golden/optim_possible_problems.npz (tools/dump_optim_possible_problems.py: synthetic
cameras, a 5-joint chain, decoy candidates; two animals per problem), with scipy's answer under the reference's
arguments (cameras.py:1473-1488; tests/possible_ref.py).  tests/test_optim_possible_ref.py re-runs scipy on the
CPU against the fixture.

Stated bounds (optim_points' own, tests/test_gpu_optim_trf.py; scipy's 2-point vs 3-point Jacobian moves its
answer by <= 0.013 mm on these problems, the dump tool refuses a problem where that reaches a quarter of a bound):
  * per problem and over all: distance to scipy's 2-point p3d <= 1 mm at the median, <= 5 mm at p99;
  * njev within +-1 of scipy's, nfev within +-2; cost under possible_ref's objective within 1e-4 relative;
  * argmax(alphas_norm) equals scipy's on every decided cell (scipy's largest weight >= 0.9);
  * alphas_norm is NaN exactly at NaN candidates and sums to 1 over a cell's other slots.

Measured on an MI355X (distance to scipy med / p99 mm, nfev GPU/scipy, njev GPU/scipy, lsmr iterations, cost
ratio, cells where the chosen slot differs from scipy's / decided cells):
  p0a0 0.0002 / 0.0012   7/7   7/7  1251  1.0000000  0/109     p0a1 0.0002 / 0.0006   7/7   7/7  1015  1.0000000  0/96
  p1a0 0.0001 / 0.0005   9/9   8/8  1873  1.0000000  0/148     p1a1 0.0001 / 0.0004 13/13 10/10  2127  1.0000027  0/138
  p2a0 0.0000 / 0.0001   7/7   7/7  1075  1.0000000  0/43      p2a1 0.0000 / 0.0001   7/7   7/7   945  1.0000000  0/39
  p3a0 0.0001 / 0.0006   7/7   7/7  2000  1.0000000  0/273     p3a1 0.0000 / 0.0001   7/7   7/7  2032  1.0000000  0/252
  all: median 0.0001, p99 0.0006, max 0.0014 mm.
Decoy scene (p3), distance to the truth, median / p99 mm: optim_points_possible 2.532 / 5.701 and 2.446 / 7.076
(scipy's the same to three decimals); optim_points on slot 0 from the same start 7.180 / 22.361 and 6.107 / 24.596.
"""
import functools
import os

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

FIX = os.path.join(os.path.dirname(__file__), "golden", "optim_possible_problems.npz")
MED_MM, P99_MM = 1.0, 5.0
N_PROBLEMS, N_ANIMALS = 4, 2
DECOY = 3  # 16 frames: four blocks of the solver's 4 frames per workgroup (F = 6: 4 + 2, F = 9: 4 + 4 + 1)


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(FIX)


def _group(C):
    from mqhip import synth
    from mqhip.geometry import CameraGroup
    return CameraGroup.from_dicts(synth.make_cameras(C))


def _run(i, animals):
    from mqhip.optim import optim_points_possible_batch
    z = _fixture()
    P2 = np.stack([z[f"p{i}a{k}_points"] for k in animals])
    I3 = np.stack([z[f"p{i}a{k}_init"] for k in animals])
    return optim_points_possible_batch(_group(P2.shape[1]), P2, I3, z[f"p{i}_cons"], z[f"p{i}_weak"],
                                       n_deriv_smooth=int(z[f"p{i}_nd"]), return_stats=True)


@functools.lru_cache(maxsize=None)
def _solve(i):
    """The problem's two animals in one call (computed once, shared by the tests; nobody writes into it)."""
    return _run(i, tuple(range(N_ANIMALS)))


def _cost(z, i, k, p3, an, jl):
    import possible_ref as pr
    from mqhip import synth
    from oracle.geometry import CameraGroupOracle
    pts = z[f"p{i}a{k}_points"]
    with np.errstate(divide="ignore"):
        raw = np.log(an[~np.isnan(pts[..., 0])]) / pr.BETA  # softmax(beta raw) = alphas_norm
    x = np.hstack([p3.ravel(), jl, raw])
    r = pr.error_fun(x, CameraGroupOracle(synth.make_cameras(pts.shape[0])), pts, z[f"p{i}_cons"], z[f"p{i}_weak"],
                     z[f"p{i}a{k}_stats"][4], 2, 0.5, 15, "soft_l1", int(z[f"p{i}_nd"]))
    return 0.5 * float(r @ r)


def test_possible_matches_scipy_on_fixture_problems():
    import possible_ref as pr
    z = _fixture()
    allv, rows = [], []
    for i in range(N_PROBLEMS):
        p3, an, jl, st, _ = _solve(i)
        for k in range(N_ANIMALS):
            key = f"p{i}a{k}"
            pts, ref = z[key + "_points"], z[key + "_x2"]
            C, F, J, P, _ = pts.shape
            d = np.linalg.norm(p3[k] - ref[:F * J * 3].reshape(F, J, 3), axis=-1).ravel()
            allv.append(d)
            nfev, njev, cost_ref = z[key + "_stats"][:3]
            cr = _cost(z, i, k, p3[k], an[k], jl[k]) / cost_ref
            rows.append((key, float(np.median(d)), float(np.percentile(d, 99)), int(st[k, 4]), int(nfev),
                         int(st[k, 5]), int(njev), int(st[k, 6]), cr, int(st[k, 3])))
            # the weights: NaN exactly at NaN candidates, rows summing to 1, scipy's choice on decided cells
            bad = np.isnan(pts[..., 0])
            np.testing.assert_array_equal(np.isnan(an[k]), bad)
            some = ~np.all(bad, axis=3)
            np.testing.assert_allclose(np.nansum(an[k], axis=3)[some], 1.0, rtol=0, atol=1e-12)
            aref = np.where(bad, -1.0, pr.alphas_out(pts, ref, z[f"p{i}_cons"], z[f"p{i}_weak"]))
            decided = (np.sum(~bad, axis=3) >= 2) & (aref.max(axis=3) >= 0.9)
            got = np.argmax(np.where(bad, -1.0, an[k]), axis=3)
            rows[-1] += (int(np.sum(got[decided] != np.argmax(aref, axis=3)[decided])), int(decided.sum()))
    for r in rows:
        print("%s med %.4f p99 %.4f mm  nfev %d/%d  njev %d/%d  lsmr %d  cost ratio %.7f  status %d  "
              "other slot than scipy on %d of %d decided cells" % r)
    allv = np.concatenate(allv)
    print("all: median %.4f p99 %.4f max %.4f mm" % (np.median(allv), np.percentile(allv, 99), allv.max()))
    for key, med, p99, nf, nf_ref, nj, nj_ref, _, cr, _, n_other, _ in rows:
        assert n_other == 0, (key, n_other)
        assert med <= MED_MM and p99 <= P99_MM, (key, med, p99)
        assert abs(nj - nj_ref) <= 1 and abs(nf - nf_ref) <= 2, (key, nf, nf_ref, nj, nj_ref)
        assert abs(cr - 1) <= 1e-4, (key, cr)
    assert np.median(allv) <= MED_MM and np.percentile(allv, 99) <= P99_MM


@pytest.mark.parametrize("i", [1, DECOY])
def test_possible_batch_equals_single_problem(i):
    """An animal solved alone equals the same animal inside the batch, bit for bit (per-animal per-block partials,
    reduced in block order; F = 9 has a one-frame tail block, F = 16 four full blocks)."""
    p3, an, jl, st, _ = _solve(i)
    q3, qa, ql, qs, _ = _run(i, (1,))
    np.testing.assert_array_equal(q3[0], p3[1])
    np.testing.assert_array_equal(qa[0], an[1])
    np.testing.assert_array_equal(ql[0], jl[1])
    np.testing.assert_array_equal(qs[0], st[1])


def test_possible_beats_slot0_on_decoy_scene():
    """What the soft choice buys: as close to the truth as scipy's answer (within the parity bounds), and closer
    at the median than optim_points on slot 0 alone from the same start."""
    from mqhip.optim import optim_points_batch
    z = _fixture()
    i = DECOY
    p3, _, _, _, _ = _solve(i)
    P2 = np.stack([z[f"p{i}a{k}_points"] for k in range(N_ANIMALS)])
    I3 = np.stack([z[f"p{i}a{k}_init"] for k in range(N_ANIMALS)])
    s3, _ = optim_points_batch(_group(P2.shape[1]), P2[:, :, :, :, 0], I3, z[f"p{i}_cons"], z[f"p{i}_weak"],
                               n_deriv_smooth=int(z[f"p{i}_nd"]), solver="trf")
    for k in range(N_ANIMALS):
        truth = z[f"p{i}a{k}_truth"]
        F, J, _ = truth.shape
        ref = z[f"p{i}a{k}_x2"][:F * J * 3].reshape(F, J, 3)
        dg = np.linalg.norm(p3[k] - truth, axis=-1).ravel()
        dr = np.linalg.norm(ref - truth, axis=-1).ravel()
        d0 = np.linalg.norm(s3[k] - truth, axis=-1).ravel()
        print("p%da%d to truth, median / p99 mm: possible %.3f / %.3f, scipy %.3f / %.3f, optim_points(slot 0) "
              "%.3f / %.3f" % (i, k, np.median(dg), np.percentile(dg, 99), np.median(dr), np.percentile(dr, 99),
                               np.median(d0), np.percentile(d0, 99)))
        assert np.median(dg) <= np.median(dr) + MED_MM
        assert np.percentile(dg, 99) <= np.percentile(dr, 99) + P99_MM
        assert np.median(d0) > np.median(dg)


def _clean_points(F=4, seed=11):
    from mqhip import synth
    cams = synth.make_cameras(8)
    skel = synth.make_skeletons(1, F, seed=seed)
    kp = synth.make_kp2d(cams, skel, noise_px=1.0, drop=0.1, seed=seed)[0]  # (F, C, J, 3), zero rows = missing
    pts = np.transpose(kp[..., :2], (1, 0, 2, 3)).copy()
    pts[np.transpose(kp[..., 2], (1, 0, 2)) == 0] = np.nan
    return cams, pts


CONS = [[5, 7], [7, 9], [6, 8], [8, 10]]


def test_triangulate_optim_is_triangulate_then_optim_points():
    from mqhip.geometry import CameraGroup
    cams, pts = _clean_points()
    g = CameraGroup.from_dicts(cams)
    C, F, J, _ = pts.shape
    got = g.triangulate_optim(pts, constraints=CONS)
    want = g.optim_points(pts, g.triangulate(pts.reshape(C, -1, 2)).reshape(F, J, 3), constraints=CONS)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


def test_triangulate_optim_init_ransac_uses_picked_points():
    from mqhip.geometry import CameraGroup
    cams, pts = _clean_points()
    g = CameraGroup.from_dicts(cams)
    C, F, J, _ = pts.shape
    got = g.triangulate_optim(pts, init_ransac=True, constraints=CONS)
    p3, _, p2, _ = g.triangulate_ransac(pts.reshape(C, -1, 2))
    want = g.optim_points(p2.reshape(pts.shape), p3.reshape(F, J, 3), constraints=CONS)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


def test_triangulate_optim_returns_initial_points_when_too_few(capsys):
    from mqhip.geometry import CameraGroup
    cams, pts = _clean_points(F=2)
    pts = pts[:, :, :9].copy()  # 2 frames x 9 joints = 18 points < 20
    g = CameraGroup.from_dicts(cams)
    C, F, J, _ = pts.shape
    got = g.triangulate_optim(pts, constraints=[[5, 7]])
    np.testing.assert_array_equal(got, g.triangulate(pts.reshape(C, -1, 2)).reshape(F, J, 3))
    assert "not enough 3D points" in capsys.readouterr().out
