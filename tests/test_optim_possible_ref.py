"""CPU: tests/possible_ref.py (the numpy restatement of CameraGroup.optim_points_possible, cameras.py:1417-1513)
checked against the oracle's optim_points residuals and scipy's finite differences; the fixture
tests/golden/optim_possible_problems.npz against scipy run here; the header / ctypes entry of
mq_optim_points_possible; and the argument checks that need no device."""
import os
import re

import numpy as np
import pytest

import possible_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "optim_possible_problems.npz")


def _problem(i, k, random_alphas=None):
    from mqhip import synth
    from oracle.geometry import CameraGroupOracle
    z = np.load(FIX)
    pts, init = z[f"p{i}a{k}_points"], z[f"p{i}a{k}_init"]
    cons, weak, nd = z[f"p{i}_cons"], z[f"p{i}_weak"], int(z[f"p{i}_nd"])
    cg = CameraGroupOracle(synth.make_cameras(pts.shape[0]))
    x0, ssf = pr.init_params(init, pts, cons, weak, 4)
    if random_alphas is not None:
        nn = pr.n_norm(pts, cons, weak)
        x0 = x0.copy()
        x0[nn:] = np.random.default_rng(random_alphas).uniform(-0.3, 0.3, x0.size - nn)
    args = (cg, pts, cons, weak, ssf, 2, 0.5, 15, "soft_l1", nd)
    return z, x0, args


def test_residuals_are_optim_points_on_soft_points_plus_std_rows():
    z, x, args = _problem(1, 0, random_alphas=0)
    cg, pts, cons, weak = args[:4]
    nn = pr.n_norm(pts, cons, weak)
    r = pr.error_fun(x, *args)
    an, bad, all_bad = pr.soft_weights(pts, x[nn:])
    # the weights by hand: softmax over the finite slots, the soft point their weighted mean
    c, f, j = (int(v[0]) for v in np.nonzero((~bad).sum(axis=3) == 2))
    e = np.where(bad[c, f, j], 0.0, np.exp(pr.BETA * _alphas_dense(pts, x[nn:])[c, f, j]))
    np.testing.assert_allclose(an[c, f, j], e / e.sum(), rtol=1e-15)
    soft = pr.soft_points(pts, an, bad, all_bad)
    np.testing.assert_allclose(soft[c, f, j], np.nansum(an[c, f, j][:, None] * pts[c, f, j], axis=0), rtol=1e-14)
    assert np.all(np.isnan(soft[all_bad])) and not np.any(np.isnan(soft[~all_bad]))
    base = cg._error_fun_triangulation(x[:nn], soft, cons, weak, *args[4:])
    np.testing.assert_array_equal(r[:base.size], base)
    std_rows = 10 * (1 - np.std(an[~all_bad], axis=1))
    np.testing.assert_array_equal(r[base.size:], std_rows)
    assert r.size == base.size + int((~all_bad).sum())
    assert pr.jac_sparsity(pts, cons, weak, args[-1]).shape == (r.size, x.size)


def _alphas_dense(pts, flat):
    a = np.zeros(pts.shape[:4])
    a[~np.isnan(pts[..., 0])] = flat
    return a


@pytest.mark.parametrize("i", [1, 2])
def test_analytic_jacobian_beats_two_point_differences_at_a_generic_point(i):
    from scipy.optimize._numdiff import approx_derivative, group_columns
    z, x, args = _problem(i, 0, random_alphas=i)
    pts, cons, weak = args[1:4]
    sp = pr.jac_sparsity(pts, cons, weak, args[-1])
    spg = (sp, group_columns(sp))
    fun = lambda v: pr.error_fun(v, *args)  # noqa: E731
    j2 = approx_derivative(fun, x, method="2-point", sparsity=spg).toarray()
    j3 = approx_derivative(fun, x, method="3-point", sparsity=spg).toarray()
    ja = pr.jac_analytic(x, *args)
    assert (abs(ja) > 0).multiply(sp == 0).nnz == 0  # inside the reference's pattern
    ja = ja.toarray()
    e_an, e_2p = np.abs(ja - j3).max(), np.abs(j2 - j3).max()
    print("max |J_an - J_3p| %.3e   max |J_2p - J_3p| %.3e" % (e_an, e_2p))
    assert e_an <= e_2p


def test_std_rows_take_the_forward_difference_at_x0():
    """At x0 every cell whose P slots are all finite has equal weights, where the std has a kink: the std rows'
    alpha columns equal scipy's 2-point ones, to the gap the two Jacobians show on all other entries."""
    from scipy.optimize._numdiff import approx_derivative, group_columns
    z, x0, args = _problem(1, 0)
    pts, cons, weak = args[1:4]
    sp = pr.jac_sparsity(pts, cons, weak, args[-1])
    fun = lambda v: pr.error_fun(v, *args)  # noqa: E731
    j2 = approx_derivative(fun, x0, method="2-point", sparsity=(sp, group_columns(sp))).toarray()
    ja = pr.jac_analytic(x0, *args).toarray()
    nn = pr.n_norm(pts, cons, weak)
    n_std = int(np.any(~np.isnan(pts[..., 0]), axis=3).sum())
    kink = np.zeros_like(ja, dtype=bool)
    kink[-n_std:, nn:] = True
    assert np.abs(ja[kink]).max() > 1  # the kink cells' entries are there (10 beta std(d a) of a full cell)
    gap_other = np.abs(ja - j2)[~kink].max()
    gap_kink = np.abs(ja - j2)[kink].max()
    print("max |J_an - J_2p|: std rows' alpha columns %.3e, every other entry %.3e" % (gap_kink, gap_other))
    assert gap_kink <= gap_other


@pytest.mark.parametrize("i,k", [(0, 0), (1, 1), (2, 0), (3, 1)])
def test_fixture_holds_scipys_answer(i, k):
    from mqhip import synth
    from oracle.geometry import CameraGroupOracle
    z = np.load(FIX)
    pts = z[f"p{i}a{k}_points"]
    cg = CameraGroupOracle(synth.make_cameras(pts.shape[0]))
    res, _, ssf = pr.optim_points_possible(cg, pts, z[f"p{i}a{k}_init"], z[f"p{i}_cons"], z[f"p{i}_weak"],
                                           n_deriv_smooth=int(z[f"p{i}_nd"]))
    np.testing.assert_array_equal(res.x, z[f"p{i}a{k}_x2"])
    nfev, njev, cost, status, ssf_fix = z[f"p{i}a{k}_stats"]
    assert (res.nfev, res.njev, res.status) == (int(nfev), int(njev), int(status)) and res.cost == cost
    assert ssf == ssf_fix


def test_fixture_covers_the_branches():
    z = np.load(FIX)
    counts = np.sum(~np.isnan(z["p1a0_points"][..., 0]), axis=3)
    assert set(np.unique(counts)) == {0, 1, 2, 3}          # cells with 3, 2, 1 and 0 finite slots
    assert len(z["p1_weak"]) == 1 and int(z["p2_nd"]) == 2 and z["p2a0_points"].shape[0] == 4
    assert z["p3a0_points"].shape[1] == 16                  # four blocks of the solver's 4 frames
    assert z["p0a0_points"].shape[1] == 6 and z["p1a0_points"].shape[1] == 9  # tail blocks of 2 and 1 frames
    for i in range(4):
        for k in range(2):
            pts = z[f"p{i}a{k}_points"]
            # the reference's own limit: slot 0 finite wherever any slot is
            assert not np.any(np.isnan(pts[:, :, :, 0, 0]) & ~np.all(np.isnan(pts[..., 0]), axis=3))


def test_entry_is_declared_exported_and_additive():
    from mqhip import _lib
    name = "mq_optim_points_possible"
    assert name in _lib.EXPORTED and name in _lib._SIGS
    header = open(os.path.join(ROOT, "include", "mq_hip.h")).read()
    m = re.search(r"int mq_optim_points_possible\(([^;]*)\);", header)
    assert m, "mq_optim_points_possible is not declared in include/mq_hip.h"
    assert len(m.group(1).split(",")) == len(_lib._SIGS[name][1])
    assert "cameras.py:1417-1513" in header and ":1622-1667" in header
    assert "#define MQ_ABI_VERSION 8" in header and _lib.ABI_VERSION == 8  # purely additive


def test_argument_checks_need_no_device():
    from mqhip import synth
    from mqhip.geometry import CameraGroup
    from mqhip.optim import optim_points_possible_batch
    g = CameraGroup.from_dicts(synth.make_cameras(8))
    pts = np.zeros((8, 6, 5, 2, 2))
    p3 = np.zeros((6, 5, 3))
    with pytest.raises(AssertionError, match="number of cameras"):
        g.optim_points_possible(pts[:7], p3)
    with pytest.raises(ValueError, match="n_possible"):
        g.optim_points_possible(np.zeros((8, 6, 5, 5, 2)), p3)
    with pytest.raises(NotImplementedError):
        g.optim_points_possible(pts, p3, scores=np.ones((8, 6, 5, 2)))
    with pytest.raises(ValueError, match="n_deriv_smooth"):
        g.optim_points_possible(pts[:, :2], p3[:2], n_deriv_smooth=2)
    with pytest.raises(ValueError, match="trf solver only"):
        optim_points_possible_batch(g, pts[None], p3[None], solver="lm")
    with pytest.raises(AssertionError, match="number of cameras"):
        g.triangulate_optim(np.zeros((7, 6, 5, 2)))
