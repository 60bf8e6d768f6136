"""TEST INFRASTRUCTURE ONLY -- numpy restatement of CameraGroup.optim_points_possible (aniposelib
cameras.py:1417-1513): the error function (_error_fun_triangulation_possible :1622-1667), the initialisation
(_initialize_params_triangulation_possible :1699-1712), the sparsity pattern (_jac_sparsity_triangulation_possible
:1795-1847), the analytic Jacobian the GPU solver uses (csrc/optim_possible.hip), and a driver that hands the
problem to scipy.optimize.least_squares with the reference's arguments.  The reference module itself needs numba
and cv2; this file is the yardstick of tests/test_optim_possible_ref.py and tests/test_gpu_optim_possible.py.

Layouts (the reference's):
  params  [p3d (F J 3), strong lengths, weak lengths, one alpha per non-NaN candidate in C-order of
           (camera, frame, joint, slot)]
  rows    [reprojection (cells with a finite candidate, C-order, u then v), smoothness, strong lengths
           (constraint-major), weak lengths, one std row per cell with a finite candidate]
The reference builds its pattern from slot 0, so it only works when slot 0 is finite wherever any slot is; on
such inputs "cells with a finite candidate" and "cells with a finite slot 0" are the same set.
"""
from math import comb

import numpy as np
from scipy import optimize
from scipy.sparse import coo_matrix

from oracle.geometry import optim_init

BETA = 5  # cameras.py:1470


def _bad(points):
    return np.isnan(points[..., 0])


def soft_weights(points, alphas_flat, beta=BETA):
    """alphas_norm (C, F, J, P) with 0 at NaN candidates (:1641-1653), and the bad / all_bad masks."""
    bad = _bad(points)
    all_bad = np.all(bad, axis=3)
    alphas = np.zeros(points.shape[:4], dtype='float64')
    alphas[~bad] = alphas_flat
    alphas_exp = np.exp(beta * alphas)
    alphas_exp[bad] = 0
    alphas_sum = np.sum(alphas_exp, axis=3)
    alphas_sum[all_bad] = 1
    return alphas_exp / alphas_sum[:, :, :, None], bad, all_bad


def soft_points(points, alphas_norm, bad, all_bad):
    """The soft 2D point per cell (:1656-1659), NaN where every slot is NaN."""
    p2ds_test = np.copy(points)
    p2ds_test[bad] = 0
    p2ds_adj = np.sum(alphas_norm[:, :, :, :, None] * p2ds_test, axis=3)
    p2ds_adj[all_bad] = np.nan
    return p2ds_adj


def n_norm(points, constraints, constraints_weak):
    C, F, J, P, _ = points.shape
    return F * J * 3 + len(constraints) + len(constraints_weak)


def error_fun(params, cg, points, constraints, constraints_weak, scale_smooth, scale_length, scale_length_weak,
              reproj_error_threshold, reproj_loss, n_deriv_smooth, beta=BETA):
    """_error_fun_triangulation_possible: the optim_points residuals on the soft points, then the std rows."""
    nn = n_norm(points, constraints, constraints_weak)
    an, bad, all_bad = soft_weights(points, params[nn:], beta)
    p2 = soft_points(points, an, bad, all_bad)
    errors = cg._error_fun_triangulation(np.array(params[:nn]), p2, constraints, constraints_weak, scale_smooth,
                                         scale_length, scale_length_weak, reproj_error_threshold, reproj_loss,
                                         n_deriv_smooth)
    errors_alphas = (1 - np.std(an[~all_bad], axis=1)) * 10
    return np.hstack([errors, errors_alphas])


def init_params(p3ds, points, constraints, constraints_weak, scale_smooth):
    """x0 (optim_points' initialisation, then a zero per finite candidate) and scale_smooth_full."""
    x0, ssf = optim_init(p3ds, np.asarray(constraints).reshape(-1, 2), np.asarray(constraints_weak).reshape(-1, 2),
                         scale_smooth)
    return np.hstack([x0, np.zeros(int(np.sum(~_bad(points))))]), ssf


class _Index:
    """Row and column numbers of a problem."""

    def __init__(self, points, constraints, constraints_weak, n_deriv_smooth):
        C, F, J, P, _ = points.shape
        self.C, self.F, self.J, self.P, self.n = C, F, J, P, n_deriv_smooth
        self.cons = np.vstack([np.asarray(constraints, dtype=int).reshape(-1, 2),
                               np.asarray(constraints_weak, dtype=int).reshape(-1, 2)])
        self.nS = len(constraints)
        good = ~_bad(points)
        self.good = good
        self.any_good = np.any(good, axis=3)
        self.cell_rank = (np.cumsum(self.any_good.ravel()) - 1).reshape(C, F, J)
        self.n_cells = int(self.any_good.sum())
        self.r_smooth = 2 * self.n_cells
        self.r_len = self.r_smooth + (F - n_deriv_smooth) * J * 3
        self.r_alpha = self.r_len + len(self.cons) * F
        self.m = self.r_alpha + self.n_cells
        self.c_len = F * J * 3
        self.c_alpha = self.c_len + len(self.cons)
        self.alpha_rank = (np.cumsum(good.ravel()) - 1).reshape(C, F, J, P)
        self.nv = self.c_alpha + int(good.sum())


def _entries(ix, vals):
    """COO triplets of the Jacobian; vals None gives the pattern (ones)."""
    C, F, J, P, n = ix.C, ix.F, ix.J, ix.P, ix.n
    rows, cols, data = [], [], []

    def add(r, c, v):
        r, c = np.broadcast_arrays(np.asarray(r), np.asarray(c))
        rows.append(r.ravel())
        cols.append(c.ravel())
        data.append(np.ones(r.size) if v is None else np.broadcast_to(v, r.shape).ravel())

    cc, ff, jj = np.nonzero(ix.any_good)
    rk = ix.cell_rank[cc, ff, jj]
    for comp in range(2):
        for k in range(3):
            add(2 * rk + comp, (ff * J + jj) * 3 + k, None if vals is None else vals['jx'][cc, ff, jj, comp, k])
    gc, gf, gj, gp = np.nonzero(ix.good)
    grk = ix.cell_rank[gc, gf, gj]
    acol = ix.c_alpha + ix.alpha_rank[gc, gf, gj, gp]
    for comp in range(2):
        add(2 * grk + comp, acol, None if vals is None else vals['ja'][gc, gf, gj, comp, gp])
    add(ix.r_alpha + grk, acol, None if vals is None else vals['ja'][gc, gf, gj, 2, gp])
    fr = np.arange(F - n)
    for m in range(n + 1):
        coef = (-1.0) ** (n - m) * comb(n, m)
        for q in range(J * 3):
            add(ix.r_smooth + fr * J * 3 + q, (fr + m) * J * 3 + q, None if vals is None else coef * vals['ssf'])
    fa = np.arange(F)
    for l, (a, b) in enumerate(ix.cons):
        r = ix.r_len + l * F + fa
        add(r, ix.c_len + l, None if vals is None else vals['dL'][l])
        for k in range(3):
            add(r, (fa * J + a) * 3 + k, None if vals is None else vals['dX'][l, :, k])
            add(r, (fa * J + b) * 3 + k, None if vals is None else -vals['dX'][l, :, k])
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(data)


def jac_sparsity(points, constraints, constraints_weak, n_deriv_smooth=1):
    """The pattern of _jac_sparsity_triangulation_possible (from the cells with a finite candidate; see above)."""
    ix = _Index(points, constraints, constraints_weak, n_deriv_smooth)
    r, c, d = _entries(ix, None)
    return coo_matrix((d, (r, c)), shape=(ix.m, ix.nv)).tocsr()


def _loss(e, rp, loss):
    """rho(|e|) and its derivative by e."""
    a, sg = np.abs(e), np.where(e < 0, -1.0, 1.0)
    if loss == 'soft_l1':
        s = np.sqrt(1 + a / rp)
        return rp * 2 * (s - 1), sg / s
    if loss == 'huber':
        big = a > rp
        sa = np.where(big, a, rp)
        return np.where(big, rp * (2 * np.sqrt(sa / rp) - 1), a), np.where(big, sg * np.sqrt(rp / sa), sg)
    return a, sg


def jac_analytic(params, cg, points, constraints, constraints_weak, scale_smooth, scale_length, scale_length_weak,
                 reproj_error_threshold, reproj_loss, n_deriv_smooth, beta=BETA, h=1e-3):
    """The Jacobian of error_fun as the GPU solver states it (scipy sparse, the reference's row / column order).
    The camera models' d(u, v)/dX is a central difference of the oracle's projection here (step h mm: its error is
    far below a 2-point difference's); everything else is closed form.  Where a cell's P weights are exactly
    equal the std is not differentiable: the std row takes the right-hand derivative std_P(d a / d alpha_k),
    which is what forward differences see there."""
    ix = _Index(points, constraints, constraints_weak, n_deriv_smooth)
    C, F, J, P = ix.C, ix.F, ix.J, ix.P
    nn = ix.c_alpha
    p3d = np.asarray(params[:F * J * 3]).reshape(F * J, 3)
    an, bad, all_bad = soft_weights(points, params[nn:], beta)
    soft = soft_points(points, an, bad, all_bad)
    proj = cg.project(p3d).reshape(C, F, J, 2)
    dproj = np.empty((C, F, J, 2, 3))
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        dproj[..., k] = ((cg.project(p3d + d) - cg.project(p3d - d)) / (2 * h)).reshape(C, F, J, 2)
    with np.errstate(invalid='ignore'):
        _, dr = _loss(soft - proj, reproj_error_threshold, reproj_loss)
    jx = -dr[..., None] * dproj
    cand = np.where(bad[..., None], 0.0, points)
    ja = np.zeros((C, F, J, 3, P))
    for comp in range(2):
        ja[:, :, :, comp] = dr[..., comp, None] * beta * an * (cand[..., comp] - soft[..., comp, None])
    mean = an.mean(axis=3, keepdims=True)
    sd = np.std(an, axis=3)
    T = np.sum((an - mean) * an, axis=3, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        ja[:, :, :, 2] = -10 * beta * an * ((an - mean) - T) / (P * sd[..., None])
    kink = an.max(axis=3) == an.min(axis=3)
    for k in range(P):
        dv = beta * an[..., k, None] * ((np.arange(P) == k) - an)
        ja[:, :, :, 2, k] = np.where(kink, -10 * np.std(dv, axis=3), ja[:, :, :, 2, k])
    ja[np.repeat(all_bad[..., None], 3, axis=3)] = 0
    X = p3d.reshape(F, J, 3)
    L = np.asarray(params[ix.c_len:ix.c_alpha])
    dX = np.empty((len(ix.cons), F, 3))
    dL = np.empty((len(ix.cons), F))
    for l, (a, b) in enumerate(ix.cons):
        s = scale_length if l < ix.nS else scale_length_weak
        dv = X[:, a] - X[:, b]
        nr = np.linalg.norm(dv, axis=1)
        dX[l] = (s * 100 / L[l] / nr)[:, None] * dv
        dL[l] = -s * 100 * nr / L[l] ** 2
    r, c, d = _entries(ix, dict(jx=jx, ja=ja, ssf=scale_smooth, dX=dX, dL=dL))
    return coo_matrix((d, (r, c)), shape=(ix.m, ix.nv)).tocsr()


def alphas_out(points, params, constraints, constraints_weak, beta=BETA):
    """alphas_norm as optim_points_possible returns it (:1493-1506): NaN at NaN candidates."""
    an, bad, _ = soft_weights(points, params[n_norm(points, constraints, constraints_weak):], beta)
    an[bad] = np.nan
    return an


def optim_points_possible(cg, points, p3ds, constraints=(), constraints_weak=(), scale_smooth=4, scale_length=2,
                          scale_length_weak=0.5, reproj_error_threshold=15, reproj_loss='soft_l1', n_deriv_smooth=1,
                          jac='2-point'):
    """The reference's call (:1473-1488).  jac: '2-point' (the reference), '3-point', or 'analytic'.
    Returns scipy's result, x0 and scale_smooth_full."""
    constraints = np.asarray(constraints, dtype=int).reshape(-1, 2)
    constraints_weak = np.asarray(constraints_weak, dtype=int).reshape(-1, 2)
    x0, ssf = init_params(p3ds, points, constraints, constraints_weak, scale_smooth)
    args = (cg, points, constraints, constraints_weak, ssf, scale_length, scale_length_weak, reproj_error_threshold,
            reproj_loss, n_deriv_smooth)
    if jac == 'analytic':
        res = optimize.least_squares(error_fun, x0=x0, jac=jac_analytic, loss='linear', ftol=1e-3, args=args)
    else:
        sp = jac_sparsity(points, constraints, constraints_weak, n_deriv_smooth)
        res = optimize.least_squares(error_fun, x0=x0, jac=jac, jac_sparsity=sp, loss='linear', ftol=1e-3, args=args)
    return res, x0, ssf
