"""The scalar core of the trf solver as headers -- csrc/lsmr_dev.hpp (sym_ortho, lsmr's start, recurrences and
stop test) and csrc/trf_host.hpp (the trust-region loop's per-problem state, the 2-D subproblem) -- compiled for the
host and run on small dense problems by tests/trf_core_check.cpp, against oracle/trf.py.  No GPU, no libmq_hip.so."""
import os
import shutil
import subprocess

import numpy as np

from oracle import trf as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "macaque-3d-pose-estimation_amd", "csrc")

# x agrees to 16 times the largest relative difference measured on the CPU (test's docstring), never looser than this
X_RTOL_CAP = 1e-9


def _lsmr_cases():
    rng = np.random.default_rng(5)
    A = rng.standard_normal((7, 4))
    b = rng.standard_normal(7)
    E = rng.standard_normal((5, 5))
    E[:, 3] = E[:, 1]
    e = rng.standard_normal(5)
    U, V = (np.linalg.qr(rng.standard_normal((5, 5)))[0] for _ in range(2))
    G = U @ np.diag([1.0, 0.7, 0.4, 1e-3, 1e-4]) @ V.T
    # name, A, b, damp, maxiter, atol = btol, conlim, the (istop, itn) both must report
    return [("7x4", A, b, 0.0, 4, 1e-6, 1e8, (2, 4)),
            ("7x4 damped", A, b, 0.3, 4, 1e-6, 1e8, (2, 4)),
            # two equal columns: the Krylov space never meets the null space, so the oracle (as scipy) converges
            # with istop 2, not on the condition number ...
            ("5x5 equal columns", E, e, 0.0, 5, 1e-6, 1e8, (2, 4)),
            # ... so the condition-number stop (istop 3) has a case of its own: singular values down to 1e-4, conlim 100
            ("5x5 graded, conlim 100", G, e, 0.0, 5, 1e-6, 1e2, (3, 4)),
            ("b = 0", A, np.zeros(7), 0.0, 4, 1e-6, 1e8, (8, 0)),
            ("maxiter 2", A, b, 0.0, 2, 1e-6, 1e8, (7, 2))]


_T = np.linspace(0.0, 2.5, 6)
_Y = 2.0 * np.exp(-1.3 * _T) + 0.5 + 0.01 * np.array([1.0, -2.0, 1.5, -0.5, 2.0, -1.0])


def _trf_cases():
    def efun(x):
        return x[0] * np.exp(x[1] * _T) + x[2] - _Y

    def ejac(x, f):
        return np.stack([np.exp(x[1] * _T), x[0] * _T * np.exp(x[1] * _T), np.ones_like(_T)], 1)

    def rfun(x):
        return np.array([10 * (x[1] - x[0] ** 2), 1 - x[0]])

    def rjac(x, f):
        return np.array([[-20 * x[0], 10.0], [-1.0, 0.0]])

    # kind, data, x0, ftol, fun, jac
    return [(0, np.concatenate([_T, _Y]), np.array([1.0, -0.5, 0.0]), 1e-8, efun, ejac),
            (1, np.zeros(0), np.array([-3.0, 4.0]), 1e-8, rfun, rjac)]


def _fmt(v):
    return " ".join(repr(float(e)) for e in np.ravel(v))


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def test_shared_trf_core_on_the_host(tmp_path):
    """lsmr_start / lsmr_recurrence / lsmr_istop in the kernels' phase order, and mq::TrfAnimal driving a dense
    trf_no_bounds loop, against oracle.trf on the same problems, under -fsanitize=address,undefined.

    istop, itn, status, nfev and njev are equal.  x (and the final cost) are not expected bit for bit: numpy's norm
    and @ do not add in index order.  Largest relative differences measured on the CPU: lsmr x 5.9e-16 (7x4 4.5e-16,
    damped 5.8e-16, equal columns 5.9e-16, maxiter 2 1.3e-16, b = 0 exact); trf x 2.2e-16 and cost 1.1e-14 on the
    exponential fit, both exact on the Rosenbrock pair.  The bounds are 16 times the largest: 9.5e-15 for x, 1.8e-13
    for the cost.  The graded matrix of the condition-number stop has singular values down to 1e-4, which its x
    shows: 1.1e-11 measured, held to 16 times that, 1.8e-10.
    The oracle's counts on both trf problems are the same from starts moved by +-1e-12 relative (checked here), so
    their equality with the core's does not hang on a rounding."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the core check needs a host C++ compiler"
    exe = str(tmp_path / "trf_core_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "trf_core_check.cpp"), "-o", exe],
                   check=True)
    lsmr, trf, lines = _lsmr_cases(), _trf_cases(), []
    for _, A, b, damp, maxiter, tol, conlim, _ in lsmr:
        lines.append(f"lsmr {A.shape[0]} {A.shape[1]} {damp!r} {maxiter} {tol!r} {conlim!r} {_fmt(A)} {_fmt(b)}")
    for kind, data, x0, ftol, _, _ in trf:
        lines.append(f"trf {kind} {ftol!r} 0 {len(data)} {_fmt(data)} {len(x0)} {_fmt(x0)}")
    fin, fout = tmp_path / "in.txt", tmp_path / "out.txt"
    fin.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "runtime error" not in out.stderr
    got = [ln.split() for ln in fout.read_text().splitlines()]
    assert len(got) == len(lsmr) + len(trf)

    x_rtol, cost_rtol = 16 * 5.9e-16, 16 * 1.1e-14
    assert max(x_rtol, cost_rtol) <= X_RTOL_CAP
    for (name, A, b, damp, maxiter, tol, conlim, (code, itn_want)), g in zip(lsmr, got):
        x, istop, itn = T.lsmr_phased(A.dot, A.T.dot, b, A.shape[1], damp=damp, atol=tol, btol=tol, conlim=conlim,
                                      maxiter=maxiter)
        gx = np.array(g[3:], float)
        rel = _rel(gx, x) if np.any(x) else float(np.abs(gx).max())
        print(f"lsmr {name}: oracle istop {istop} itn {itn}, core {g[1]} {g[2]}, x rel {rel:.3g}")
        assert g[0] == "lsmr" and int(g[2]) == itn
        if code == 8:  # the x = 0 exit: the core's code 8 is the oracle's (istop 0, itn 0)
            assert (int(g[1]), istop, itn) == (8, 0, 0) and rel == 0.0
        else:
            assert int(g[1]) == istop == code and itn == itn_want
            assert rel <= (16 * 1.1e-11 if code == 3 else x_rtol)
    for (kind, data, x0, ftol, fun, jac), g in zip(trf, got[len(lsmr):]):
        x, cost, nfev, njev, status = T.trf_no_bounds(fun, jac, x0, ftol=ftol)
        for s in (1 + 1e-12, 1 - 1e-12):
            assert T.trf_no_bounds(fun, jac, x0 * s, ftol=ftol)[2:] == (nfev, njev, status)
        gx, gcost = np.array(g[5:], float), float(g[4])
        rel, crel = _rel(gx, x), abs(gcost - cost) / max(cost, 1e-300) if cost else abs(gcost)
        print(f"trf {kind}: oracle status {status} nfev {nfev} njev {njev}, core {g[1:4]}, x rel {rel:.3g}, "
              f"cost rel {crel:.3g}")
        assert g[0] == "trf" and (int(g[1]), int(g[2]), int(g[3])) == (status, nfev, njev)
        assert rel <= x_rtol and crel <= cost_rtol
        if kind == 1:
            assert nfev > njev, "the Rosenbrock start must see a rejected trial step"
