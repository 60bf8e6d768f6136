"""Call time of optim_points_possible on synthetic decoy data: 4 animals, F = 300, J = 17, C = 8, P = 2 and P = 3
(mqhip.synth.make_candidates), by device events around the whole call, median of --reps after a warm-up.  Beside
it, in the same run: optim_points (trf) on slot 0 of the same data, and both solvers' lsmr iterations.  With
--scipy, scipy's wall time for animal 0 on the CPU (tests/possible_ref.py, the reference's arguments), for scale;
--no-gpu runs that part alone.  Writes profiles/optim_possible_bench.json (or --out); a case already in that file
keeps the fields this run does not measure, so a --no-gpu --scipy run adds scipy's figures to a GPU run's file.

python tools/bench_optim_possible.py [--reps 3] [--frames 300] [--animals 4] [--scipy] [--no-gpu] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "macaque-3d-pose-estimation_amd"), os.path.join(ROOT, "tests")]


def problem(A, F, P, cams):
    from mqhip import synth
    skel = synth.make_skeletons(A, F, seed=2)
    pts = np.stack([synth.make_candidates(cams, skel[a], P, seed=10 + a)[0] for a in range(A)])
    return skel, pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--animals", type=int, default=4)
    ap.add_argument("--possible", default="2,3")
    ap.add_argument("--scipy", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_possible_bench.json"))
    a = ap.parse_args()
    from mqhip import synth
    cams = synth.make_cameras(8)
    cons = synth.constraint_indices(synth.CONSTRAINTS)
    weak = synth.constraint_indices(synth.CONSTRAINTS_WEAK)
    out = {"animals": a.animals, "frames": a.frames, "joints": 17, "cameras": 8, "reps": a.reps, "cases": []}
    before = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if all(old.get(k) == out[k] for k in ("animals", "frames", "joints", "cameras")):
            before = {c["P"]: c for c in old["cases"]}
            out["reps"] = old["reps"] if a.no_gpu else a.reps
    for P in (int(v) for v in a.possible.split(",")):
        skel, pts = problem(a.animals, a.frames, P, cams)
        A, C, F, J = pts.shape[:4]
        case = {"P": P}
        if not a.no_gpu:
            import torch
            from mqhip import optim
            from mqhip.geometry import CameraGroup
            g = CameraGroup.from_dicts(cams)
            slot0 = np.ascontiguousarray(pts[:, :, :, :, 0])
            init = np.stack([g.triangulate(slot0[i].reshape(C, -1, 2)).reshape(F, J, 3) for i in range(A)])

            def timed(fn):
                ms, res = [], None
                for r in range(a.reps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    res = fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if r:
                        ms.append(e0.elapsed_time(e1))
                return ms, res

            ms, (p3, an, jl, st, _) = timed(lambda: optim.optim_points_possible_batch(
                g, pts, init, cons, weak, return_stats=True))
            ms0, (q3, ql, st0, _) = timed(lambda: optim.optim_points_batch(
                g, slot0, init, cons, weak, solver="trf", return_stats=True))
            dist = lambda x: np.linalg.norm(x - skel, axis=-1)  # noqa: E731
            case.update({
                "possible_ms": ms, "possible_ms_median": float(np.median(ms)),
                "possible_nfev": st[:, 4].astype(int).tolist(), "possible_njev": st[:, 5].astype(int).tolist(),
                "possible_status": st[:, 3].astype(int).tolist(), "possible_lsmr": st[:, 6].astype(int).tolist(),
                "possible_ms_per_lsmr_iteration": float(np.median(ms) / st[:, 6].max()),
                "slot0_ms": ms0, "slot0_ms_median": float(np.median(ms0)),
                "slot0_nfev": st0[:, 4].astype(int).tolist(), "slot0_lsmr": st0[:, 6].astype(int).tolist(),
                "slot0_ms_per_lsmr_iteration": float(np.median(ms0) / st0[:, 6].max()),
                "to_truth_median_mm": {"init": float(np.nanmedian(dist(init))), "possible": float(np.median(dist(p3))),
                                       "slot0": float(np.median(dist(q3)))}})
        if a.scipy:
            import possible_ref as pr
            from oracle.geometry import CameraGroupOracle
            cg = CameraGroupOracle(cams)
            init0 = cg.triangulate(pts[0, :, :, :, 0].reshape(C, -1, 2)).reshape(F, J, 3)
            t0 = time.perf_counter()
            res, _, _ = pr.optim_points_possible(cg, pts[0], init0, cons, weak)
            case.update({"scipy_one_animal_s": time.perf_counter() - t0, "scipy_nfev": int(res.nfev),
                         "scipy_njev": int(res.njev), "scipy_status": int(res.status),
                         "scipy_to_truth_median_mm": float(np.median(np.linalg.norm(
                             res.x[:F * J * 3].reshape(F, J, 3) - skel[0], axis=-1)))})
        print(json.dumps(case), flush=True)
        before[P] = {**before.get(P, {}), **case}
    out["cases"] = [before[P] for P in sorted(before)]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
