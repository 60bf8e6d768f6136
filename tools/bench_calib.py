"""``mqhip.calib.calibrate_views`` (csrc/calib.hip) on one MI355X: ``--cams`` (8) cameras x ``--views`` (200) views x
54 chessboard corners, the pinhole and the omnidir model, one call each (start + solve, all cameras in the call),
beside the scipy restatement (tests/calib_ref.py: least_squares, trf, x_scale='jac', sparse Jacobian, ftol = xtol =
gtol = 1e-8) of the same problems from the same starts on this machine's CPU.  scipy solves ``--scipy-cams`` (1) of
the cameras; its time for all of them is that figure times the camera count, stated as an extrapolation.

Wall clock around synchronised calls, one run each after one warm-up of the GPU path.  One JSON object on stdout
(and in ``--out``).

python tools/bench_calib.py [--cams 8] [--views 200] [--scipy-cams 1] [--no-scipy] [--out profiles/calib_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "macaque-3d-pose-estimation_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=8)
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--scipy-cams", type=int, default=1)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import calib_ref as cr
    from mqhip.calib import calibrate_views

    assert torch.cuda.is_available(), "bench_calib needs a HIP device"
    res = {"tool": "bench_calib", "cams": a.cams, "views": a.views, "corners": 54, "runs": 1,
           "cpu_threads": os.environ.get("OMP_NUM_THREADS")}
    for model, tag in ((cr.MODEL_PINHOLE, "pinhole"), (cr.MODEL_OMNIDIR, "omnidir")):
        scenes = [cr.make_scene(model, a.views, 1000 + c) for c in range(a.cams)]
        obj = [o for sc in scenes for o in sc["obj"]]
        img = [i for sc in scenes for i in sc["img"]]
        vpp = [a.views] * a.cams
        calibrate_views(model, obj, img, vpp, cr.IMAGE_SIZE)                          # warm-up
        torch.cuda.synchronize()
        t = time.perf_counter()
        k, poses, rms, infos = calibrate_views(model, obj, img, vpp, cr.IMAGE_SIZE)
        torch.cuda.synchronize()
        one = {"gpu_call_s": time.perf_counter() - t, "gpu_rms_px": [float(r) for r in rms],
               "gpu_steps": [i["iterations"] for i in infos], "gpu_stop": [i["stop"] for i in infos],
               "gpu_cost": [i["cost"] for i in infos]}
        if not a.no_scipy:
            ts, costs, nfev = [], [], []
            for c in range(min(a.scipy_cams, a.cams)):
                sc = scenes[c]
                t = time.perf_counter()
                k0, p0 = cr.init_numpy(model, sc["obj"], sc["img"])
                _, _, cost, r = cr.solve_scipy(model, k0, p0, sc["obj"], sc["img"], tol=cr.LOOSE, sparse=True)
                ts.append(time.perf_counter() - t)
                costs.append(cost)
                nfev.append(int(r.nfev))
            one.update(scipy_s_per_camera=ts, scipy_cost=costs, scipy_nfev=nfev,
                       scipy_s_all_cameras_extrapolated=float(np.mean(ts)) * a.cams,
                       cost_ratio=[one["gpu_cost"][c] / costs[c] for c in range(len(costs))])
        res[tag] = one
        print(json.dumps(res), file=sys.stderr, flush=True)
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
