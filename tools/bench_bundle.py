"""Rig bundle adjustment (csrc/bundle.hip, src/utils/multicam_toolbox.py) on a synthetic marker trace, on one
MI355X, beside scipy with the reference's least_squares call (tests/ba_ref.py) on the same machine's CPU.  One
JSON object on stdout.

* mode 0: ``optimize_extrinsic`` on ``--frames`` (5000) frames x ``--cams`` (8) cameras -- the whole call
  (frame mask, undistortion, triangulation, uploads, solve) and the solve alone -- beside scipy fed the same
  undistorted points and the same triangulation.
* mode 1: ``optimize_all_camera_params`` with ``--sample`` (500) sampled frames beside scipy on the numpy
  vectorised omnidir projection.  That is the only CPU figure there is here: the reference's objective calls
  cv2.omnidir.projectPoints once per observation in a Python loop, and cv2 is absent, so the reference itself
  would be slower than the figure printed.

One run each after a warm-up of the GPU path (the first call loads the library and allocates the workspace).

python tools/bench_bundle.py [--frames 5000] [--cams 8] [--sample 500] [--no-scipy]
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
    ap.add_argument("--frames", type=int, default=5000)
    ap.add_argument("--cams", type=int, default=8)
    ap.add_argument("--sample", type=int, default=500)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    import random

    import numpy as np
    import torch

    import ba_ref
    from mqhip import synth
    from mqhip.bundle import bundle_adjust
    from src.utils import multicam_toolbox as mt

    assert torch.cuda.is_available(), "bench_bundle needs a HIP device"
    F, C = a.frames, a.cams
    rng = np.random.default_rng(0)
    cams = synth.make_cameras(C)
    X = rng.uniform(-1.0, 1.0, (F + 5, 3)) * np.array([600.0, 600.0, 300.0])
    trace = [synth.project_numpy(c, X) + rng.normal(0, 0.5, (F + 5, 2)) for c in cams]
    for c in range(C):
        trace[c][rng.uniform(size=F + 5) < 0.15] = -1.0
    start = [dict(c) for c in cams]
    for c in start[1:]:
        c["rvec"] = c["rvec"] + rng.normal(0, 0.01, 3)
        c["tvec"] = c["tvec"] + rng.normal(0, 10.0, 3)
    camparam = synth.camparam_from_cams(start)
    res = {"tool": "bench_bundle", "frames": F, "cams": C, "sample": a.sample,
           "cpu_threads": os.environ.get("OMP_NUM_THREADS")}

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t

    # ---- mode 0
    run0 = lambda: mt.optimize_extrinsic("unused", False, True, camparam=camparam, marker_trace=trace,
                                         return_info=True)
    run0()
    (out, info), t_call = clock(run0)
    n_frame, frame_use = mt.ba_frame_use(trace)
    und = mt.undistortPoints(None, [t[:n_frame] for t in trace], True, camparam)
    P3 = mt.triangulatePoints(None, und, frame_use, False, camparam)
    keep = np.argwhere(frame_use.sum(axis=1) >= 2).ravel()
    cam0 = ba_ref.cam_rows(start, 0)
    obs, use = np.stack(und)[:, keep], frame_use[keep]
    (_, _, info_s), t_solve = clock(lambda: bundle_adjust(cam0, P3[keep], obs, use, 0))
    m0 = {"points": int(keep.size), "observations": int(use.sum()), "gpu_call_s": t_call, "gpu_solve_s": t_solve,
          "gpu_cost": info["cost"], "gpu_steps": info["iterations"], "gpu_stop": info["stop"]}
    if not a.no_scipy:
        t = time.perf_counter()
        cam5, _, r5 = ba_ref.solve_scipy(0, cam0, P3[keep], obs, use)
        m0.update(scipy_s=time.perf_counter() - t, scipy_cost=float(r5.cost), scipy_nfev=int(r5.nfev),
                  cost_ratio=info["cost"] / float(r5.cost))
        cam_gpu = np.stack([np.concatenate([r, t_.ravel()]) for r, t_ in out])
        m0["gauge_distance_to_scipy"] = ba_ref.gauge_distance(cam_gpu, cam5)
    res["mode0"] = m0
    print(json.dumps(res), file=sys.stderr, flush=True)

    # ---- mode 1 on sampled frames
    run1 = lambda: mt.optimize_all_camera_params("unused", False, True, camparam=camparam, marker_trace=trace,
                                                 n_random_sample=a.sample, seed=1, return_info=True)
    run1()
    (_, info1), t_call1 = clock(run1)
    I = random.Random(1).sample(list(range(n_frame)), a.sample)
    sub = [t[:n_frame][I] for t in trace]
    use1 = np.stack([s[:, 0] >= 0.0 for s in sub], axis=1)
    und1 = mt.undistortPoints(None, sub, True, camparam)
    P31 = mt.triangulatePoints(None, und1, use1, False, camparam)
    keep1 = np.argwhere(use1.sum(axis=1) >= 2).ravel()
    cam16 = ba_ref.cam_rows(start, 1)
    obs1 = np.stack(sub)[:, keep1]
    m1 = {"points": int(keep1.size), "gpu_call_s": t_call1, "gpu_cost": info1["cost"],
          "gpu_steps": info1["iterations"], "gpu_stop": info1["stop"]}
    if not a.no_scipy:
        t = time.perf_counter()
        _, _, r3 = ba_ref.solve_scipy(1, cam16, P31[keep1], obs1, use1[keep1])
        m1.update(scipy_numpy_projection_s=time.perf_counter() - t, scipy_cost=float(r3.cost),
                  scipy_nfev=int(r3.nfev), cost_ratio=info1["cost"] / float(r3.cost))
    res["mode1"] = m1
    print(json.dumps(res))


if __name__ == "__main__":
    main()
