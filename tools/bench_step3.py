"""Step 3 (cross-frame matching) on the 300-frame x 8-view x 4-individual clip of BASELINE config 4:
``main_proc``'s wall time on one MI355X and, beside it, the wall time of the same host stages driven by
the oracle's per-cell Python lift (tests/step3_scenes.OracleLift) -- the only available yardstick, not the
reference's time.  The rows and keyframe records are a seeded ``step3_scenes`` scene with one broken
keyframe, one id switch, one unlabelled animal.  Writes one JSON object to stdout.

python tools/bench_step3.py [--reps 3] [--no-oracle]
(under rocprofv3 --kernel-trace --stats: --reps 1 --no-oracle)
"""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "macaque-3d-pose-estimation_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

RECIPE = {"seed": 2, "n_frame": 300, "n_cam": 8, "n_animal": 4, "p_seen": 0.95, "p_dup": 0.1,
          "events": [["kf_drop", 9, 1], ["switch", 2, 0, 140], ["noid", 3], ["dup", 1, 2, 40, 90]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import yaml

    import step3_scenes as scenes
    from mqhip import synth, tracklets
    from mqhip.association import StepTwoCameras
    from src.pipeline import step3_crossframematching as s3

    cams, T, keyframes = scenes.build_scene(RECIPE)
    camparam = synth.camparam_from_cams(cams)
    res = {"config": "BASELINE config 4 rows: 300 frames x 8 views x 4 individuals x 17 joints",
           "keyframes": len(keyframes), "rows": int(sum(len(r) for cam in T for r in cam))}
    with tempfile.TemporaryDirectory() as tmp:
        cfg = os.path.join(tmp, "config.yaml")
        with open(cfg, "w") as f:
            yaml.safe_dump({"camera_id": [int(c["name"]) for c in cams]}, f)
        for c, cam in enumerate(cams):
            os.makedirs(os.path.join(tmp, str(cam["name"])))
            with open(os.path.join(tmp, str(cam["name"]), "alldata.json"), "w") as f:
                json.dump(T[c], f)
        with open(os.path.join(tmp, "match_keyframe.pickle"), "wb") as f:
            pickle.dump(keyframes, f)
        stc = StepTwoCameras(camparam)
        ts = []
        for _ in range(args.reps + 1):      # the first run warms the context up
            t0 = time.perf_counter()
            Trk, Cid, _ = s3.main_proc(cfg, tmp, camparam=stc)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res["main_proc_wall_s"] = float(np.median(ts[1:]))
        res["main_proc_first_s"] = ts[0]
        res["tracklets"] = len(Trk)

    # the stages alone (no file I/O), on the kernels and on the oracle lift
    lifts = []

    def gpu_lift(rows):
        lifts.append(tracklets.TrackletLift(stc, rows))
        return lifts[-1]

    t0 = time.perf_counter()
    g = s3.run_stages([[[list(r) for r in fr] for fr in cam] for cam in T], keyframes, 8, gpu_lift)
    res["stages_gpu_lift_s"] = time.perf_counter() - t0
    res["launches"] = lifts[-1].launches
    if not args.no_oracle:
        oracle = []

        def cpu_lift(rows):
            oracle.append(scenes.OracleLift(camparam, rows))
            return oracle[-1]

        t0 = time.perf_counter()
        o = s3.run_stages([[[list(r) for r in fr] for fr in cam] for cam in T], keyframes, 8, cpu_lift)
        res["stages_oracle_lift_s"] = time.perf_counter() - t0
        res["oracle_cells_lifted"] = oracle[-1].cells_lifted
        res["same_result"] = bool(sorted(o[0]) == sorted(g[0]) and all(
            np.array_equal(o[0][k], g[0][k]) and np.array_equal(o[1][k], g[1][k]) for k in g[0]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
