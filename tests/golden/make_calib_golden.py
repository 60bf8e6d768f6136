"""Writes tests/golden/calib_scenes.npz: the seeded scenes of tests/calib_ref.py, their starts, and scipy's
solutions at a loose and a tight tolerance (calib_ref.LOOSE, TIGHT), so that no GPU test runs scipy.

    python tests/golden/make_calib_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import calib_ref as cr  # noqa: E402


def main():
    out = {}
    for name in cr.SCENES:
        sc = cr.scene(name)
        k0, p0, free = cr.scene_start(name, sc)
        put = lambda key, val: out.__setitem__(f"{name}/{key}", np.asarray(val))
        put("model", sc["model"])
        put("counts", [len(o) for o in sc["obj"]])
        put("obj", np.concatenate(sc["obj"]))
        put("img", np.concatenate(sc["img"]))
        put("k_true", sc["k_true"])
        put("poses_true", sc["poses_true"])
        put("k0", k0)
        put("poses0", p0)
        put("free", free)
        for tag, tol in (("loose", cr.LOOSE), ("tight", cr.TIGHT)):
            k, p, c, res = cr.solve_scipy(sc["model"], k0, p0, sc["obj"], sc["img"], free_mask=free, tol=tol)
            put(f"k_{tag}", k)
            put(f"poses_{tag}", p)
            put(f"cost_{tag}", c)
            put(f"nfev_{tag}", res.nfev)
            print(f"{name:12s} {tag}: cost {c:.12e} nfev {res.nfev} status {res.status}")
    sc = cr.make_chain_scene()
    out["chain/trace"] = np.stack(sc["trace"])            # the seeded inputs, so that a test can tell a drifted builder
    out["chain/cage"] = np.stack(sc["cage"])
    out["chain/board_img"] = np.stack([np.stack(b["img"]) for b in sc["boards"]])
    for tag, tol in (("loose", cr.LOOSE), ("tight", cr.TIGHT)):
        kp, ko, ext = cr.chain_scipy(sc, tol)
        out[f"chain/k_pinhole_{tag}"], out[f"chain/k_omnidir_{tag}"], out[f"chain/ext_{tag}"] = kp, ko, ext
        print(f"chain {tag}: xi {ko[:, 5]} |ext - true| {np.abs(ext - sc['ext_true']).max(axis=0)}")
    path = os.path.join(HERE, cr.GOLDEN)
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
