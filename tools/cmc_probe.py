"""Times one batched camera-motion-compensation call (mqhip.cmc.SiftCmc.apply_batch) for 8 views of 2048 x 1536
with HIP events, warm-up excluded, and prints one JSON line.  Needs an MI355X; no CPU fallback.

    python tools/cmc_probe.py [--views 8] [--steps 20] [--warmup 3] [--ref]

``--ref`` also times the numpy restatement (tests/cmc_ref.py) on the CPU for the same frames."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "macaque-3d-pose-estimation_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import cmc_ref as R
    from mqhip.cmc import SiftCmc
    if not torch.cuda.is_available():
        raise SystemExit("cmc_probe: needs a HIP device")
    H, W = 1536, 2048
    # two time steps of `views` cameras: each camera its own blob field, panned between the steps
    fields = [R.blob_field(seed=7 + v) for v in range(a.views)]
    pan = np.array([[1, 0, -90.0], [0, 1, 40.0]])
    f0 = np.stack([R.render_blobs(b, H, W) for b in fields])
    f1 = np.stack([R.render_blobs(b, H, W, warp=pan) for b in fields])
    d0, d1 = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda()
    dets = [np.array([[800.0, 500, 1100, 900], [300, 200, 500, 600]])] * a.views
    c = SiftCmc(H, W, n_slots=a.views)
    for _ in range(a.warmup):
        c.apply_batch(d0, dets)
        w = c.apply_batch(d1, dets)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
    for k, (e0, e1) in enumerate(ev):
        e0.record()
        w = c.apply_batch(d1 if k % 2 == 0 else d0, dets)
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    out = dict(tool="cmc_probe", views=a.views, height=H, width=W, steps=a.steps, warmup=a.warmup,
               ms_per_step_median=ms[len(ms) // 2], ms_per_step_min=ms[0], ms_per_step_max=ms[-1],
               stats=c.stats[0], translation_last=[float(w[0, 0, 2]), float(w[0, 1, 2])])
    if a.ref:
        refs = [R.SiftCmcRef() for _ in range(a.views)]
        for r, f in zip(refs, f0):
            r.apply(f, dets[0])
        t = time.perf_counter()
        for r, f in zip(refs, f1):
            r.apply(f, dets[0])
        out["numpy_restatement_cpu_ms_per_step"] = (time.perf_counter() - t) * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
