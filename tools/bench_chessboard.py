"""Chessboard-corner detection (csrc/chessboard.hip, mqhip/chessboard.py) at the cameras' 2048 x 1536 on one MI355X:
the stages and the whole ``mq_find_chessboard`` call on ``--batch`` BGR frames resident on the device, beside a plain
device copy of the same frames, alternating twice after a warm-up (HIP events).  The frames are two rendered views
(tests/chessboard_ref.py) and a frame without a board, repeated over the batch.  One JSON object on stdout, also written
to profiles/chessboard_bench.json.

python tools/bench_chessboard.py [--batch 8] [--reps 20] [--out profiles/chessboard_bench.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "macaque-3d-pose-estimation_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

H, W, K, WIN = 1536, 2048, 256, 11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chessboard_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import chessboard_ref as cr
    from mqhip import _lib, chessboard

    assert torch.cuda.is_available(), "bench_chessboard needs a HIP device"
    B = a.batch
    c = np.array([4.0, 2.5, 0.0])
    views, truth = [], []
    for seed, (rx, ry, rz, z) in enumerate(((10, -15, 20, 16.0), (30, 20, -35, 19.0))):
        R = cr.rot_xyz(math.radians(rx), math.radians(ry), math.radians(rz))
        g, uv = cr.render_view(W, H, 1650.0, R, np.array([0.3, -0.2, z]) - R @ c, -0.25, 2, 40 + seed)
        views.append(g)
        truth.append(cr.canonical_truth(uv))
    views.append(cr.make_empty(W, H, 42))
    gray = np.stack([views[i % 3] for i in range(B)])
    frames = torch.from_numpy(np.repeat(gray[..., None], 3, axis=3)).cuda()
    found, corners = chessboard.find_chessboard_corners(frames, win=WIN)
    assert found.tolist() == [i % 3 != 2 for i in range(B)], found
    err = max(float(np.linalg.norm(corners[i] - truth[i % 3], axis=1).max()) for i in range(B) if i % 3 != 2)

    ctx = _lib.Context.get(0)
    lib, hnd, st = ctx.lib, ctx.handle, _lib.stream_ptr(0)
    h, w, scale = H // 2, W // 2, 0.5
    i32, dev = torch.int32, frames.device
    full = torch.zeros((B, H, W), dtype=torch.uint8, device=dev)
    small = torch.zeros((B, h, w), dtype=torch.uint8, device=dev)
    resp = torch.zeros((B, h, w), dtype=i32, device=dev)
    pos = torch.zeros((B, K, 2), dtype=i32, device=dev)
    val = torch.zeros((B, K), dtype=i32, device=dev)
    cnt = torch.zeros((B,), dtype=i32, device=dev)
    fnd = torch.zeros((B,), dtype=i32, device=dev)
    cor = torch.zeros((B, 54, 2), dtype=torch.float64, device=dev)
    cor0 = torch.zeros_like(cor)
    dst = torch.empty_like(frames)
    P = _lib.ptr
    fs = int(frames.stride(0))

    def ok(rc):
        _lib.check(rc, "bench_chessboard")

    stages = {
        "gray_full": lambda: ok(lib.mq_cmc_preprocess(hnd, P(frames), fs, B, H, W, 1.0, P(full), st)),
        "gray_half": lambda: ok(lib.mq_cmc_preprocess(hnd, P(frames), fs, B, H, W, scale, P(small), st)),
        "response": lambda: ok(lib.mq_chess_response(hnd, P(small), B, h, w, P(resp), st)),
        "candidates": lambda: ok(lib.mq_chess_candidates(hnd, P(resp), B, h, w, K, P(pos), P(val), P(cnt), st)),
        "grid": lambda: ok(lib.mq_chess_grid(hnd, P(pos), P(val), P(cnt), B, K, scale, P(fnd), P(cor0), None, st)),
        "subpix": lambda: (cor.copy_(cor0), ok(lib.mq_corner_subpix(hnd, P(full), B, H, W, P(cor), 54, P(fnd), WIN, 30,
                                                                    1e-3, st))),
        "find_chessboard": lambda: ok(lib.mq_find_chessboard(hnd, P(frames), fs, B, H, W, scale, WIN, 30, 1e-3, K,
                                                             P(fnd), P(cor), st)),
        "device_copy": lambda: dst.copy_(frames),
    }

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps / B          # ms per frame

    for fn in stages.values():      # every stage once, in order, so each has its inputs
        fn()
    times = {k: [] for k in stages}
    for _ in range(2):              # alternate, twice, so a clock drift shows as a spread rather than as a ratio
        for k, fn in stages.items():
            times[k].append(timed(fn))
    best = {k: min(v) for k, v in times.items()}
    res = {"tool": "bench_chessboard", "height": H, "width": W, "batch": B, "reps": a.reps, "scale": scale, "win": WIN,
           "max_candidates": K, "found": found.tolist(), "max_error_px_against_the_truth": err,
           "ms_per_frame": times, "find_over_copy": best["find_chessboard"] / best["device_copy"],
           "sum_of_stages_ms_per_frame": sum(best[k] for k in ("gray_full", "gray_half", "response", "candidates", "grid",
                                                              "subpix")),
           "frame_bytes": H * W * 3}
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
