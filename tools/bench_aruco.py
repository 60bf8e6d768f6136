"""ArUco-marker detection (csrc/aruco.hip, mqhip/aruco.py) at the cameras' 2048 x 1536 on one MI355X: the stages and
the whole ``mq_find_markers`` call on ``--batch`` BGR frames resident on the device, detected at 640 x 480 as the
reference does, beside a plain device copy of the same frames, alternating twice after a warm-up (HIP events).  The
frames are two rendered views (tests/aruco_ref.py, rendered at 1024 x 768 and doubled) and a frame without a marker,
repeated over the batch.  One JSON object on stdout, also written to profiles/aruco_bench.json.

Expected before the first run: the resize reads every byte of the frame and is the only
memory-bound stage (9.4 MB in, 0.9 MB out per frame); everything after it works on 0.3 M pixels per frame and is
bound by launch and dependency latency: the gray and threshold kernels are a few microseconds of work, the labelling
is three launches whose merge chases parent chains through atomics, the components are a memset and four launches of
which two are one workgroup per image with serial scans, and the quads are one wave per candidate.

python tools/bench_aruco.py [--batch 8] [--reps 20] [--out profiles/aruco_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "macaque-3d-pose-estimation_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

H, W, DW, DH, Q, M = 1536, 2048, 640, 480, 64, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aruco_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import aruco_ref as ar
    from mqhip import _lib, aruco

    assert torch.cuda.is_available(), "bench_aruco needs a HIP device"
    B = a.batch
    d = ar.make_dictionary()
    views, truth, want = [], [], []
    for seed, (rx, ry, rz, pos, k) in enumerate(((10, -15, 20, (0.4, -0.3, 2.2), 3), (30, 20, -35, (-1.0, 0.5, 3.0), 9))):
        R, t = ar.marker_pose(rx, ry, rz, pos)
        g, c, _ = ar.render_scene(W // 2, H // 2, 800.0, [(R, t, 1.0, ar.marker_cells(int(d[k])))], 0.0, 2, 40 + seed)
        views.append(np.repeat(np.repeat(g, 2, axis=0), 2, axis=1))
        truth.append(c[0] * 2.0 + 0.5)              # a pixel of the small image covers two of the doubled one
        want.append(k)
    views.append(np.repeat(np.repeat(ar.render_scene(W // 2, H // 2, 800.0, [], 0.0, 1, 42)[0], 2, axis=0), 2, axis=1))
    gray = np.stack([views[i % 3] for i in range(B)])
    frames = torch.from_numpy(np.repeat(gray[..., None], 3, axis=3)).cuda()
    count, ids, corners, info = aruco.find_markers(frames, d, det_size=(DW, DH), return_info=True)
    assert count.tolist() == [int(i % 3 != 2) for i in range(B)], count
    assert all(ids[i, 0] == want[i % 3] for i in range(B) if i % 3 != 2), ids
    err = max(float(np.linalg.norm(corners[i, 0] - truth[i % 3], axis=1).max()) for i in range(B) if i % 3 != 2)

    ctx = _lib.Context.get(0)
    lib, hnd, st = ctx.lib, ctx.handle, _lib.stream_ptr(0)
    i32, u8, dev = torch.int32, torch.uint8, frames.device
    small = torch.zeros((B, DH, DW, 3), dtype=u8, device=dev)
    g_d = torch.zeros((B, DH, DW), dtype=u8, device=dev)
    dark = torch.zeros((B, DH, DW), dtype=u8, device=dev)
    lab = torch.zeros((B, DH, DW), dtype=i32, device=dev)
    cnt = torch.zeros((B,), dtype=i32, device=dev)
    cand = torch.zeros((B, Q, 16), dtype=i32, device=dev)
    ok_d = torch.zeros((B, Q), dtype=i32, device=dev)
    id_d = torch.zeros((B, Q), dtype=i32, device=dev)
    rot = torch.zeros((B, Q), dtype=i32, device=dev)
    qc = torch.zeros((B, Q, 4, 2), dtype=torch.float64, device=dev)
    n_out = torch.zeros((B,), dtype=i32, device=dev)
    id_out = torch.zeros((B, M), dtype=i32, device=dev)
    c_out = torch.zeros((B, M, 4, 2), dtype=torch.float64, device=dev)
    dic = torch.from_numpy(d.astype(np.uint16).view(np.int16).copy()).to(dev)
    dst = torch.empty_like(frames)
    P = _lib.ptr
    fs = int(frames.stride(0))

    def ok(rc):
        _lib.check(rc, "bench_aruco")

    stages = {
        "resize": lambda: ok(lib.mq_resize_bilinear(hnd, P(frames), fs, B, H, W, P(small), DH * DW * 3, DH, DW, st)),
        "gray": lambda: ok(lib.mq_cmc_preprocess(hnd, P(small), DH * DW * 3, B, DH, DW, 1.0, P(g_d), st)),
        "threshold": lambda: ok(lib.mq_aruco_threshold(hnd, P(g_d), B, DH, DW, P(dark), st)),
        "label": lambda: ok(lib.mq_aruco_label(hnd, P(dark), B, DH, DW, P(lab), st)),
        "components": lambda: ok(lib.mq_aruco_components(hnd, P(lab), B, DH, DW, Q, P(cnt), P(cand), st)),
        "quads": lambda: ok(lib.mq_aruco_quads(hnd, P(g_d), B, DH, DW, P(cnt), P(cand), Q, P(dic), len(d), 0, 0, P(ok_d),
                                               P(id_d), P(rot), P(qc), st)),
        "find_markers": lambda: ok(lib.mq_find_markers(hnd, P(frames), fs, B, H, W, DW, DH, P(dic), len(d), 0, 0, Q, M,
                                                       P(n_out), P(id_out), P(c_out), None, st)),
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
    torch.cuda.synchronize()
    assert n_out.cpu().tolist() == count.tolist() and int(ok_d.sum()) == int(count.sum())
    times = {k: [] for k in stages}
    for _ in range(2):              # alternate, twice, so a clock drift shows as a spread rather than as a ratio
        for k, fn in stages.items():
            times[k].append(timed(fn))
    best = {k: min(v) for k, v in times.items()}
    res = {"tool": "bench_aruco", "height": H, "width": W, "det_size": [DW, DH], "batch": B, "reps": a.reps,
           "max_quads": Q, "count": count.tolist(), "candidates": info["candidates"].tolist(),
           "max_error_px_against_the_truth": err, "ms_per_frame": times,
           "find_over_copy": best["find_markers"] / best["device_copy"],
           "sum_of_stages_ms_per_frame": sum(best[k] for k in ("resize", "gray", "threshold", "label", "components",
                                                              "quads")),
           "frame_bytes": H * W * 3}
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
