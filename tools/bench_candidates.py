"""The three candidate entry points (csrc/imgproc.hip, csrc/candidates.hip) at the sizes DESIGN.md section 8.7 reports, each beside
its single-candidate counterpart on the same data, on one MI355X.  Call times are HIP events around the
library calls on device-resident inputs (one JSON object on stdout); kernel times come from a run of its own
under the profiler:  rocprofv3 --kernel-trace --stats -- python tools/bench_candidates.py --reps 3

* mq_decode_udp_topk at n = 64, J = 17, 64 x 48, K = 3 beside mq_decode_udp on the same heatmaps;
* mq_viterbi_filter_multi at config-4 size (544 chains x 300 frames), K = 3 beside mq_viterbi_filter on slot 0;
* mq_triangulate_possible at C = 8, P = 2, N = 20,400 beside mq_triangulate_ransac on the true slot.

python tools/bench_candidates.py [--reps 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "macaque-3d-pose-estimation_amd")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch

    from mqhip import _lib, synth
    from mqhip.geometry import CameraGroup

    assert torch.cuda.is_available(), "bench_candidates needs a HIP device"
    ctx = _lib.Context.get(0)
    lib, h = ctx.lib, ctx.handle
    dev = torch.device("cuda", 0)
    st = _lib.stream_ptr(dev)
    rng = np.random.default_rng(0)

    def timed(fn):
        fn()                                                     # warm-up: code objects, scratch
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    res = {"tool": "bench_candidates", "reps": a.reps}

    # ---- decode: 64 crops, three blobs per map
    n, J, hh, ww, K = 64, 17, 64, 48, 3
    yy, xx = np.mgrid[0:hh, 0:ww]
    hm = rng.normal(0, 0.02, (n, J, hh, ww)).astype(np.float32)
    for i in range(n):
        for k in range(J):
            for amp in (1.0, 0.7, 0.45):
                cx, cy = rng.uniform(0, ww), rng.uniform(0, hh)
                hm[i, k] += (amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 8.0)).astype(np.float32)
    hm_d = torch.from_numpy(hm).to(dev)
    center = torch.full((n, 2), 500.0, device=dev)
    scale = torch.full((n, 2), 200.0, device=dev)
    kp1 = torch.empty((n, J, 2), dtype=torch.float64, device=dev)
    sc1 = torch.empty((n, J), dtype=torch.float32, device=dev)
    am1 = torch.empty((n, J), dtype=torch.int32, device=dev)
    kpk = torch.empty((n, J, K, 2), dtype=torch.float64, device=dev)
    sck = torch.empty((n, J, K), dtype=torch.float32, device=dev)
    amk = torch.empty((n, J, K), dtype=torch.int32, device=dev)
    res["decode_udp_ms"] = timed(lambda: _lib.check(lib.mq_decode_udp(
        h, _lib.ptr(hm_d), n, J, hh, ww, _lib.ptr(center), _lib.ptr(scale), _lib.ptr(kp1), _lib.ptr(sc1),
        _lib.ptr(am1), None, st), "mq_decode_udp"))
    res["decode_udp_topk_ms"] = timed(lambda: _lib.check(lib.mq_decode_udp_topk(
        h, _lib.ptr(hm_d), n, J, hh, ww, _lib.ptr(center), _lib.ptr(scale), K, 3, 0.0, _lib.ptr(kpk), _lib.ptr(sck),
        _lib.ptr(amk), None, st), "mq_decode_udp_topk"))
    res["decode_slots_filled"] = float((amk >= 0).float().mean().item())

    # ---- Viterbi: config 4 (4 animals x 8 cameras x 17 joints, 300 frames), slot 0 + two decoys
    cams = synth.make_cameras(8)
    kp2d = synth.make_kp2d(cams, synth.make_skeletons(4, 300), drop=0.1, seed=3)      # (4, 300, 8, 17, 3)
    A, F, C, Jv, _ = kp2d.shape
    cand = np.zeros((A, F, C, Jv, 3, 3))
    cand[..., 0, :] = kp2d
    for k in (1, 2):
        cand[..., k, :2] = kp2d[..., :2] + rng.normal(0, 80, kp2d[..., :2].shape)
        cand[..., k, 2] = rng.uniform(0.2, 0.9, kp2d.shape[:4])
    one_d = torch.from_numpy(kp2d).to(dev)
    cand_d = torch.from_numpy(cand).to(dev)
    out_d = torch.empty((A, F, C, Jv, 3), dtype=torch.float64, device=dev)
    res["viterbi_filter_ms"] = timed(lambda: _lib.check(lib.mq_viterbi_filter(
        h, _lib.ptr(one_d), A, F, C, Jv, 0.3, 3, 25.0, _lib.ptr(out_d), st), "mq_viterbi_filter"))
    res["viterbi_filter_multi_ms"] = timed(lambda: _lib.check(lib.mq_viterbi_filter_multi(
        h, _lib.ptr(cand_d), A, F, C, Jv, 3, 0.3, 3, 25.0, _lib.ptr(out_d), st), "mq_viterbi_filter_multi"))
    res["viterbi_chains"], res["viterbi_frames"] = A * C * Jv, F

    # ---- triangulation: 20,400 points, the true projection in a random one of two slots
    g = CameraGroup.from_dicts(cams)
    X = synth.make_skeletons(4, 300).reshape(-1, 3)                                   # 20,400 points
    N, P = X.shape[0], 2
    uv = g.project(X)
    pts = uv[:, :, None, :] + rng.normal(0, 60, (8, N, P, 2))
    slot = rng.integers(0, P, (8, N))
    ci, ni = np.meshgrid(np.arange(8), np.arange(N), indexing="ij")
    true = uv + rng.normal(0, 0.2, uv.shape)
    pts[ci, ni, slot] = true
    pts[rng.uniform(0, 1, (8, N, P)) < 0.15] = np.nan
    true[np.isnan(pts[ci, ni, slot][..., 0])] = np.nan
    pts_d = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
    true_d = torch.from_numpy(np.ascontiguousarray(true)).to(dev)
    cams_d = g.cams_tensor()
    p3 = torch.empty((N, 3), dtype=torch.float64, device=dev)
    pk1 = torch.empty((8, N), dtype=torch.uint8, device=dev)
    pk2 = torch.empty((8, N, P), dtype=torch.uint8, device=dev)
    p2 = torch.empty((8, N, 2), dtype=torch.float64, device=dev)
    er = torch.empty((N,), dtype=torch.float64, device=dev)
    res["triangulate_ransac_ms"] = timed(lambda: _lib.check(lib.mq_triangulate_ransac(
        h, _lib.ptr(cams_d), 8, _lib.ptr(true_d), N, 2, 0.5, _lib.ptr(p3), _lib.ptr(pk1), _lib.ptr(p2),
        _lib.ptr(er), st), "mq_triangulate_ransac"))
    res["triangulate_possible_ms"] = timed(lambda: _lib.check(lib.mq_triangulate_possible(
        h, _lib.ptr(cams_d), 8, _lib.ptr(pts_d), N, P, 2, 0.5, _lib.ptr(p3), _lib.ptr(pk2), _lib.ptr(p2),
        _lib.ptr(er), st), "mq_triangulate_possible"))
    err = np.linalg.norm(p3.cpu().numpy() - X, axis=1)
    res["triangulate_points"] = N
    res["triangulate_possible_within_5mm"] = float(np.mean(err < 5.0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
