"""Pose overlay (csrc/overlay.hip, src/pipeline/visualize_result.py) on one camera of a ``synth.write_clip`` clip
at 2048 x 1536 with 4 animals, on one MI355X.  Two measurements, each beside its yardstick, one JSON object on
stdout:

* kernel: ``OverlayRenderer.render`` of ``--batch`` images from a device-resident pool (HIP events; the time is
  both kernels plus the small uploads of the poses) beside a plain device copy of the same images
  (``torch.Tensor.copy_``) in the same process.  Either way one image is read once and written once: 18.9 MB.
  The ``overlay_draw_kernel`` time itself comes from a run of its own under the profiler:
  ``rocprofv3 --kernel-trace --stats -- python tools/bench_overlay.py --kernel-only``.
* stage: ``visualize_result.proc`` (read the store, upload, render, download, write the overlay store) beside the
  same ``proc`` with the NumPy oracle (tests/overlay_ref.py) injected as the renderer, on the same frames --
  the only available yardstick, not the reference's cv2 time.

python tools/bench_overlay.py [--frames 48] [--batch 16] [--reps 20] [--kernel-only] [--no-oracle]
"""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "macaque-3d-pose-estimation_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

H, W, N_ANIMALS = 1536, 2048, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true", help="the render / copy loops only (for the profiler)")
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch

    import overlay_ref
    from mqhip import io as mqio
    from mqhip import synth
    from mqhip.geometry import CameraGroup
    from mqhip.overlay import OverlayRenderer
    from src.pipeline import visualize_result as vis

    assert torch.cuda.is_available(), "bench_overlay needs a HIP device"
    F, B = a.frames, a.batch
    img_bytes = H * W * 3
    res = {"tool": "bench_overlay", "height": H, "width": W, "animals": N_ANIMALS, "frames": F, "batch": B,
           "bytes_per_image_read_plus_write": 2 * img_bytes}
    with tempfile.TemporaryDirectory() as tmp:
        cams, raw, results, cfg, _ = synth.write_clip(tmp, "clip", n_frames=F, n_views=1, n_animals=N_ANIMALS, pool=4)
        name = str(cams[0]["name"])
        rd = os.path.join(results, "clip")
        skel = synth.make_skeletons(N_ANIMALS, F + 1, seed=2)[:, :F]            # the clip's own poses (A, F, J, 3)
        score = np.ones(skel.shape[:3])
        mqio.dump_pickle({"kp3d": skel, "kp3d_score": score}, os.path.join(rd, "kp3d.pickle"))
        os.makedirs(os.path.join(rd, name))
        np.save(os.path.join(rd, name, "frame_num.npy"), np.arange(F, dtype=np.int32))

        # ---- kernel: render of B images from the resident pool vs a device copy of the same images
        store = mqio.FrameStore(os.path.join(raw, f"clip.{name}"))
        pool_d = torch.from_numpy(np.asarray(store.frames)).cuda()
        src = (np.arange(B) % len(pool_d)).astype(np.int32)
        kp = np.ascontiguousarray(skel[:, :B].transpose(1, 0, 2, 3))
        sc = np.ascontiguousarray(score[:, :B].transpose(1, 0, 2))
        r = OverlayRenderer(CameraGroup.from_dicts(cams), H, W)
        same = pool_d[torch.from_numpy(src).long().cuda()].contiguous()       # the B source images, gathered once
        dst = torch.empty_like(same)
        ev = lambda: torch.cuda.Event(enable_timing=True)

        def timed(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.reps / B          # ms per image

        out = r.render(pool_d, 0, kp, sc, src_index=src)
        drawn = int((out != same).any(dim=3).sum().item())
        # alternate the two, twice, so a clock drift shows as a spread rather than as a ratio
        t_render, t_copy = [], []
        for _ in range(2):
            t_render.append(timed(lambda: r.render(pool_d, 0, kp, sc, src_index=src)))
            t_copy.append(timed(lambda: dst.copy_(same)))
        res["kernel"] = {
            "drawn_pixels_per_image": drawn / B,
            "render_ms_per_image": t_render, "copy_ms_per_image": t_copy,
            "render_GBps": [2 * img_bytes / (t * 1e6) for t in t_render],
            "copy_GBps": [2 * img_bytes / (t * 1e6) for t in t_copy],
            "render_over_copy": min(t_render) / min(t_copy),
            "note": "render = mq_overlay_render (both kernels + the pose uploads); draw kernel alone: rocprofv3"}
        if a.kernel_only:
            print(json.dumps(res))
            return

        # ---- stage: visualize_result.proc on the GPU vs the same proc on the NumPy oracle
        kw = dict(results_dir_root=results, batch=B)
        quiet = contextlib.redirect_stdout(sys.stderr)       # proc's progress lines: stdout is the JSON line's
        with quiet:
            vis.proc("clip", 0, cfg, raw, out_dir=os.path.join(tmp, "warm"), frame_range=(0, B), **kw)
            t0 = time.perf_counter()
            path = vis.proc("clip", 0, cfg, raw, out_dir=os.path.join(tmp, "out_gpu"), **kw)
            t_gpu = time.perf_counter() - t0
        res["stage"] = {"gpu_s": t_gpu, "gpu_ms_per_frame": 1e3 * t_gpu / F}
        if not a.no_oracle:
            factory = overlay_ref.oracle_renderer_factory(os.path.join(rd, "calibration.toml"))
            with quiet:
                t0 = time.perf_counter()
                path_o = vis.proc("clip", 0, cfg, raw, out_dir=os.path.join(tmp, "out_ref"), renderer=factory, **kw)
                t_ref = time.perf_counter() - t0
            same_bytes = bool(np.array_equal(np.asarray(mqio.FrameStore(path).frames),
                                             np.asarray(mqio.FrameStore(path_o).frames)))
            res["stage"].update(oracle_s=t_ref, oracle_ms_per_frame=1e3 * t_ref / F, oracle_over_gpu=t_ref / t_gpu,
                                stores_identical=same_bytes)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
