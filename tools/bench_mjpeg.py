"""Motion-JPEG encoding of the overlay frames (csrc/jpeg.hip, mqhip/mjpeg.py, ``visualize_result.proc(video='avi')``)
on one camera of a ``synth.write_clip`` clip at 2048 x 1536 with 4 animals, on one MI355X.  One JSON object on stdout:

* encode: ``JpegEncoder.encode_device`` of ``--batch`` rendered overlay frames resident on the device, at restart
  intervals 4, 8, 16 and 32 (HIP events after a warm-up; the time is the four kernels of ``mq_jpeg_encode``), beside
  a plain device copy of the same frames (``torch.Tensor.copy_``) in the same process, alternating; the mean stream
  bytes per frame at ``--quality``; the algorithm's bytes per image (frame read, coefficients written and read,
  stream written twice and read once).  The per-kernel times come from a run of its own under the profiler:
  ``rocprofv3 --kernel-trace --stats -- python tools/bench_mjpeg.py --kernel-only``.
* stage: ``visualize_result.proc`` with ``video='avi'`` (read the store, upload, render, encode, download the
  streams, write the AVI) beside the frame-store path (``video=None``: download the frames, write ``frames.npy``),
  alternating, on the same frames.

python tools/bench_mjpeg.py [--frames 48] [--batch 16] [--reps 20] [--quality 90] [--kernel-only]
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
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--kernel-only", action="store_true", help="the RI 16 encode / copy loops only (for the profiler)")
    a = ap.parse_args()
    import numpy as np
    import torch

    from mqhip import io as mqio
    from mqhip import synth
    from mqhip.geometry import CameraGroup
    from mqhip.mjpeg import JpegEncoder
    from mqhip.overlay import OverlayRenderer
    from src.pipeline import visualize_result as vis

    assert torch.cuda.is_available(), "bench_mjpeg needs a HIP device"
    F, B = a.frames, a.batch
    img_bytes = H * W * 3
    n_mcu = (H // 16) * (W // 16)
    res = {"tool": "bench_mjpeg", "height": H, "width": W, "animals": N_ANIMALS, "frames": F, "batch": B,
           "quality": a.quality, "image_bytes": img_bytes, "coefficient_bytes": n_mcu * 768}
    with tempfile.TemporaryDirectory() as tmp:
        cams, raw, results, cfg, _ = synth.write_clip(tmp, "clip", n_frames=F, n_views=1, n_animals=N_ANIMALS, pool=4)
        name = str(cams[0]["name"])
        rd = os.path.join(results, "clip")
        skel = synth.make_skeletons(N_ANIMALS, F + 1, seed=2)[:, :F]            # the clip's own poses (A, F, J, 3)
        score = np.ones(skel.shape[:3])
        mqio.dump_pickle({"kp3d": skel, "kp3d_score": score}, os.path.join(rd, "kp3d.pickle"))
        os.makedirs(os.path.join(rd, name))
        np.save(os.path.join(rd, name, "frame_num.npy"), np.arange(F, dtype=np.int32))

        # ---- encode: B rendered frames on the device, per restart interval, beside a device copy of them
        store = mqio.FrameStore(os.path.join(raw, f"clip.{name}"))
        pool_d = torch.from_numpy(np.asarray(store.frames)).cuda()
        src = (np.arange(B) % len(pool_d)).astype(np.int32)
        kp = np.ascontiguousarray(skel[:, :B].transpose(1, 0, 2, 3))
        sc = np.ascontiguousarray(score[:, :B].transpose(1, 0, 2))
        frames = OverlayRenderer(CameraGroup.from_dicts(cams), H, W).render(pool_d, 0, kp, sc, src_index=src)
        dst = torch.empty_like(frames)
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

        res["encode"] = {}
        for ri in ((16,) if a.kernel_only else (4, 8, 16, 32)):
            enc = JpegEncoder(H, W, quality=a.quality, restart_interval=ri)
            out = torch.empty((B, enc.max_bytes), dtype=torch.uint8, device="cuda")
            sizes = torch.zeros((B,), dtype=torch.int32, device="cuda")
            enc.encode_into(frames, out, sizes)
            mean_bytes = float(sizes.float().mean().item())
            # alternate the two, twice, so a clock drift shows as a spread rather than as a ratio
            t_enc, t_copy = [], []
            for _ in range(2):
                t_enc.append(timed(lambda: enc.encode_into(frames, out, sizes)))
                t_copy.append(timed(lambda: dst.copy_(frames)))
            moved = img_bytes + 2 * n_mcu * 768 + 3 * mean_bytes
            res["encode"][f"ri{ri}"] = {
                "stream_bytes_per_frame": mean_bytes, "slot_bytes_per_frame": enc.max_bytes,
                "encode_ms_per_image": t_enc, "copy_ms_per_image": t_copy,
                "encode_over_copy": min(t_enc) / min(t_copy),
                "algorithm_bytes_per_image": moved, "algorithm_GBps": moved / (min(t_enc) * 1e6)}
            del out
        if a.kernel_only:
            print(json.dumps(res))
            return

        # ---- stage: visualize_result.proc to an AVI vs to a frame store, alternating
        kw = dict(results_dir_root=results, batch=B)
        quiet = contextlib.redirect_stdout(sys.stderr)       # proc's progress lines: stdout is the JSON line's
        t_avi, t_store = [], []
        with quiet:
            vis.proc("clip", 0, cfg, raw, out_dir=os.path.join(tmp, "warm_a"), frame_range=(0, B), video="avi",
                     quality=a.quality, **kw)
            vis.proc("clip", 0, cfg, raw, out_dir=os.path.join(tmp, "warm_s"), frame_range=(0, B), **kw)
            for k in range(2):
                t0 = time.perf_counter()
                avi = vis.proc("clip", 0, cfg, raw, out_dir=os.path.join(tmp, f"avi{k}"), video="avi",
                               quality=a.quality, **kw)
                t_avi.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                vis.proc("clip", 0, cfg, raw, out_dir=os.path.join(tmp, f"store{k}"), **kw)
                t_store.append(time.perf_counter() - t0)
        r = mqio.MjpegAviReader(avi)
        res["stage"] = {"avi_ms_per_frame": [1e3 * t / F for t in t_avi],
                        "frame_store_ms_per_frame": [1e3 * t / F for t in t_store],
                        "avi_over_frame_store": min(t_avi) / min(t_store), "avi_frames": len(r),
                        "avi_file_bytes": os.path.getsize(avi), "frame_store_bytes": F * img_bytes}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
