"""Motion-JPEG decoding of frame stores (csrc/jpeg_dec.hip, mqhip/mjpeg.py ``JpegDecoder``, ``format: mjpeg`` stores of
mqhip/io.py) on one camera of a ``synth.write_clip`` clip at 2048 x 1536, on one MI355X.  One JSON object on stdout:

* decode: ``JpegDecoder.decode_into`` of ``--batch`` streams resident on the device (encoded by ``JpegEncoder`` at
  ``--quality``, restart interval 16; HIP events after a warm-up; the time is the memset and the four kernels of
  ``mq_jpeg_decode``), beside a plain device copy of the frames it writes and ``mq_jpeg_encode`` of the same frames,
  alternating in one process; the algorithm's bytes per image.  The per-kernel times come from a run of its own under
  the profiler: ``rocprofv3 --kernel-trace --stats -- python tools/bench_mjpeg_decode.py --kernel-only``.
* ri0: one frame without restart markers (written by Pillow): the one-lane path.
* stage: ``visualize_result.proc(video='avi')`` from the ``mjpeg`` store beside the same call from the ``npy`` store
  of the same clip, alternating twice after a warm-up of each.

python tools/bench_mjpeg_decode.py [--frames 48] [--batch 16] [--reps 20] [--quality 90] [--pool N] [--kernel-only]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "macaque-3d-pose-estimation_amd")):
    sys.path.insert(0, p)

H, W, N_ANIMALS, RI = 1536, 2048, 4, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--pool", type=int, default=0, help="distinct images in the store (default: one per frame)")
    ap.add_argument("--kernel-only", action="store_true", help="the decode / copy / encode loops only (for the profiler)")
    a = ap.parse_args()
    import numpy as np
    import torch

    from mqhip import io as mqio
    from mqhip import synth
    from mqhip.mjpeg import JpegDecoder, JpegEncoder, parse_header
    from src.pipeline import visualize_result as vis

    assert torch.cuda.is_available(), "bench_mjpeg_decode needs a HIP device"
    F, B = a.frames, a.batch
    pool = a.pool or (B if a.kernel_only else F + 1)
    img_bytes = H * W * 3
    n_mcu = (H // 16) * (W // 16)
    res = {"tool": "bench_mjpeg_decode", "height": H, "width": W, "frames": F, "batch": B, "pool": pool,
           "quality": a.quality, "restart_interval": RI, "image_bytes": img_bytes, "coefficient_bytes": n_mcu * 768,
           "plane_bytes": H * W * 3 // 2}
    with tempfile.TemporaryDirectory() as tmp:
        cams, raw, results, cfg, _ = synth.write_clip(tmp, "clip", n_frames=F, n_views=1, n_animals=N_ANIMALS,
                                                      pool=pool)
        name = str(cams[0]["name"])
        src_dir = os.path.join(raw, f"clip.{name}")
        store = mqio.FrameStore(src_dir)
        frames = torch.from_numpy(np.array(store.frames[:B])).cuda()
        if len(frames) < B:
            frames = frames[torch.arange(B) % len(frames)]

        # ---- decode: B streams on the device, beside a device copy of the frames and their encode
        enc = JpegEncoder(H, W, quality=a.quality, restart_interval=RI)
        streams = torch.zeros((B, (enc.max_bytes + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
        sizes = torch.zeros((B,), dtype=torch.int32, device="cuda")
        enc.encode_into(frames, streams, sizes)
        mean_bytes = float(sizes.float().mean().item())
        info = parse_header(streams[0, :int(sizes[0])].cpu().numpy().tobytes())
        dec = JpegDecoder()
        out = torch.empty_like(frames)
        dst = torch.empty_like(frames)
        status = torch.zeros((B,), dtype=torch.int32, device="cuda")
        dec.decode_into(streams, sizes, info, out, status)
        assert status.cpu().tolist() == [0] * B
        err = (out.int() - frames.int()).abs().float().mean().item()
        ev = lambda: torch.cuda.Event(enable_timing=True)

        def timed(fn, reps=a.reps, per=B):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps / per          # ms per image

        t_dec, t_copy, t_enc = [], [], []
        for _ in range(2):      # alternate, twice, so a clock drift shows as a spread rather than as a ratio
            t_dec.append(timed(lambda: dec.decode_into(streams, sizes, info, out, status)))
            t_copy.append(timed(lambda: dst.copy_(out)))
            t_enc.append(timed(lambda: enc.encode_into(frames, streams, sizes)))
        # stream read twice (markers, entropy); coefficients zeroed, (sparsely) written, read; planes written, read;
        # frame written
        moved = 2 * mean_bytes + 2 * n_mcu * 768 + 2 * (H * W * 3 // 2) + img_bytes
        res["decode"] = {"stream_bytes_per_frame": mean_bytes, "mean_abs_error_of_the_round_trip": err,
                         "decode_ms_per_image": t_dec, "copy_ms_per_image": t_copy, "encode_ms_per_image": t_enc,
                         "decode_over_copy": min(t_dec) / min(t_copy), "decode_over_encode": min(t_dec) / min(t_enc),
                         "algorithm_bytes_per_image": moved, "algorithm_GBps": moved / (min(t_dec) * 1e6)}
        if a.kernel_only:
            print(json.dumps(res))
            return

        # ---- ri0: one frame without restart markers, one lane
        try:
            from PIL import Image
            b = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(frames[0].cpu().numpy()[..., ::-1])).save(
                b, "JPEG", quality=a.quality, subsampling=2)
            data = b.getvalue()
            i0 = parse_header(data)
            assert i0.restart_interval == 0
            s0 = torch.zeros((1, (len(data) + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
            s0[0, :len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            z0 = torch.tensor([len(data)], dtype=torch.int32, device="cuda")
            st0 = torch.zeros((1,), dtype=torch.int32, device="cuda")
            t0 = timed(lambda: dec.decode_into(s0, z0, i0, out[:1], st0), reps=2, per=1)
            assert st0.cpu().tolist() == [0]
            res["ri0"] = {"stream_bytes": len(data), "decode_ms_per_image": t0}
        except ImportError:
            res["ri0"] = "not measured: Pillow is not installed"

        # ---- stage: visualize_result.proc(video='avi') from the mjpeg store vs from the npy store, alternating
        rd = os.path.join(results, "clip")
        skel = synth.make_skeletons(N_ANIMALS, F + 1, seed=2)[:, :F]
        mqio.dump_pickle({"kp3d": skel, "kp3d_score": np.ones(skel.shape[:3])}, os.path.join(rd, "kp3d.pickle"))
        os.makedirs(os.path.join(rd, name))
        np.save(os.path.join(rd, name, "frame_num.npy"), np.arange(F, dtype=np.int32))
        raw_j = os.path.join(tmp, "videos_mjpeg")
        t0 = time.perf_counter()
        n_raw, n_jpg = mqio.convert_frame_store(src_dir, os.path.join(raw_j, f"clip.{name}"), quality=a.quality,
                                                restart_interval=RI, batch=B)
        t_conv = time.perf_counter() - t0
        kw = dict(results_dir_root=results, batch=B, video="avi", quality=a.quality)
        quiet = contextlib.redirect_stdout(sys.stderr)       # proc's progress lines: stdout is the JSON line's
        t_j, t_n = [], []
        with quiet:
            vis.proc("clip", 0, cfg, raw_j, out_dir=os.path.join(tmp, "warm_j"), frame_range=(0, B), **kw)
            vis.proc("clip", 0, cfg, raw, out_dir=os.path.join(tmp, "warm_n"), frame_range=(0, B), **kw)
            for k in range(2):
                t0 = time.perf_counter()
                vis.proc("clip", 0, cfg, raw_j, out_dir=os.path.join(tmp, f"j{k}"), **kw)
                t_j.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                vis.proc("clip", 0, cfg, raw, out_dir=os.path.join(tmp, f"n{k}"), **kw)
                t_n.append(time.perf_counter() - t0)
        res["stage"] = {"mjpeg_store_ms_per_frame": [1e3 * t / F for t in t_j],
                        "npy_store_ms_per_frame": [1e3 * t / F for t in t_n],
                        "mjpeg_over_npy": min(t_j) / min(t_n), "store_raw_bytes": n_raw, "store_jpeg_bytes": n_jpg,
                        "bytes_ratio": n_raw / n_jpg, "convert_s": t_conv}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
