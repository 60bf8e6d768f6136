"""Turn a raw frame store (``format: npy``: ``frames.npy``, 9.4 MB per 2048 x 1536 frame) into a Motion-JPEG one
(``format: mjpeg``: ``frames.avi``, baseline JPEG frames encoded on the GPU), which ``mqhip.io.FrameStore`` decodes on
the GPU.  ``mqhip.io.convert_frame_store`` is the function; JPEG is lossy.

python tools/compress_store.py SRC DST [--quality 90] [--restart-interval 16] [--batch 16] [--device 0]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "macaque-3d-pose-estimation_amd")):
    sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("src", help="a store directory (holds metadata.yaml and frames.npy)")
    ap.add_argument("dst", help="the directory to write")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--restart-interval", type=int, default=16)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    from mqhip import io as mqio
    raw, packed = mqio.convert_frame_store(a.src, a.dst, quality=a.quality, restart_interval=a.restart_interval,
                                           batch=a.batch, device=a.device)
    print(json.dumps({"src": a.src, "dst": a.dst, "raw_bytes": raw, "jpeg_bytes": packed,
                      "ratio": round(raw / max(packed, 1), 2)}))


if __name__ == "__main__":
    main()
