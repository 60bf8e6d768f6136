"""Step 3's tracking video on one MI355X, at the cameras' 2048 x 1536:

* ``mq_resize_bilinear`` to 800 x 600 beside a plain device copy of the same source bytes (1 and 16 images);
* the unlabelled ``mq_overlay_render`` of 4 frames with 4 animals, this build and -- with ``--base-lib`` -- another
  build of libmq_hip.so (the parent commit's) alternating in one process, and whether their outputs are equal;
* ``mq_overlay_render_labelled`` on the same frames with a colour table only, and with four 2-digit labels;
* ``step3.visualize`` on a small step-3 scene: ms per frame, the GPU calls (lift, render, resize, encode; each
  ended by a device synchronise) split from the host's share (reading the store, uploads, writing the AVI).

Times are device events around windows of 100-200 calls, several windows each.  ``--out`` takes the JSON."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "macaque-3d-pose-estimation_amd")
sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from mqhip import _lib as L  # noqa: E402
from mqhip import synth  # noqa: E402
from mqhip.geometry import CameraGroup  # noqa: E402
from mqhip.overlay import SKELETONS, OverlayRenderer, label_tables  # noqa: E402
from mqhip.resize import resize_bilinear  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--base-lib", default=None, help="another libmq_hip.so to alternate the unlabelled render with")
ap.add_argument("--out", default=None, help="write the results as JSON here")
args = ap.parse_args()
out = {"device": torch.cuda.get_device_name(0)}
print(out, flush=True)
dev = torch.device("cuda", 0)
J = 17


def timed(fn, reps, rounds=5):
    """Median and spread over ``rounds`` windows of ``reps`` calls, device events: microseconds per call."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        res.append(1e3 * a.elapsed_time(b) / reps)
    return res


import track_video_ref as ref  # noqa: E402

# ---------------------------------------------------------------- resize vs a plain device copy
H, W, h, w = 1536, 2048, 600, 800
for nimg in (1, 16):
    src_d = torch.randint(0, 256, (nimg, H, W, 3), dtype=torch.uint8, device=dev)
    dst_copy = torch.empty_like(src_d)
    ctx = L.Context.get(0)
    dst = torch.empty((nimg, h, w, 3), dtype=torch.uint8, device=dev)
    s = L.stream_ptr(dev)
    rs = timed(lambda: ctx.lib.mq_resize_bilinear(ctx.handle, L.ptr(src_d), H * W * 3, nimg, H, W, L.ptr(dst), h * w * 3,
                                                  h, w, s), 200)
    cp = timed(lambda: dst_copy.copy_(src_d), 200)
    out[f"resize_n{nimg}"] = dict(resize_us=rs, copy_us=cp, ratio_median=float(np.median(rs) / np.median(cp)),
                                  src_bytes=nimg * H * W * 3, dst_bytes=nimg * h * w * 3)
    print(f"resize n={nimg}", out[f"resize_n{nimg}"], flush=True)
    del src_d, dst_copy, dst

# ---------------------------------------------------------------- overlay draw: parent vs this build, alternating
cams = synth.make_cameras(1)
cg = CameraGroup.from_dicts(cams)
B, A = 4, 4
kp = np.ascontiguousarray(synth.make_skeletons(A, B, seed=2).transpose(1, 0, 2, 3))
sc = np.ones((B, A, J))
frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
new = OverlayRenderer(cg, H, W)
pairs, radius, flags = new._pairs, new._radius, new._flags
P = len(pairs)


class Raw:
    """mq_overlay_render of a library loaded by path (the parent build has none of the new symbols)."""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        res, args = L._SIGS["mq_overlay_render"]
        self.lib.mq_overlay_render.restype, self.lib.mq_overlay_render.argtypes = res, args
        self.lib.mq_create.restype, self.lib.mq_create.argtypes = L._SIGS["mq_create"]
        self.h = C.c_void_p()
        assert self.lib.mq_create(0, C.byref(self.h)) == 0
        up = lambda a: torch.from_numpy(a).to(dev)
        self.cam, self.kp, self.sc = up(np.zeros(B, dtype=np.int32)), up(kp), up(sc)
        self.src = up(np.arange(B, dtype=np.int32))
        self.pi = torch.zeros((B, A, J + 1 + P, 8), dtype=torch.int32, device=dev)
        self.pd = torch.zeros((B, A, P, 4), dtype=torch.float64, device=dev)
        self.out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        self.cams = cg.cams_tensor()

    def __call__(self):
        rc = self.lib.mq_overlay_render(self.h, L.ptr(self.cams), 1, L.ptr(self.cam), L.ptr(self.kp), L.ptr(self.sc), B, A,
                                        J, pairs.ctypes.data, P, radius.ctypes.data, flags.ctypes.data, 3, L.ptr(frames),
                                        H * W * 3, B, L.ptr(self.src), H, W, L.ptr(self.pi), L.ptr(self.pd),
                                        L.ptr(self.out), L.stream_ptr(dev))
        assert rc == 0


runs = {"new": Raw(L.LIB_PATH)}
if args.base_lib:
    runs["parent"] = Raw(args.base_lib)
res = {k: [] for k in runs}
for rnd in range(4):                       # alternate the two builds
    for k, fn in runs.items():
        res[k] += timed(fn, 100, rounds=3)
out["overlay_render_unlabelled_us_per_call_B4"] = res
if "parent" in runs:
    runs["new"]()
    runs["parent"]()
    torch.cuda.synchronize()
    out["unlabelled_new_equals_parent"] = bool(torch.equal(runs["new"].out, runs["parent"].out))
print({k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in res.items()},
      out.get("unlabelled_new_equals_parent"), flush=True)

# the labelled entry on the same frames: colours only, then four 2-digit labels per image
col = np.tile(np.array([2, -1, 0, 3], dtype=np.int32), (B, 1))
labs = [["12", "34", "56", "78"]] * B
largs_c, keep_c = new._label_args(B, A, col, None, 2.0, 5)
largs_l, keep_l = new._label_args(B, A, col, labs, 2.0, 5)
raw = runs["new"]
pi2 = torch.zeros((B, A, J + 2 + P, 8), dtype=torch.int32, device=dev)


def labelled(largs):
    rc = L.load().mq_overlay_render_labelled(
        L.Context.get(0).handle, L.ptr(raw.cams), 1, L.ptr(raw.cam), L.ptr(raw.kp), L.ptr(raw.sc), B, A, J,
        pairs.ctypes.data, P, radius.ctypes.data, flags.ctypes.data, 3, L.ptr(frames), H * W * 3, B, L.ptr(raw.src), H, W,
        *largs, L.ptr(pi2), L.ptr(raw.pd), L.ptr(raw.out), L.stream_ptr(dev))
    assert rc == 0


out["overlay_render_colour_only_us_per_call_B4"] = timed(lambda: labelled(largs_c), 100)
out["overlay_render_labelled_us_per_call_B4"] = timed(lambda: labelled(largs_l), 100)
out["copy_B4_us"] = timed(lambda: raw.out.copy_(frames), 100)
print({k: float(np.median(out[k])) for k in ("overlay_render_colour_only_us_per_call_B4",
                                              "overlay_render_labelled_us_per_call_B4", "copy_B4_us")}, flush=True)
lab_img = raw.out.cpu().numpy()
runs["new"]()
torch.cuda.synchronize()
out["labelled_pixels_beyond_unlabelled"] = int((lab_img != runs["new"].out.cpu().numpy()).any(axis=3).sum())

# ---------------------------------------------------------------- the whole visualize stage at camera size
import tempfile  # noqa: E402

from src.pipeline import step3_crossframematching as s3  # noqa: E402

tmp = tempfile.mkdtemp()
scn = ref.write_scene(tmp, ref.SMALL_RECIPE, H, W, 1)
Trk, Cid, T = s3.main_proc(scn["cfg"], scn["rd"], camparam=scn["camparam"], n_animal=3)
gpu_s = [0.0]


def wrap(obj, name):
    fn = getattr(obj, name)

    def f(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = fn(*a, **k)
        torch.cuda.synchronize()
        gpu_s[0] += time.perf_counter() - t0
        return o
    setattr(obj, name, f)
    return obj


def renderer(*a):
    return wrap(s3._gpu_renderer(*a), "render")


def encoder(*a, **k):
    return wrap(s3._gpu_encoder(*a, **k), "encode")


def resizer(*a, **k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = s3._gpu_resizer(*a, **k)
    torch.cuda.synchronize()
    gpu_s[0] += time.perf_counter() - t0
    return o


def lift(rows):
    from mqhip.association import StepTwoCameras
    from mqhip.tracklets import TrackletLift
    return wrap(TrackletLift(StepTwoCameras(scn["camparam"]), rows, 0), "traces")


stage = []
for i in range(3):
    gpu_s[0] = 0.0
    t0 = time.perf_counter()
    path = s3.visualize(1, scn["cfg"], scn["rd"], scn["raw"], T=T, vidfile_prefix=os.path.join(tmp, f"v{i}_"),
                        camparam=scn["camparam"], renderer=renderer, encoder=encoder, resizer=resizer, lift=lift)
    dt = time.perf_counter() - t0
    from mqhip import io as mqio
    nfr = len(mqio.MjpegAviReader(path))
    stage.append(dict(frames=nfr, total_ms_per_frame=1e3 * dt / nfr, gpu_ms_per_frame=1e3 * gpu_s[0] / nfr,
                      host_io_ms_per_frame=1e3 * (dt - gpu_s[0]) / nfr, avi_bytes=os.path.getsize(path)))
    print(stage[-1], flush=True)
out["visualize_stage_1536x2048_to_800x600"] = stage
import shutil  # noqa: E402

shutil.rmtree(tmp)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
