"""GPU: the baseline JPEG encoder (csrc/jpeg.hip through mqhip.mjpeg.JpegEncoder) against the NumPy restatement
tests/jpeg_ref.py, byte for byte -- the codec is integer-only, so nothing has a tolerance -- and
``visualize_result.proc(video='avi')`` on the device against the same run with the NumPy renderer and encoder."""
import os

import numpy as np
import pytest

import jpeg_ref
import overlay_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]


def _encode(img, quality, ri):
    from mqhip.mjpeg import JpegEncoder
    return JpegEncoder(img.shape[0], img.shape[1], quality=quality, restart_interval=ri).encode(img[None])[0]


def _first_difference(got, want):
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return dict(lengths=(len(got), len(want)), at=k, got=got[max(k - 4, 0):k + 8].hex(),
                want=want[max(k - 4, 0):k + 8].hex())


@pytest.mark.parametrize("case", jpeg_ref.streams(), ids=lambda c: c[0])
def test_small_streams_equal_the_reference(case):
    """A single MCU (DC + EOB only); the stress image at quality 100, RI 1 (DC category 11, AC category 10, ZRLs,
    blocks without EOB, stuffed bytes, an RSTn index past RST7 -- asserted on the reference's own statistics);
    17 x 33 and 40 x 24 (padding on each axis, the byte-wise load path); 48 x 80 at RI 4 (W / 16 = 5: intervals span
    the ends of MCU rows, the 16-byte load path); qualities 1, 50, 75, 90 and 100."""
    name, img, quality, ri = case
    want, st = jpeg_ref.encode(img, quality, ri)
    if name == "stress":
        assert 11 in st["dc_cat"] and 10 in st["ac_cat"] and st["zrl"] and st["no_eob"] and st["stuffed"]
        assert st["rst"] == 11
    if name == "flat16":
        assert st["blocks"] == 6 and st["eob"] == 6 and st["zrl"] == 0
    got = _encode(img, quality, ri)
    assert got == want, _first_difference(got, want)


@pytest.mark.parametrize("ri,quality", [(16, 90), (32, 50)])
def test_wide_image_vector_path(ri, quality):
    """64 x 2048: rows of 6144 bytes (16-byte loads), 512 MCUs, 32 or 16 restart intervals."""
    img = jpeg_ref.smooth_image(64, 2048, 5)
    img[16:32] = np.random.default_rng(ri).integers(0, 256, (16, 2048, 3), dtype=np.uint8)
    want, st = jpeg_ref.encode(img, quality, ri)
    assert st["rst"] == 512 // ri - 1
    got = _encode(img, quality, ri)
    assert got == want, _first_difference(got, want)


def test_batch_slots_are_independent_and_untouched_past_their_size():
    """n = 3 different images, a device tensor and a host array, two calls: equal bytes, every out_size right, and
    the bytes past out_size still hold the sentinel the slots were filled with."""
    import torch
    from mqhip.mjpeg import JpegEncoder
    rng = np.random.default_rng(3)
    imgs = np.stack([jpeg_ref.smooth_image(40, 56, 7), rng.integers(0, 256, (40, 56, 3), dtype=np.uint8),
                     np.full((40, 56, 3), 255, dtype=np.uint8)])
    want = [jpeg_ref.encode(im, 75, 4)[0] for im in imgs]
    assert len(set(len(w) for w in want)) == 3
    enc = JpegEncoder(40, 56, quality=75, restart_interval=4)
    assert enc.max_bytes == jpeg_ref.max_bytes(40, 56, 4)
    dev = torch.from_numpy(imgs).cuda()
    out = torch.full((3, enc.max_bytes + 37), 0xA5, dtype=torch.uint8, device="cuda")     # a stride above the bound
    sizes = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    enc.encode_into(dev, out, sizes)
    out, sizes = out.cpu().numpy(), sizes.cpu().numpy()
    assert sizes.tolist() == [len(w) for w in want]
    for i in range(3):
        assert out[i, :sizes[i]].tobytes() == want[i], (i, _first_difference(out[i, :sizes[i]].tobytes(), want[i]))
        assert (out[i, sizes[i]:] == 0xA5).all(), i
    assert np.array_equal(dev.cpu().numpy(), imgs), "the frames were written"
    assert enc.encode(dev) == want           # a device tensor
    assert enc.encode(imgs) == want          # a host array, and a second (third) call: the same bytes
    o2, s2 = enc.encode_device(dev)
    assert tuple(o2.shape) == (3, enc.max_bytes) and s2.cpu().tolist() == [len(w) for w in want]
    assert enc.encode(imgs[:0]) == []


def test_bad_arguments():
    import torch
    from mqhip._lib import MqError
    from mqhip.mjpeg import JpegEncoder
    for kw, word in ((dict(height=0), "height"), (dict(width=65536), "width"), (dict(quality=0), "quality"),
                     (dict(quality=101), "quality"), (dict(restart_interval=0), "restart_interval"),
                     (dict(restart_interval=33), "restart_interval")):
        a = dict(height=16, width=16)
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            JpegEncoder(**a)
    enc = JpegEncoder(16, 32)
    with pytest.raises(ValueError):
        enc.encode(np.zeros((1, 16, 16, 3), dtype=np.uint8))
    frames = torch.zeros((1, 16, 32, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((1, enc.max_bytes - 1), 0xA5, dtype=torch.uint8, device="cuda")       # one byte short
    sizes = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(MqError, match=r"\(-2\).*out_stride"):
        enc.encode_into(frames, out, sizes)
    assert (out.cpu().numpy() == 0xA5).all() and sizes.cpu().tolist() == [-1]


def test_proc_video_avi_on_the_device_equals_the_injected_run(tmp_path):
    """The scene of tests/test_overlay_ref.py: GPU renderer + GPU encoder against NumPy renderer + NumPy encoder,
    the AVI files byte for byte."""
    from mqhip import io as mqio
    from src.pipeline import visualize_result as vis
    from test_overlay_ref import H, W, _scene
    cams, res, cfg, raw, skel, score, pool, numbers = _scene(tmp_path)
    rd = os.path.join(res, "clip")
    mqio.dump_pickle({"kp3d": skel, "kp3d_score": score}, os.path.join(rd, "kp3d.pickle"))
    kw = dict(results_dir_root=res, batch=4, video="avi", quality=90, fps=24.0)
    gpu = vis.proc("clip", 1, cfg, raw, out_dir=str(tmp_path / "gpu"), **kw)
    cpu = vis.proc("clip", 1, cfg, raw, out_dir=str(tmp_path / "cpu"), encoder=jpeg_ref.Encoder,
                   renderer=ref.oracle_renderer_factory(os.path.join(rd, "calibration.toml")), **kw)
    assert os.path.basename(gpu) == os.path.basename(cpu) and gpu.endswith(".avi")
    assert open(gpu, "rb").read() == open(cpu, "rb").read()
    r = mqio.MjpegAviReader(gpu)
    assert len(r) == 5 and (r.height, r.width) == (H, W)
    for side in ("frame_number", "frame_time"):
        assert np.array_equal(np.load(gpu[:-4] + f".{side}.npy"), np.load(cpu[:-4] + f".{side}.npy"))


def test_run_demo_video_avi_holds_the_rendered_overlay(tmp_path):
    """run_demo with ``visualize=[0], visualize_video='avi'`` (the CLI's ``--visualize 0 --video avi``): every
    frame of the AVI is the reference stream of the frame the frame-store path renders, and Pillow decodes it."""
    import io

    import torch
    import run_demo
    from mqhip import io as mqio
    from mqhip import synth
    from mqhip.apis import PoseModelHip
    from mqhip.weights import VIT_TINY, make_random_weights
    n_frames, n_views, n_animals, h, w = 6, 3, 2, 120, 160
    cams, raw, res, cfg, truth = synth.write_clip(str(tmp_path), "clip", n_frames=n_frames, n_views=n_views,
                                                  n_animals=n_animals, height=h, width=w)
    sx, sy = w / 2048.0, h / 1536.0
    for c in cams:      # the clip's cameras see 2048 x 1536: scale them, and the tracker boxes, to the small frames
        c["K"] = np.asarray(c["K"], dtype=np.float64) * np.array([[sx], [sy], [1.0]])
        d = os.path.join(raw, f"clip.{c['name']}")
        st = mqio.FrameStore(d)
        imgs, times, nums, fidx = np.array(st.frames), st.frame_time, st.frame_number, st.frame_index
        tracks = [[[r[0] * sx, r[1] * sy, r[2] * sx, r[3] * sy] + list(r[4:]) for r in t] for t in st.tracks]
        del st
        mqio.write_frame_store(d, imgs, times, nums, tracks, c["name"], frame_index=fidx)
    synth.write_calibration_toml(cams, os.path.join(res, "clip", "calibration.toml"))
    wts = synth.confident_head(make_random_weights(VIT_TINY, seed=0, device=torch.device("cuda", 0)))
    pose = PoseModelHip(VIT_TINY, wts, 0)
    run = lambda **kw: run_demo.proc("clip", 24, res, "cuda:0", cfg, raw, 17, n_animal=n_animals, pose_model=pose,
                                     id_model="random", visualize=[0], **kw)
    name = cams[0]["name"]
    out_v, out_s = str(tmp_path / "out_video"), str(tmp_path / "out_store")
    run(out_dir=out_v, visualize_video="avi", video_quality=80)
    run(out_dir=out_s)
    assert sorted(os.listdir(out_v)) == [f"clip_{name}.avi", f"clip_{name}.frame_number.npy",
                                         f"clip_{name}.frame_time.npy"]
    store = mqio.FrameStore(os.path.join(out_s, f"clip_{name}"))
    r = mqio.MjpegAviReader(os.path.join(out_v, f"clip_{name}.avi"))
    assert len(r) == len(store.frame_number) > 0 and r.fps == 24.0 and (r.height, r.width) == (h, w)
    assert np.load(os.path.join(out_v, f"clip_{name}.frame_number.npy")).tolist() == store.frame_number.tolist()
    for i in range(len(r)):
        assert r.frame_bytes(i) == jpeg_ref.encode(np.asarray(store.frames[i]), 80, 16)[0], i
    try:
        from PIL import Image
    except ImportError:
        return
    im = Image.open(io.BytesIO(r.frame_bytes(0)))
    im.load()
    assert im.size == (w, h)
