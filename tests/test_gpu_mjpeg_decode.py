"""GPU: the baseline JPEG decoder (csrc/jpeg_dec.hip through mqhip.mjpeg.JpegDecoder) against the NumPy restatement
tests/jpeg_dec_ref.py, byte for byte -- the codec is integer-only, so nothing has a tolerance.  The restatement is
pinned to Pillow by tests/test_jpeg_dec_ref.py and the malformed streams used here ran clean through the host
program of tests/test_jpeg_dec_host.py."""
import numpy as np
import pytest

import jpeg_dec_ref as D
import jpeg_ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

CASES = D.case_streams()
_REF = {}


def _ref(name):
    if name not in _REF:
        stats = {}
        img, st = D.decode(CASES[name], stats=stats)
        assert st == 0
        _REF[name] = (img, stats)
    return _REF[name]


def _where(got, want):
    bad = np.argwhere(got != want)
    return dict(shape=(got.shape, want.shape), n_bad=len(bad), first=bad[:4].tolist())


@pytest.mark.parametrize("name", list(CASES))
def test_small_streams_equal_the_reference(name):
    """flat16 (one MCU, DC only); the stress image at quality 100, RI 1 (DC category 11, AC category 10, ZRLs, blocks
    without EOB, stuffed bytes, an RSTn index past RST7); 17 x 33 and 40 x 24 (cropping, chroma edges at the true
    extent); 48 x 80 at RI 4 (intervals across MCU-row ends); 31 x 2 and 1 x 1 (the replication rule); Pillow's
    4:2:2, 4:4:4 and L; an optimize=True stream with codes longer than the first-level lookup; 50 x 47 without restart
    markers (the one-lane path)."""
    from mqhip.mjpeg import JpegDecoder
    want, stats = _ref(name)
    if name == "40x56-420opt":
        assert stats.get("long_codes", 0) >= 1          # the slow path is known to run
    if name == "50x47-420":
        assert D.parse(CASES[name]).restart_interval == 0
    got = JpegDecoder().decode([CASES[name]])
    assert got.shape == (1,) + want.shape and got.dtype == np.uint8
    assert np.array_equal(got[0], want), _where(got[0], want)


@pytest.mark.parametrize("ri", [4, 3])
def test_many_intervals(ri):
    """64 x 2048, 512 MCUs at RI 4 and RI 3: 128 and 171 intervals, so more than one wave per frame and a partly
    filled last wave; 16-byte marker loads over more than two of the marker kernel's 16 KB steps."""
    from mqhip.mjpeg import JpegDecoder
    img = jpeg_ref.smooth_image(64, 2048, 5)
    img[16:32] = np.random.default_rng(ri).integers(0, 256, (16, 2048, 3), dtype=np.uint8)
    data, st = jpeg_ref.encode(img, 75, ri)
    assert st["rst"] + 1 == -(-512 // ri) and len(data) > 2 * 16384
    want, status = D.decode(data)
    assert status == 0
    got = JpegDecoder().decode([data])[0]
    assert np.array_equal(got, want), _where(got, want)


def _slots(streams, info, pad, odd=False):
    """Device (streams, sizes, out, status) for one decode_into call: out rows of H * W * 3 + pad bytes of 0xA5."""
    import torch
    stride = (max(len(s) for s in streams) + 15) // 16 * 16 + (7 if odd else 0)
    host = np.zeros((len(streams), stride), dtype=np.uint8)
    for r, s in enumerate(streams):
        host[r, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    out = torch.full((len(streams), info.height * info.width * 3 + pad), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((len(streams),), -7, dtype=torch.int32, device="cuda")
    sizes = torch.tensor([len(s) for s in streams], dtype=torch.int32, device="cuda")
    return torch.from_numpy(host).cuda(), sizes, out, status


def test_batch_groups_strides_and_sentinels():
    """Three images of one header plus one with other tables (a second group); decode_into with a frame_stride above
    H * W * 3 leaves the pad bytes untouched; two calls give the same bits."""
    from mqhip.mjpeg import JpegDecoder, parse_header
    rng = np.random.default_rng(3)
    imgs = [jpeg_ref.smooth_image(40, 56, 7), rng.integers(0, 256, (40, 56, 3), dtype=np.uint8),
            np.full((40, 56, 3), 255, dtype=np.uint8)]
    streams = [jpeg_ref.encode(im, 75, 4)[0] for im in imgs] + [jpeg_ref.encode(imgs[0], 30, 4)[0]]
    want = np.stack([D.decode(s)[0] for s in streams])
    dec = JpegDecoder()
    got = dec.decode(streams)
    assert np.array_equal(got, want), _where(got, want)
    assert np.array_equal(dec.decode(streams), got)
    with pytest.raises(ValueError):
        dec.decode([streams[0], CASES["17x33"]])
    info = parse_header(streams[0])
    n = 40 * 56 * 3
    for odd in (False, True):                   # 16-byte marker loads, and the byte path of an odd stride
        dev, sizes, out, status = _slots(streams[:3], info, 37, odd)
        dec.decode_into(dev, sizes, info, out, status)
        out = out.cpu().numpy()
        assert status.cpu().tolist() == [0, 0, 0]
        assert np.array_equal(out[:, :n].reshape(3, 40, 56, 3), want[:3])
        assert (out[:, n:] == 0xA5).all()


def test_encode_device_chains_into_decode_into():
    """JpegEncoder.encode_device -> decode_into with no host copy of the streams (the header comes from the
    encoder's own arguments)."""
    import torch
    from mqhip.mjpeg import JpegDecoder, JpegEncoder, parse_header
    imgs = np.stack([jpeg_ref.smooth_image(40, 56, s) for s in (1, 2)])
    enc = JpegEncoder(40, 56, quality=80, restart_interval=4)
    streams, sizes = enc.encode_device(torch.from_numpy(imgs).cuda())
    info = parse_header(jpeg_ref.header(40, 56, 80, 4) + b"\xff\xd9")
    out = torch.empty((2, 40, 56, 3), dtype=torch.uint8, device="cuda")
    status = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    JpegDecoder().decode_into(streams, sizes, info, out, status)
    assert status.cpu().tolist() == [0, 0]
    want = np.stack([D.decode(jpeg_ref.encode(im, 80, 4)[0])[0] for im in imgs])
    assert np.array_equal(out.cpu().numpy(), want)


def test_workspace_growth_small_large_small():
    from mqhip.mjpeg import JpegDecoder
    dec = JpegDecoder()
    small, big = CASES["flat16"], jpeg_ref.encode(jpeg_ref.smooth_image(96, 160, 3), 90, 8)[0]
    want_small, want_big = D.decode(small)[0], D.decode(big)[0]
    assert np.array_equal(dec.decode([small])[0], want_small)
    assert np.array_equal(dec.decode([big, big])[1], want_big)
    assert np.array_equal(dec.decode([small])[0], want_small)


def test_malformed_streams_set_their_status_and_nothing_else():
    """A scan cut inside an interval (with its EOI put back) and one corrupted interval, in a batch with good frames:
    the statuses are the restatement's, the good frames are right, the sentinels intact."""
    from mqhip.mjpeg import JpegDecoder, JpegError, parse_header
    good = jpeg_ref.encode(jpeg_ref.smooth_image(48, 80, 9), 75, 4)[0]
    info, ref_info = parse_header(good), D.parse(good)
    marks = [i for i in range(ref_info.scan_offset, len(good) - 1) if good[i] == 0xFF and 0xD0 <= good[i + 1] <= 0xD7]
    cut = good[:marks[1] + 4] + good[marks[2]:]                      # interval 2 keeps two bytes
    noisy = bytearray(good)
    rng = np.random.default_rng(11)
    for p in range(marks[0] + 2, marks[1]):                          # interval 1: random bytes, no 0xFF
        noisy[p] = int(rng.integers(0, 255))
    no_eoi = good[:-2]
    streams = [good, cut, bytes(noisy), no_eoi, good]
    want = [D.decode(s, ref_info) for s in streams]
    assert [st for _, st in want] == [0, want[1][1], want[2][1], 1, 0] and want[1][1] == 4 and want[2][1] in (2, 3, 4)
    dec = JpegDecoder()
    dev, sizes, out, status = _slots(streams, info, 64)
    dec.decode_into(dev, sizes, info, out, status)
    out, n = out.cpu().numpy(), 48 * 80 * 3
    assert status.cpu().tolist() == [st for _, st in want]
    for i in (0, 4):
        assert np.array_equal(out[i, :n].reshape(48, 80, 3), want[i][0]), i
    assert (out[:, n:] == 0xA5).all()
    with pytest.raises(JpegError) as e:
        dec.decode([good, cut])
    assert (e.value.frame, e.value.code) == (1, 4)
    with pytest.raises(JpegError) as e:
        dec.decode([good, no_eoi])
    assert (e.value.frame, e.value.code) == (1, -30)


def test_bad_arguments():
    import torch
    from mqhip._lib import MqError
    from mqhip.mjpeg import JpegDecoder, parse_header
    data = CASES["40x24"]
    info = parse_header(data)
    dev, sizes, out, status = _slots([data], info, -1)               # one byte short
    with pytest.raises(MqError, match=r"\(-2\).*frame_stride"):
        JpegDecoder().decode_into(dev, sizes, info, out, status)
    assert (out.cpu().numpy() == 0xA5).all() and status.cpu().tolist() == [-7]
    assert JpegDecoder().decode([]).shape == (0, 0, 0, 3)


def test_decode_into_reads_views_with_their_own_strides():
    """A column slice of wider tensors (stride(0) above the row length) decodes right and leaves the rest of the
    wider output alone; tensors whose rows are not contiguous, or of another dtype, are refused before the call."""
    import torch
    from mqhip.mjpeg import JpegDecoder, parse_header
    streams = [CASES["40x24"], CASES["40x24"]]
    info = parse_header(streams[0])
    want, n = D.decode(streams[0])[0], 40 * 24 * 3
    dev, sizes, out, status = _slots(streams, info, 0)
    wide = torch.zeros((2, dev.shape[1] + 48), dtype=torch.uint8, device="cuda")
    wide[:, :dev.shape[1]] = dev
    wide_out = torch.full((2, n + 40), 0xA5, dtype=torch.uint8, device="cuda")
    dec = JpegDecoder()
    dec.decode_into(wide[:, :dev.shape[1]], sizes, info, wide_out[:, :n], status)
    got = wide_out.cpu().numpy()
    assert status.cpu().tolist() == [0, 0] and (got[:, n:] == 0xA5).all()
    assert np.array_equal(got[0, :n].reshape(want.shape), want) and np.array_equal(got[1, :n].reshape(want.shape), want)
    for bad in (dict(dev_streams=wide[:, ::2]), dict(dev_sizes=sizes.long()), dict(status=status.cpu()),
                dict(out=wide_out[:, :n:2])):
        a = dict(dev_streams=dev, dev_sizes=sizes, info=info, out=out, status=status)
        a.update(bad)
        with pytest.raises(ValueError):
            dec.decode_into(**a)


# --------------------------------------------------------------------------------------------- frame stores
def test_proc_video_avi_from_an_mjpeg_store_on_the_device_equals_the_injected_run(tmp_path):
    """The scene of tests/test_overlay_ref.py with its store converted on the GPU: GPU decoder + renderer + encoder
    (the decoded batch stays on the device) against the NumPy decoder, renderer and encoder, the AVI files byte for
    byte."""
    import os

    import overlay_ref as ref
    from mqhip import io as mqio
    from src.pipeline import visualize_result as vis
    from test_overlay_ref import H, W, _scene
    cams, res, cfg, raw, skel, score, pool, numbers = _scene(tmp_path)
    rd = os.path.join(res, "clip")
    mqio.dump_pickle({"kp3d": skel, "kp3d_score": score}, os.path.join(rd, "kp3d.pickle"))
    cam = str(cams[1]["name"])
    raw_j = str(tmp_path / "videos_mjpeg")
    n_raw, n_jpg = mqio.convert_frame_store(os.path.join(raw, f"clip.{cam}"), os.path.join(raw_j, f"clip.{cam}"),
                                            quality=90, restart_interval=4)
    assert n_raw == pool.nbytes and 0 < n_jpg
    st = mqio.FrameStore(os.path.join(raw_j, f"clip.{cam}"))
    assert st.format == "mjpeg" and st.frames.shape == (2, H, W, 3)
    for k in range(2):      # the GPU encoder wrote the restatement's streams and the shim decodes them
        assert st.frames.frame_bytes(k) == jpeg_ref.encode(pool[k], 90, 4)[0]
        assert np.array_equal(st.frames[k], D.decode(st.frames.frame_bytes(k))[0])
    kw = dict(results_dir_root=res, batch=4, video="avi", quality=90, fps=24.0)
    gpu = vis.proc("clip", 1, cfg, raw_j, out_dir=str(tmp_path / "gpu"), **kw)
    cpu = vis.proc("clip", 1, cfg, raw_j, out_dir=str(tmp_path / "cpu"), encoder=jpeg_ref.Encoder, decoder=D.Decoder,
                   renderer=ref.oracle_renderer_factory(os.path.join(rd, "calibration.toml")), **kw)
    assert gpu.endswith(".avi") and open(gpu, "rb").read() == open(cpu, "rb").read()
    assert len(mqio.MjpegAviReader(gpu)) == 5


def test_run_demo_on_mjpeg_stores_equals_npy_stores_of_the_decoded_frames(tmp_path):
    """run_demo (steps 1-4 and ``visualize=[0], visualize_video='avi'``) on ``format: mjpeg`` stores: the same
    kp3d.pickle and AVI bytes as on npy stores that hold the decoded frames."""
    import os
    import shutil

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
    raw_j, raw_d = str(tmp_path / "videos_mjpeg"), str(tmp_path / "videos_decoded")
    for c in cams:      # the clip's cameras see 2048 x 1536: scale them, and the tracker boxes, to the small frames
        c["K"] = np.asarray(c["K"], dtype=np.float64) * np.array([[sx], [sy], [1.0]])
        d = os.path.join(raw, f"clip.{c['name']}")
        st = mqio.FrameStore(d)
        imgs, times, nums, fidx = np.array(st.frames), st.frame_time, st.frame_number, st.frame_index
        tracks = [[[r[0] * sx, r[1] * sy, r[2] * sx, r[3] * sy] + list(r[4:]) for r in t] for t in st.tracks]
        del st
        mqio.write_frame_store(d, imgs, times, nums, tracks, c["name"], frame_index=fidx)
        mqio.convert_frame_store(d, os.path.join(raw_j, f"clip.{c['name']}"), quality=92, restart_interval=8)
        sj = mqio.FrameStore(os.path.join(raw_j, f"clip.{c['name']}"))
        mqio.write_frame_store(os.path.join(raw_d, f"clip.{c['name']}"), np.asarray(sj.frames), times, nums, tracks,
                               c["name"], frame_index=fidx)
    synth.write_calibration_toml(cams, os.path.join(res, "clip", "calibration.toml"))
    res_j, res_d = str(tmp_path / "results_mjpeg"), str(tmp_path / "results_decoded")
    shutil.copytree(res, res_j), shutil.copytree(res, res_d)
    wts = synth.confident_head(make_random_weights(VIT_TINY, seed=0, device=torch.device("cuda", 0)))
    pose = PoseModelHip(VIT_TINY, wts, 0)
    run = lambda res_dir, raw_dir, out: run_demo.proc(
        "clip", 24, res_dir, "cuda:0", cfg, raw_dir, 17, n_animal=n_animals, pose_model=pose, id_model="random",
        visualize=[0], visualize_video="avi", video_quality=80, out_dir=out)
    out_j, out_d = str(tmp_path / "out_mjpeg"), str(tmp_path / "out_decoded")
    run(res_j, raw_j, out_j)
    run(res_d, raw_d, out_d)
    a = mqio.load_array_pickle(os.path.join(res_j, "clip", "kp3d.pickle"))
    b = mqio.load_array_pickle(os.path.join(res_d, "clip", "kp3d.pickle"))
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    name = cams[0]["name"]
    assert sorted(os.listdir(out_j)) == sorted(os.listdir(out_d)) and f"clip_{name}.avi" in os.listdir(out_j)
    assert open(os.path.join(out_j, f"clip_{name}.avi"), "rb").read() == \
        open(os.path.join(out_d, f"clip_{name}.avi"), "rb").read()
    assert len(mqio.MjpegAviReader(os.path.join(out_j, f"clip_{name}.avi"))) > 0
