"""CPU: the Motion-JPEG AVI container (mqhip.io.MjpegAviWriter / MjpegAviReader) and ``visualize_result.proc``'s
``video='avi'`` path with the NumPy renderer (tests/overlay_ref.py) and the NumPy encoder (tests/jpeg_ref.py)
injected.  No media player exists in the test environment: the structure is pinned here, playback is not."""
import io
import os
import struct

import numpy as np
import pytest

import jpeg_ref
import overlay_ref as ref
from test_overlay_ref import H, W, _scene


def _payloads():
    return [bytes([i + 1]) * n for i, n in enumerate((100, 101, 1, 2, 255))]    # odd and even lengths


def test_writer_reader_round_trip(tmp_path):
    from mqhip import io as mqio
    path = str(tmp_path / "sub" / "a.avi")
    w = mqio.MjpegAviWriter(path, 48, 64, fps=29.97)
    for i, p in enumerate(_payloads()):
        w.append(p, 10 + i, 0.5 * i)
    w.close()
    w.close()                                                  # idempotent
    with pytest.raises(ValueError):
        w.append(b"x")
    assert mqio.mjpeg_avi_files(path) == [path]
    r = mqio.MjpegAviReader(path)
    assert len(r) == 5 and (r.width, r.height) == (64, 48) and r.fps == pytest.approx(29.97, abs=1e-9)
    assert [r.frame_bytes(i) for i in range(5)] == _payloads()
    assert np.load(str(tmp_path / "sub" / "a.frame_number.npy")).tolist() == [10, 11, 12, 13, 14]
    assert np.load(str(tmp_path / "sub" / "a.frame_time.npy")).tolist() == [0.0, 0.5, 1.0, 1.5, 2.0]


def test_header_fields_and_index_offsets(tmp_path):
    from mqhip import io as mqio
    path = str(tmp_path / "a.avi")
    w = mqio.MjpegAviWriter(path, 48, 64, fps=24.0)
    for p in _payloads():
        w.append(p)
    w.close()
    assert sorted(os.listdir(tmp_path)) == ["a.avi"]           # no numbers given: no side files
    d = open(path, "rb").read()
    u32 = lambda at: struct.unpack_from("<I", d, at)[0]
    assert d[:4] == b"RIFF" and u32(4) == len(d) - 8 and d[8:12] == b"AVI "
    assert d[12:16] == b"LIST" and d[20:24] == b"hdrl" and u32(16) == 4 + 64 + 12 + 64 + 48
    assert d[24:28] == b"avih" and u32(28) == 56
    avih = struct.unpack_from("<14I", d, 32)
    assert avih[0] == 41667 and avih[3] == 0x10 and avih[4] == 5 and avih[6] == 1       # us / frame, HASINDEX
    assert avih[7] == 255 and avih[8:10] == (64, 48)
    assert d[88:92] == b"LIST" and d[96:100] == b"strl" and d[100:104] == b"strh" and u32(104) == 56
    assert d[108:116] == b"vidsMJPG"
    scale, rate, start, length = struct.unpack_from("<4I", d, 108 + 20)
    assert (scale, rate, start, length) == (1, 24, 0, 5)
    assert d[164:168] == b"strf" and u32(168) == 40
    bih = struct.unpack_from("<IiiHH4sI", d, 172)
    assert bih == (40, 64, 48, 1, 24, b"MJPG", 64 * 48 * 3)
    assert d[212:216] == b"LIST" and d[220:224] == b"movi"
    movi_bytes = sum(8 + len(p) + (len(p) & 1) for p in _payloads())
    assert u32(216) == 4 + movi_bytes
    at = 224 + movi_bytes
    assert d[at:at + 4] == b"idx1" and u32(at + 4) == 16 * 5 and at + 8 + 80 == len(d)
    pos = 224
    for i, p in enumerate(_payloads()):
        cc, flags, off, size = struct.unpack_from("<4sIII", d, at + 8 + 16 * i)
        assert (cc, flags, size) == (b"00dc", 0x10, len(p))
        assert 220 + off == pos and d[pos:pos + 4] == b"00dc" and u32(pos + 4) == len(p)   # offset from 'movi'
        assert d[pos + 8:pos + 8 + len(p)] == p
        pos += 8 + len(p) + (len(p) & 1)
        assert pos % 2 == 0


def test_rollover_with_a_tiny_max_bytes(tmp_path):
    from mqhip import io as mqio
    path = str(tmp_path / "r.avi")
    w = mqio.MjpegAviWriter(path, 48, 64, max_bytes=700)
    payloads = [bytes([i]) * (100 + i) for i in range(7)]
    for i, p in enumerate(payloads):
        w.append(p, i, i / 24.0)
    w.close()
    files = mqio.mjpeg_avi_files(path)
    assert files == [path, str(tmp_path / "r.001.avi"), str(tmp_path / "r.002.avi")] == w.paths
    got = []
    for f in files:
        assert os.path.getsize(f) <= 700
        r = mqio.MjpegAviReader(f)
        got += [r.frame_bytes(i) for i in range(len(r))]
    assert got == payloads
    assert np.load(str(tmp_path / "r.frame_number.npy")).tolist() == list(range(7))     # beside the first file
    with pytest.raises(ValueError):
        mqio.MjpegAviWriter(str(tmp_path / "s.avi"), 48, 64, max_bytes=300).append(b"x" * 400)


def test_writer_rejects_bad_arguments(tmp_path):
    from mqhip import io as mqio
    for kw in (dict(path="a.mp4"), dict(height=0), dict(width=65536), dict(fps=0.0), dict(max_bytes=2 ** 32)):
        a = dict(path=str(tmp_path / "a.avi"), height=16, width=16)
        a.update(kw)
        with pytest.raises(ValueError):
            mqio.MjpegAviWriter(**a)
    bad = tmp_path / "bad.avi"
    bad.write_bytes(b"RIFF\x00\x00\x00\x00AVI ")
    with pytest.raises(ValueError):
        mqio.MjpegAviReader(str(bad))


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_proc_video_avi_with_injected_renderer_and_encoder(tmp_path, capsys):
    Image = pytest.importorskip("PIL.Image")
    from mqhip import io as mqio
    from mqhip.overlay import SKELETONS
    from src.pipeline import visualize_result as vis
    cams, res, cfg, raw, skel, score, pool, numbers = _scene(tmp_path)
    rd = os.path.join(res, "clip")
    mqio.dump_pickle({"kp3d": skel, "kp3d_score": score}, os.path.join(rd, "kp3d.pickle"))
    factory = ref.oracle_renderer_factory(os.path.join(rd, "calibration.toml"))
    cam = str(cams[1]["name"])
    out = str(tmp_path / "output")
    kw = dict(results_dir_root=res, out_dir=out, renderer=factory, batch=4)

    path = vis.proc("clip", 1, cfg, raw, video="avi", quality=85, fps=30.0, encoder=jpeg_ref.Encoder, **kw)
    assert path == os.path.join(out, f"clip_{cam}.avi")
    assert sorted(os.listdir(out)) == [f"clip_{cam}.avi", f"clip_{cam}.frame_number.npy", f"clip_{cam}.frame_time.npy"]
    r = mqio.MjpegAviReader(path)
    assert len(r) == 5 and r.fps == 30.0 and (r.height, r.width) == (H, W)
    assert np.load(os.path.join(out, f"clip_{cam}.frame_number.npy")).tolist() == [10, 11, 12, 14, 15]
    np.testing.assert_array_equal(np.load(os.path.join(out, f"clip_{cam}.frame_time.npy")),
                                  100.0 + np.array([10, 11, 12, 14, 15]) / 24.0)
    sk = SKELETONS["v1"]
    kept, src = [0, 1, 2, 4, 5], np.array([0, 1, 0, 1, 0])
    want = ref.render(pool, [cams[1]], np.zeros(5, dtype=int), skel[:, kept].transpose(1, 0, 2, 3),
                      score[:, kept].transpose(1, 0, 2), sk.pairs, sk.radius(3), sk.flags, 3, src)
    psnr = lambda a, b: 10 * np.log10(255.0 ** 2 / max(np.mean((a.astype(float) - b.astype(float)) ** 2), 1e-12))
    for i in range(5):
        direct = jpeg_ref.encode(want[i], 85, 16)[0]
        assert r.frame_bytes(i) == direct                      # the rendered frame's own stream
        dec = lambda b: np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))[..., ::-1]
        assert dec(r.frame_bytes(i)).shape == want[i].shape
        assert psnr(dec(r.frame_bytes(i)), want[i]) >= psnr(dec(direct), want[i])

    # already exists: the early return tests the .avi and leaves it alone
    before = open(path, "rb").read()
    capsys.readouterr()
    assert vis.proc("clip", 1, cfg, raw, video="avi", encoder=jpeg_ref.Encoder, **kw) is None
    assert "already exists:" in capsys.readouterr().out and open(path, "rb").read() == before
    with pytest.raises(ValueError):
        vis.proc("clip", 1, cfg, raw, video="mp4", **kw)


def test_proc_default_still_writes_the_same_frame_store(tmp_path):
    """``video=None`` is the frame-store path: its directory equals the one the same call without the new
    arguments writes, file for file, and the new arguments are inert."""
    from mqhip import io as mqio
    from src.pipeline import visualize_result as vis
    cams, res, cfg, raw, skel, score, pool, numbers = _scene(tmp_path)
    rd = os.path.join(res, "clip")
    mqio.dump_pickle({"kp3d": skel, "kp3d_score": score}, os.path.join(rd, "kp3d.pickle"))
    factory = ref.oracle_renderer_factory(os.path.join(rd, "calibration.toml"))

    def boom(*a, **k):
        raise AssertionError("the encoder must not be built on the frame-store path")
    a, b = str(tmp_path / "out_a"), str(tmp_path / "out_b")
    pa = vis.proc("clip", 1, cfg, raw, results_dir_root=res, out_dir=a, renderer=factory, batch=4)
    pb = vis.proc("clip", 1, cfg, raw, results_dir_root=res, out_dir=b, renderer=factory, batch=4, video=None,
                  quality=10, fps=5.0, encoder=boom)
    cam = str(cams[1]["name"])
    assert pa == os.path.join(a, f"clip_{cam}") and pb == os.path.join(b, f"clip_{cam}")
    ta, tb = _tree(a), _tree(b)
    assert sorted(ta) == sorted(os.path.join(f"clip_{cam}", f) for f in
                                ("frame_number.npy", "frame_time.npy", "frames.npy", "metadata.yaml", "tracks.json"))
    assert ta == tb
    store = mqio.FrameStore(pa)
    assert store.frame_number.tolist() == [10, 11, 12, 14, 15] and store.frames.shape == (5, H, W, 3)
