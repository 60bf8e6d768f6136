"""CPU: the NumPy JPEG decoder tests/jpeg_dec_ref.py (the restatement csrc/jpeg_dec.hip is compared with byte for
byte) pinned from outside -- it equals Pillow (libjpeg-turbo) on every pixel of every stream both accept -- the host
parser csrc/jpeg_parse.cpp against it field by field and refusal by refusal, and the ``format: mjpeg`` frame store
with the restatement injected as its decoder."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import jpeg_dec_ref as D
import jpeg_ref

def _pil():
    """Pillow's Image module; a machine without Pillow skips the tests that compare with it, and only those."""
    return pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pillow_bgr(data):
    im = _pil().open(io.BytesIO(data))
    im.load()
    return np.asarray(im.convert("RGB"))[..., ::-1]


# ------------------------------------------------------------------------------------------------ the codec
@pytest.mark.parametrize("case", D.streams(), ids=lambda c: c[0])
def test_own_streams_equal_pillow(case):
    name, data = case
    stats = {}
    img, st = D.decode(data, stats=stats)
    assert st == 0 and not stats.get("wrapped")
    assert np.array_equal(img, _pillow_bgr(data))


@pytest.mark.parametrize("size", D.PILLOW_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pillow_streams_equal_pillow(size):
    """4:4:4, 4:2:2, 4:2:0; restart_marker_blocks 1, 2, 3, 5 and restart_marker_rows 1; no restart markers;
    optimize=True; qualities 30, 85, 100; mode L -- at 40 x 56, 17 x 33, 8 x 8, 1 x 1, 31 x 2 (the replication rule)
    and 50 x 47."""
    _pil()
    cases = [(n, d) for n, d in D.pillow_streams() if n.startswith(f"{size[0]}x{size[1]}-")]
    assert len(cases) == len(D.PILLOW_MODES)
    for name, data in cases:
        stats = {}
        img, st = D.decode(data, stats=stats)
        assert st == 0 and not stats.get("wrapped"), name
        assert img.shape == size + (3,) and np.array_equal(img, _pillow_bgr(data)), name


def test_restart_modes_and_long_codes_are_what_the_names_say():
    _pil()
    p = dict(D.pillow_streams())
    assert D.parse(p["50x47-420"]).restart_interval == 0
    assert D.parse(p["40x56-420rb2"]).restart_interval == 2 and D.parse(p["40x56-444rb5"]).restart_interval == 5
    assert (D.parse(p["40x56-422"]).h_luma, D.parse(p["40x56-422"]).v_luma) == (2, 1)
    assert D.parse(p["40x56-L"]).n_comp == 1
    stats = {}
    D.decode(p["40x56-420opt"], stats=stats)
    assert stats["long_codes"] >= 1


@pytest.mark.parametrize("case", D.streams(), ids=lambda c: c[0])
def test_stream_without_dht_uses_the_annex_k_tables(case):
    name, data = case
    bare = D.strip_dht(data)
    assert len(bare) == len(data) - 4 * 4 - 2 * (17 + 12) - 2 * (17 + 162) and b"\xff\xc4" not in bare[:200]
    a, b = D.decode(bare), D.decode(data)
    assert a[1] == b[1] == 0 and np.array_equal(a[0], b[0])


def test_statuses():
    name, data = D.streams()[4]                                    # 48x80ri4
    info = D.parse(data)
    marks = [i for i in range(info.scan_offset, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert len(marks) == 3
    assert D.decode(data[:marks[0]] + data[marks[0] + 2:])[1] == D.ST_MARKERS           # a marker missing
    swapped = bytearray(data)
    swapped[marks[0] + 1], swapped[marks[1] + 1] = swapped[marks[1] + 1], swapped[marks[0] + 1]
    assert D.decode(bytes(swapped))[1] == D.ST_MARKERS                                   # out of sequence
    assert D.decode(data[:marks[1] + 4] + data[marks[2]:])[1] == D.ST_EXHAUSTED
    assert D.decode(data[:info.scan_offset] + b"\xff\x00" * 40 + data[marks[0]:])[1] in (D.ST_NO_CODE, D.ST_RUN)


# ------------------------------------------------------------------------------------------------ the parser
def _c_parse(data):
    from mqhip import _lib, mjpeg
    info = mjpeg.JpegInfo()
    rc = _lib.load().mq_jpeg_parse(bytes(data), len(data), ctypes.byref(info))     # host only: no device
    return rc, info


def _same_info(c, r):
    for f in D.Info.FIELDS:
        assert getattr(c, f) == getattr(r, f), f
    assert np.array_equal(np.ctypeslib.as_array(c.quant), r.quant)
    assert list(c.dc_sel) == r.dc_sel and list(c.ac_sel) == r.ac_sel
    for t in range(2):
        for ours, theirs in ((c.dc[t], r.dc[t]), (c.ac[t], r.ac[t])):
            assert list(ours.bits) == list(theirs[0]) and list(ours.vals) == list(theirs[1])


def test_host_parser_equals_the_restatement_field_by_field():
    try:
        import PIL.Image  # noqa: F401
        extra = D.pillow_streams()
    except ImportError:
        extra = []
    for name, data in D.streams() + extra + [("bare", D.strip_dht(D.streams()[0][1]))]:
        rc, info = _c_parse(data)
        assert rc == 0, name
        _same_info(info, D.parse(data))
    rc, info = _c_parse(D.streams()[2][1])
    assert (info.height, info.width, info.n_comp, info.h_luma, info.v_luma, info.restart_interval,
            info.scan_offset) == (17, 33, 3, 2, 2, 16, jpeg_ref.HEADER_BYTES)


def _own_refusals():
    own = D.streams()[3][1]
    sof = own.index(b"\xff\xc0")
    dht = own.index(b"\xff\xc4")
    return [("header cut short", own[:own.index(b"\xff\xda") + 5], D.E_TRUNCATED),
            ("cut inside DQT", own[:40], D.E_TRUNCATED),
            ("EOI removed", own[:-2], D.E_NO_EOI),
            ("not a JPEG", b"RIFF" + own[4:], D.E_NOT_JPEG),
            ("size 0", b"", D.E_NOT_JPEG),
            ("12 bit", own[:sof + 4] + b"\x0c" + own[sof + 5:], D.E_PRECISION),
            ("Pq 1", own.replace(b"\xff\xdb\x00\x43\x00", b"\xff\xdb\x00\x43\x10", 1), D.E_DQT),
            ("sampling 1x2", own[:sof + 11] + b"\x12" + own[sof + 12:], D.E_SAMPLING),
            ("height 0", own[:sof + 5] + b"\x00\x00" + own[sof + 7:], D.E_SIZE),
            ("undefined table", own.replace(b"\xff\xdb\x00\x43\x01", b"\xff\xdb\x00\x43\x03", 1), D.E_TABLE),
            ("code overflows", own[:dht + 6] + b"\x05\x01" + own[dht + 8:], D.E_HUFFMAN),      # five codes of 2 bits
            ("second scan", own[:-2] + b"\xff\xda\x00\x02\xff\xd9", D.E_SCANS),
            ("Se 62", own[:jpeg_ref.HEADER_BYTES - 2] + b"\x3e" + own[jpeg_ref.HEADER_BYTES - 1:], D.E_SCANS)]


def _check_refusal(data, code):
    with pytest.raises(D.ParseError) as e:
        D.parse(data)
    assert e.value.code == code
    assert _c_parse(data)[0] == code
    from mqhip.mjpeg import JpegError, parse_header
    with pytest.raises(JpegError) as e:
        parse_header(data, frame=3)
    assert (e.value.frame, e.value.code) == (3, code)


@pytest.mark.parametrize("case", _own_refusals(), ids=lambda c: c[0])
def test_refusals_return_their_codes(case):
    _check_refusal(case[1], case[2])


@pytest.mark.parametrize("kind", ["progressive", "cmyk", "header cut short", "EOI removed"])
def test_refusals_of_pillow_streams_return_their_codes(kind):
    Image = _pil()
    img = D.mixed_image(24, 40, 5)
    good = D.pillow_stream(img, quality=85)
    if kind == "progressive":
        data, code = D.pillow_stream(img, progressive=True), D.E_SOF
    elif kind == "cmyk":
        b = io.BytesIO()
        Image.fromarray(img).convert("CMYK").save(b, "JPEG")
        data, code = b.getvalue(), D.E_COMPONENTS
    elif kind == "header cut short":
        data, code = good[:good.index(b"\xff\xda") + 5], D.E_TRUNCATED
    else:
        data, code = good[:-2], D.E_NO_EOI
    _check_refusal(data, code)


def test_header_and_abi():
    from mqhip import _lib, mjpeg
    assert "mq_jpeg_parse" in _lib.EXPORTED and "mq_jpeg_decode" in _lib.EXPORTED and _lib.ABI_VERSION == 8
    assert len(_lib._SIGS["mq_jpeg_parse"][1]) == 3 and len(_lib._SIGS["mq_jpeg_decode"][1]) == 10
    src = open(os.path.join(ROOT, "include", "mq_hip.h")).read()
    assert re.search(r"^int mq_jpeg_parse\(const uint8_t\* \w+, int64_t \w+, mq_jpeg_info\* \w+\);", src, re.M)
    m = re.search(r"^int mq_jpeg_decode\(([^;]*)\);", src, re.M | re.S)
    assert m and len(m.group(1).split(",")) == 10
    codes = {k: int(v) for k, v in re.findall(r"#define MQ_JPEG_E_(\w+) \((-\d+)\)", src)}
    assert codes == {k[2:]: getattr(D, k) for k in dir(D) if k.startswith("E_")} and len(set(codes.values())) == 12
    assert set(mjpeg.PARSE_ERRORS) == set(codes.values()) and set(mjpeg.STATUS) == {1, 2, 3, 4}
    assert ctypes.sizeof(mjpeg.JpegInfo) == 1320 < 4096               # kernels take it by value
    assert "#define MQ_ABI_VERSION 8" in src
    dev = open(os.path.join(ROOT, "macaque-3d-pose-estimation_amd", "csrc", "jpeg_dec_dev.hpp")).read()
    assert f"JPEG_DEC_LOOK_BITS = {D.LOOK_BITS};" in dev
    parse_cpp = open(os.path.join(ROOT, "macaque-3d-pose-estimation_amd", "csrc", "jpeg_parse.cpp")).read()
    assert "hip/" not in parse_cpp                                     # the host compiler builds it alone


# ------------------------------------------------------------------------------------------------- the store
def _stores(tmp_path, n_pool=5, max_bytes=2 ** 31 - 2 ** 20):
    from mqhip import io as mqio
    pool = np.stack([D.mixed_image(48, 64, s) for s in range(n_pool)])
    numbers = np.arange(20, 20 + 2 * n_pool)
    index = np.arange(2 * n_pool) % n_pool
    src, dst = str(tmp_path / "clip.7"), str(tmp_path / "packed" / "clip.7")
    tracks = [[[1.0, 2.0, 30.0, 40.0, float(i)]] for i in range(len(numbers))]
    preds = [[{"pred_label": 1, "pred_score": 0.5}] for _ in numbers]
    mqio.write_frame_store(src, pool, 5.0 + numbers / 24.0, numbers, tracks, 7, id_preds=preds, frame_index=index)
    raw, packed = mqio.convert_frame_store(src, dst, quality=85, restart_interval=4, batch=2,
                                           encoder=jpeg_ref.Encoder, max_bytes=max_bytes)
    assert raw == pool.nbytes and 0 < packed < raw
    return mqio, pool, numbers, index, src, dst


def test_mjpeg_store_through_the_injected_decoder(tmp_path):
    mqio, pool, numbers, index, src, dst = _stores(tmp_path)
    a, b = mqio.FrameStore(src), mqio.FrameStore(dst, decoder=D.Decoder)
    assert a.format == "npy" and isinstance(a.frames, np.memmap) and b.format == "mjpeg"
    assert not os.path.exists(os.path.join(dst, "frames.npy"))
    assert mqio.mjpeg_avi_files(os.path.join(dst, "frames.avi")) == [os.path.join(dst, "frames.avi")]
    assert b.frames.shape == a.frames.shape == (5, 48, 64, 3) and b.frames.dtype == np.uint8 and len(b.frames) == 5
    assert b.frame_number.tolist() == numbers.tolist() and b.frame_index.tolist() == index.tolist()
    assert np.array_equal(a.frame_time, b.frame_time) and a.tracks == b.tracks and a.id_preds == b.id_preds
    want = [D.decode(jpeg_ref.encode(im, 85, 4)[0])[0] for im in pool]
    for fn, k in zip(numbers, index):
        assert np.array_equal(b.image(fn), want[k]) and np.array_equal(a.image(fn), pool[k])
    assert np.array_equal(np.asarray(b.frames[int(2)]), want[2]) and np.array_equal(np.asarray(b.frames), want)
    with pytest.raises(IndexError):
        b.frames[5]


def test_mjpeg_frames_keep_a_small_lru(tmp_path):
    mqio, pool, numbers, index, src, dst = _stores(tmp_path)
    calls = []

    class Counting(D.Decoder):
        def decode(self, streams):
            calls.append(len(streams))
            return super().decode(streams)

    frames = mqio.MjpegFrames(os.path.join(dst, "frames.avi"), decoder=Counting, cache=2)
    for i in (0, 0, 0, 1, 0, 1):
        frames[i]
    assert calls == [1, 1]
    frames[2], frames[1]                                               # 2 evicts 0, the least recently used
    assert calls == [1, 1, 1]
    frames[0]
    assert calls == [1, 1, 1, 1]
    assert np.array_equal(frames.device_frames([3, 3, 1]), np.stack([frames[3], frames[3], frames[1]]))


def test_rollover_files_are_read_in_order(tmp_path):
    mqio, pool, numbers, index, src, dst = _stores(tmp_path, max_bytes=9000)
    files = mqio.mjpeg_avi_files(os.path.join(dst, "frames.avi"))
    assert len(files) >= 2 and files[1].endswith("frames.001.avi")
    b = mqio.FrameStore(dst, decoder=D.Decoder)
    assert len(b.frames) == 5 and [len(r) for r in b.frames.readers] != [5]
    for k in range(5):
        assert np.array_equal(b.frames[k], D.decode(jpeg_ref.encode(pool[k], 85, 4)[0])[0])


def test_convert_refuses_what_it_should(tmp_path):
    mqio, pool, numbers, index, src, dst = _stores(tmp_path)
    with pytest.raises(FileExistsError):
        mqio.convert_frame_store(src, dst, encoder=jpeg_ref.Encoder)
    with pytest.raises(ValueError):
        mqio.convert_frame_store(dst, str(tmp_path / "again"), encoder=jpeg_ref.Encoder)


def test_proc_video_avi_from_an_mjpeg_store_equals_the_npy_store_of_the_decoded_frames(tmp_path):
    """Every factory injected (NumPy renderer, encoder and decoder): the overlay stage reads the mjpeg store
    through the shim and writes the same AVI, byte for byte, as from an npy store that holds the decoded frames."""
    import overlay_ref as ref
    from mqhip import io as mqio
    from src.pipeline import visualize_result as vis
    from test_overlay_ref import _scene
    cams, res, cfg, raw, skel, score, pool, numbers = _scene(tmp_path)
    rd = os.path.join(res, "clip")
    mqio.dump_pickle({"kp3d": skel, "kp3d_score": score}, os.path.join(rd, "kp3d.pickle"))
    cam = str(cams[1]["name"])
    src = os.path.join(raw, f"clip.{cam}")
    raw_j, raw_d = str(tmp_path / "videos_mjpeg"), str(tmp_path / "videos_decoded")
    mqio.convert_frame_store(src, os.path.join(raw_j, f"clip.{cam}"), quality=90, restart_interval=4,
                             encoder=jpeg_ref.Encoder)
    st = mqio.FrameStore(os.path.join(raw_j, f"clip.{cam}"), decoder=D.Decoder)
    mqio.write_frame_store(os.path.join(raw_d, f"clip.{cam}"), np.asarray(st.frames), st.frame_time, st.frame_number,
                           st.tracks, cam, frame_index=st.frame_index)
    kw = dict(results_dir_root=res, batch=4, video="avi", quality=90, fps=24.0, encoder=jpeg_ref.Encoder,
              renderer=ref.oracle_renderer_factory(os.path.join(rd, "calibration.toml")))
    a = vis.proc("clip", 1, cfg, raw_j, out_dir=str(tmp_path / "a"), decoder=D.Decoder, **kw)
    b = vis.proc("clip", 1, cfg, raw_d, out_dir=str(tmp_path / "b"), **kw)
    assert a.endswith(".avi") and open(a, "rb").read() == open(b, "rb").read()
    assert len(mqio.MjpegAviReader(a)) == 5
