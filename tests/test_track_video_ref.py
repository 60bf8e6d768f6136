"""CPU: the oracle of step 3's tracking video (tests/track_video_ref.py) pinned by its own properties -- the
fixed-point resize against float64 bilinear, the integer capsule rule against a float64 distance, the stroke font's
bounds -- and ``step3.visualize`` / ``proc(save_vid=True)`` with the NumPy renderer, resizer, encoder and lift."""
import os

import numpy as np
import pytest

import jpeg_ref
import step3_scenes as scenes
import track_video_ref as ref

SHAPES = [((1536, 2048), (600, 800)), ((48, 64), (19, 25)), ((37, 53), (16, 24)), ((20, 30), (40, 45)),
          ((1, 1), (3, 3))]


def _image(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("shape", [(1536, 2048), (48, 64), (37, 53), (1, 1)])
def test_resize_is_the_identity_at_equal_sizes(shape):
    img = _image(*shape)
    assert np.array_equal(ref.resize_bilinear(img, *shape), img)
    assert np.array_equal(ref.resize_bilinear(img[None], *shape)[0], img)


@pytest.mark.parametrize("src,dst", SHAPES)
def test_resize_stays_within_one_grey_level_of_float64_bilinear(src, dst):
    """Rounding alone accounts for 0.5; coefficient quantisation (2^-11) and the two truncating shifts for the
    rest."""
    img = _image(*src, seed=3)
    got = ref.resize_bilinear(img, *dst)
    want = ref.resize_float(img, *dst)
    assert got.shape == (dst[0], dst[1], 3) and got.dtype == np.uint8
    err = np.abs(got.astype(np.float64) - want).max()
    print("max |fixed - float64| =", err)
    assert err < 1.0


def test_resize_taps_clamp_at_the_borders():
    s0, s1, c0, c1, f = ref.resize_taps(20, 40)             # upscaling: the first sample lies left of pixel 0
    assert s0[0] == 0 and c0[0] == 2048 and c1[0] == 0 and s0[-1] == 19 and s1[-1] == 19 and c1[-1] == 0
    assert np.all(c0 + c1 == 2048) and np.all((s1 - s0 >= 0) & (s1 - s0 <= 1))
    s0, s1, c0, c1, f = ref.resize_taps(1, 3)
    assert s0.tolist() == [0, 0, 0] and s1.tolist() == [0, 0, 0] and c0.tolist() == [2048] * 3


@pytest.mark.parametrize("p0,p1,t", [((10, 12), (31, 20), 5), ((20, 5), (20, 30), 4), ((7, 25), (33, 25), 1),
                                      ((30, 30), (8, 9), 7), ((15, 15), (15, 15), 5), ((15, 15), (15, 15), 6),
                                      ((-3, -2), (6, 44), 32)])
def test_capsule_rule_agrees_with_the_float_distance(p0, p1, t):
    xs, ys = np.arange(-20, 60), np.arange(-20, 60)
    got = ref.capsule_mask(p0, p1, t, xs, ys)
    X, Y = np.meshgrid(xs.astype(np.float64), ys.astype(np.float64))
    e = np.array([p1[0] - p0[0], p1[1] - p0[1]], dtype=np.float64)
    ee = e @ e
    u = np.clip(((X - p0[0]) * e[0] + (Y - p0[1]) * e[1]) / ee, 0.0, 1.0) if ee > 0 else np.zeros_like(X)
    d = np.hypot(X - (p0[0] + u * e[0]), Y - (p0[1] + u * e[1]))
    clear = np.abs(d - t / 2.0) > 1e-9
    assert clear.sum() > 0.95 * clear.size and got.any()
    assert np.array_equal(got[clear], (d <= t / 2.0)[clear])


def test_label_mask_is_the_union_of_its_strokes_around_the_origin():
    seg = np.array([[0, 0, 10, 0], [10, 0, 10, -8], [0, 0, 0, 0]], dtype=np.int32)
    slot = np.array([1, 20, 30, 0, 0, 0, 0, 0])
    xs, ys = np.arange(0, 50), np.arange(0, 50)
    m = ref.label_mask(slot, seg, 2, 3, xs, ys)
    want = ref.capsule_mask((20, 30), (30, 30), 3, xs, ys) | ref.capsule_mask((30, 30), (30, 22), 3, xs, ys)
    assert np.array_equal(m, want) and m[30, 25] and m[25, 30] and not m[25, 25]
    assert not ref.label_mask(slot, seg, 0, 3, xs, ys).any()


def test_label_origin_rules():
    p = np.array([[5.9, -7.9], [np.nan, 3.0], [12.0, np.nan]])
    assert ref.label_origin(p) == (5, -7)                    # NaN ignored per axis, truncation toward zero
    assert ref.label_origin(np.full((3, 2), np.nan)) is None
    assert ref.label_origin(np.array([[3000.5, 1.0]])) is None and ref.label_origin(np.array([[3000.0, 1.0]])) == (3000, 1)
    assert ref.label_origin(np.array([[1.0, -1000.5]])) is None and ref.label_origin(np.array([[1.0, -1000.0]])) == (1, -1000)
    assert ref.label_origin(np.array([[1.0, 2.0], [4000.0, 2.0]])) == (1, 2)   # the minimum is gated, not each slot


def test_font_fits_its_cell_and_the_segment_budget():
    from mqhip import overlay as ov
    assert sorted(ov.FONT) == sorted("0123456789-")
    for ch in ov.FONT:
        g = np.array(ov.glyph_segments(ch))
        assert 1 <= len(g) <= ov.MAX_GLYPH_SEGS, ch
        assert g[:, [0, 2]].min() >= 0 and g[:, [0, 2]].max() <= ov.ADVANCE, ch
        assert g[:, [1, 3]].min() >= 0 and g[:, [1, 3]].max() <= ov.CAP_HEIGHT, ch
        assert np.any(g[:, [0, 1]] != g[:, [2, 3]], axis=1).all(), ch         # no zero-length stroke
    for ch in "0123456789":
        assert np.array(ov.glyph_segments(ch))[:, [1, 3]].max() == ov.CAP_HEIGHT, ch    # digits reach the cap height
    worst = max(ov.FONT, key=lambda c: len(ov.glyph_segments(c)))
    m = ov.label_segments("-1")
    assert m.dtype == np.int32 and m.shape == (3, 4) and m[0].tolist() == [6, -18, 30, -18]
    assert m[:, [1, 3]].max() <= 0 and m[:, [1, 3]].min() == -42                 # above the baseline, y flipped
    assert len(ov.label_segments(worst * 6)) <= ov.MAX_LABEL_SEGS
    assert len(ov.label_segments("123456")) <= ov.MAX_LABEL_SEGS
    with pytest.raises(ValueError):
        ov.label_segments(worst * 7)
    with pytest.raises(ValueError):
        ov.label_segments("a1")
    with pytest.raises(ValueError):
        ov.label_segments("1", thickness=33)
    with pytest.raises(ValueError):
        ov.label_segments("11", scale=500.0)
    assert ov.label_segments("7", scale=0.5).tolist() == [[1, -10, 8, -10], [8, -10, 4, 0]]   # half to even
    seg, n = ov.label_tables([["12", None], [None, "-"]], 2, 2)
    assert seg.shape == (2, 2, n.max(), 4) and n.tolist() == [[len(ov.label_segments("12")), 0], [0, 1]]


def test_entry_points_are_declared_and_bound():
    import re
    from mqhip import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mq_hip.h")).read()
    assert _lib.ABI_VERSION == 8 and "#define MQ_ABI_VERSION 8" in header
    for name in ("mq_overlay_primitives_labelled", "mq_overlay_render_labelled", "mq_resize_bilinear"):
        assert name in _lib.EXPORTED and name in _lib._SIGS, name
        m = re.search(r"\b" + name + r"\(([^)]*)\);", header)
        assert m, f"{name} is not declared in include/mq_hip.h"
        assert len(m.group(1).split(",")) == len(_lib._SIGS[name][1]), name
    assert len(_lib._SIGS["mq_overlay_render_labelled"][1]) == len(_lib._SIGS["mq_overlay_render"][1]) + 5


# ----------------------------------------------------------------------------- visualize with everything injected
H, W, SIZE, VIS_CAM = 96, 128, (50, 38), 1


@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    """The small scene on disk with step 3's stages run on the oracle lift: track.pickle / collar_id.pickle."""
    from mqhip import io as mqio
    from src.pipeline import step3_crossframematching as s3
    sc = ref.write_scene(tmp_path_factory.mktemp("scene"), ref.SMALL_RECIPE, H, W, VIS_CAM)
    Trk, Cid, T2, C, n_frame = s3.run_stages(sc["T"], sc["keyframes"], len(sc["cams"]),
                                             lambda rows: scenes.OracleLift(sc["camparam"], rows), n_animal=3)
    assert len(Trk) >= 3 and n_frame > 30
    mqio.dump_pickle(Trk, os.path.join(sc["rd"], "track.pickle"))
    mqio.dump_pickle(Cid, os.path.join(sc["rd"], "collar_id.pickle"))
    sc.update(Trk=Trk, Cid=Cid, T2=T2, n_frame=n_frame)
    return sc


def _visualize(sc, prefix, calls=None, lifts=None, **kw):
    from src.pipeline import step3_crossframematching as s3

    def lift(rows):
        rec = ref.RecordingLift(scenes.OracleLift(sc["camparam"], rows))
        if lifts is not None:
            lifts.append(rec)
        return rec
    return s3.visualize(VIS_CAM, sc["cfg"], sc["rd"], sc["raw"], T=sc["T2"], vidfile_prefix=prefix, size=SIZE,
                        camparam=sc["camparam"], renderer=ref.oracle_renderer_factory(sc["cams"][VIS_CAM], calls),
                        encoder=jpeg_ref.Encoder, resizer=ref.oracle_resizer, lift=lift, **kw)


def test_visualize_frames_colours_and_files(staged, tmp_path):
    from mqhip import io as mqio
    sc = staged
    calls, lifts = [], []
    name = sc["cams"][VIS_CAM]["name"]
    path = _visualize(sc, str(tmp_path / "trk_"), calls, lifts, batch=4, quality=80, fps=12.0)
    assert path == str(tmp_path / f"trk_{name}.avi")
    assert sorted(os.listdir(tmp_path)) == [f"trk_{name}.avi", f"trk_{name}.frame_number.npy", f"trk_{name}.frame_time.npy"]
    rows = list(range(0, sc["n_frame"], 3))
    assert np.load(tmp_path / f"trk_{name}.frame_number.npy").tolist() == [100 + f for f in rows]
    np.testing.assert_array_equal(np.load(tmp_path / f"trk_{name}.frame_time.npy"), 10.0 + (100 + np.array(rows)) / 24.0)
    r = mqio.MjpegAviReader(path)
    assert len(r) == len(rows) and r.fps == 12.0 and (r.height, r.width) == (SIZE[1], SIZE[0])
    live = [any(np.any(t[f] >= 0) for t in sc["Trk"].values()) for f in rows]
    assert lifts[0].calls == sum(any(live[k:k + 4]) for k in range(0, len(rows), 4)) >= 3, "one lift launch per batch"
    want = ref.oracle_video(sc["cams"][VIS_CAM], sc["pool"], sc["Trk"], sc["Cid"], lifts[0].p3d, SIZE, quality=80)
    assert [f for f, _, _, _ in want] == rows
    # colours and labels the renderer was given, frame by frame: the live tracklets in Trk's key order
    got_meta = [([int(c) for c, t in zip(col[b], lab[b]) if t is not None], [t for t in lab[b] if t is not None])
                for col, lab in calls for b in range(len(lab))]
    assert got_meta == [(c, t) for _, c, t, _ in want]
    assert any(len(c) >= 2 for _, c, _, _ in want) and len({v for _, c, _, _ in want for v in c}) >= 2
    for i, (_, _, _, jpg) in enumerate(want):
        assert r.frame_bytes(i) == jpg, i
    # the video draws something: frames with a live tracklet differ from their plain resized source
    plain = [jpeg_ref.encode(ref.resize_bilinear(sc["pool"][i], SIZE[1], SIZE[0]), 80, 16)[0] for i in (0, 1)]
    drawn = [r.frame_bytes(i) != plain[f % 2] for i, f in enumerate(rows)]
    print("frames drawn on:", sum(drawn), "of", len(rows))
    assert sum(drawn) >= sum(live) - 2 and not drawn[0] and not live[0]


def test_visualize_passes_of_eight_and_missing_frames(staged, tmp_path, capsys):
    """Ten copies of every tracklet: two render passes per batch whose result equals one painter's-order pass; a
    frame number absent from the store is skipped with a warning; ``size=None`` keeps the camera's size."""
    from mqhip import io as mqio
    sc = dict(staged)
    keys = list(sc["Trk"].keys())
    many = {10 * j + i: sc["Trk"][k] for j in range(4) for i, k in enumerate(keys)}
    cid = {10 * j + i: np.where(sc["Cid"][k] >= 0, (sc["Cid"][k] + j) % 5 - 1, -1) for j in range(4)
           for i, k in enumerate(keys)}
    rd2 = tmp_path / "results3D" / "clip"
    rd2.mkdir(parents=True)
    name = str(sc["cams"][VIS_CAM]["name"])
    (rd2 / name).mkdir()
    nums = np.load(os.path.join(sc["rd"], name, "frame_num.npy")).copy()
    nums[6] = 7777                                           # row 6 points at a frame the store does not have
    np.save(rd2 / name / "frame_num.npy", nums)
    mqio.dump_pickle(many, str(rd2 / "track.pickle"))
    mqio.dump_pickle(cid, str(rd2 / "collar_id.pickle"))
    sc.update(rd=str(rd2), Trk=many, Cid=cid)
    calls, lifts = [], []
    capsys.readouterr()
    path = _visualize(sc, str(tmp_path / "many_"), calls, lifts, batch=3, step=6)
    assert "[warning] Skipping frame 7777" in capsys.readouterr().out
    n_live = max(sum(bool(np.any(t[f] >= 0)) for t in many.values()) for f in range(0, sc["n_frame"], 6))
    assert n_live > 8 and max(len(lab[0]) for _, lab in calls) == 8
    want = [w for w in ref.oracle_video(sc["cams"][VIS_CAM], sc["pool"], many, cid, lifts[0].p3d | _row6(sc, many),
                                        SIZE, step=6) if w[0] != 6]
    r = mqio.MjpegAviReader(path)
    assert len(r) == len(want)
    for i, (_, _, _, jpg) in enumerate(want):
        assert r.frame_bytes(i) == jpg, i
    # size=None keeps the camera's size and needs no resizer
    from src.pipeline import step3_crossframematching as s3
    full = s3.visualize(VIS_CAM, sc["cfg"], sc["rd"], sc["raw"], T=sc["T2"], vidfile_prefix=str(tmp_path / "full_"),
                        size=None, step=30, camparam=sc["camparam"], encoder=jpeg_ref.Encoder, resizer=None,
                        renderer=ref.oracle_renderer_factory(sc["cams"][VIS_CAM]),
                        lift=lambda rows: scenes.OracleLift(sc["camparam"], rows))
    r = mqio.MjpegAviReader(full)
    assert (r.height, r.width) == (H, W) and len(r) == len(range(0, sc["n_frame"], 30))


def test_visualize_without_tracklets_writes_nothing(staged, tmp_path, capsys):
    from mqhip import io as mqio
    rd2 = tmp_path / "results3D" / "clip"
    rd2.mkdir(parents=True)
    mqio.dump_pickle({}, str(rd2 / "track.pickle"))
    mqio.dump_pickle({}, str(rd2 / "collar_id.pickle"))
    assert _visualize(dict(staged, rd=str(rd2)), str(tmp_path / "none_")) is None
    assert "no tracklets" in capsys.readouterr().out and sorted(os.listdir(tmp_path)) == ["results3D"]


def _row6(sc, Trk):
    """Joints for frame row 6, which the video skips and ``oracle_video`` still walks (its frame is dropped)."""
    return {(i, 6): np.full((17, 3), np.nan) for i in range(len(Trk))}


def test_proc_save_vid_calls_visualize(staged, tmp_path, monkeypatch):
    """``proc(save_vid=True)`` used to raise NotImplementedError; now it hands main_proc's rows to ``visualize``."""
    from mqhip import io as mqio
    from src.pipeline import step3_crossframematching as s3
    sc = staged
    monkeypatch.setattr(s3, "main_proc", lambda *a, **k: (sc["Trk"], sc["Cid"], sc["T2"]))
    res_root = os.path.dirname(sc["rd"])
    name = sc["cams"][VIS_CAM]["name"]
    out = s3.proc("clip", res_root, sc["raw"], sc["cfg"], save_vid=True, save_vid_cam=VIS_CAM,
                  vidfile_prefix=str(tmp_path / "p_"), n_animal=3, size=SIZE, step=10, camparam=sc["camparam"],
                  renderer=ref.oracle_renderer_factory(sc["cams"][VIS_CAM]), encoder=jpeg_ref.Encoder,
                  resizer=ref.oracle_resizer, lift=lambda rows: scenes.OracleLift(sc["camparam"], rows))
    assert out[0] is sc["Trk"]
    r = mqio.MjpegAviReader(str(tmp_path / f"p_{name}.avi"))
    assert len(r) == len(range(0, sc["n_frame"], 10))


def test_visualize_result_proc_size(tmp_path):
    """``visualize_result.proc(size=)``: every rendered frame goes through the resizer before it is stored."""
    import overlay_ref
    from mqhip import io as mqio
    from src.pipeline import visualize_result as vis
    from test_overlay_ref import _scene
    cams, res, cfg, raw, skel, score, pool, numbers = _scene(tmp_path)
    rd = os.path.join(res, "clip")
    mqio.dump_pickle({"kp3d": skel, "kp3d_score": score}, os.path.join(rd, "kp3d.pickle"))
    factory = overlay_ref.oracle_renderer_factory(os.path.join(rd, "calibration.toml"))
    kw = dict(results_dir_root=res, renderer=factory, batch=4)
    a = vis.proc("clip", 1, cfg, raw, out_dir=str(tmp_path / "a"), **kw)
    b = vis.proc("clip", 1, cfg, raw, out_dir=str(tmp_path / "b"), size=(25, 19), resizer=ref.oracle_resizer, **kw)
    fa, fb = mqio.FrameStore(a), mqio.FrameStore(b)
    assert fb.frames.shape == (5, 19, 25, 3) and fa.frame_number.tolist() == fb.frame_number.tolist()
    assert np.array_equal(np.asarray(fb.frames), ref.resize_bilinear(np.asarray(fa.frames), 19, 25))
