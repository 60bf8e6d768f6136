"""GPU: the pose overlay (csrc/overlay.hip through mqhip.overlay.OverlayRenderer, src.pipeline.visualize_result
and run_demo's ``visualize``) against the NumPy oracle tests/overlay_ref.py -- tables field by field and images
byte for byte: the camera projection is bit-exact and both coverage rules are exact, so nothing has a tolerance."""
import os

import numpy as np
import pytest

import overlay_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

J = 17


def _skeleton(name):
    from mqhip.overlay import SKELETONS
    sk = SKELETONS[name]
    return sk.pairs, sk.radius(3), sk.flags


def _plane_camera(name="0"):
    """A pinhole camera with f = 1, c = 0, R = I, t = 0 and no distortion: (X, Y, 1) projects to pixel (X, Y)
    exactly, so a test places joints in pixels."""
    return dict(name=name, size=[94, 50], matrix=np.eye(3), distortions=np.zeros(5), rotation=np.zeros(3),
                translation=np.zeros(3), rvec=np.zeros(3), tvec=np.zeros(3), fisheye=False, omnidir=False)


def test_primitive_tables_match_the_oracle_field_by_field():
    from mqhip import synth
    from mqhip.geometry import CameraGroup
    from mqhip.overlay import OverlayRenderer
    cams = synth.make_cameras(3) + [synth.make_cameras_model(8, "pinhole")[3], synth.make_cameras_model(8, "fisheye")[4]]
    cam_of_img = np.array([0, 1, 2, 3, 4, 1], dtype=np.int32)          # camera 1 twice
    B, A = 6, 5
    kp3d = np.ascontiguousarray(synth.make_skeletons(A, B, seed=7).transpose(1, 0, 2, 3))    # (B, A, J, 3)
    score = np.random.default_rng(1).uniform(0.05, 1.0, (B, A, J))
    kp3d[0, 0, 3] = np.nan                  # a NaN joint: its disc and limbs go
    kp3d[1, 2, 5] = np.nan                  # a NaN shoulder: the neck goes too
    kp3d[2, 1, 9, 0] = 0.0                  # X == 0: flag clear, still drawn
    score[3, 4] = 0.0                       # every score 0: cnt == 0, nothing of the animal
    score[4, 0, 6] = 0.0                    # one score 0: the joint is still drawn (cnt > 0)
    score[5, 3, 2] = np.nan
    oracle_cams = [ref.make_cam(c) for c in cams]
    gated = []
    for b in range(B):      # push one joint of animal 1 away until its projection leaves the (-1000, 3000) gates
        centre = kp3d[b, 1].mean(axis=0)
        for scale in 2.0 ** np.arange(1, 12):
            p = centre + scale * (kp3d[b, 1, 10] - centre + 0.05)
            u = oracle_cams[cam_of_img[b]].project(p[None])[0]
            if np.isfinite(u).all() and (u.max() > 3000 or u.min() < -1000):
                kp3d[b, 1, 10] = p
                gated.append(b)
                break
    assert gated, "no planted joint leaves the gates"
    for name in ("v1", "v2"):
        pairs, radius, flags = _skeleton(name)
        want_i, want_d = ref.primitives(cams, cam_of_img, kp3d, score, pairs, radius, flags, 3)
        assert all(want_i[b, 1, 10, 0] == 0 for b in gated) and want_i[3, 4].sum() == 0 and want_i[2, 1, 9, 0] == 1   # the plants took
        assert want_i[1, 2, J, 0] == 0 and want_i[..., 0].mean() > 0.5
        got_i, got_d = OverlayRenderer(CameraGroup.from_dicts(cams), 1536, 2048, skeleton=name).primitives(
            cam_of_img, kp3d, score)
        assert got_i.shape == want_i.shape and got_d.shape == want_d.shape
        for f, field in enumerate(("valid", "cx", "cy", "r", "x0", "y0", "x1", "y1")):
            assert np.array_equal(got_i[..., f], want_i[..., f]), (name, field)
        for f, field in enumerate(("x1", "y1", "x2", "y2")):
            bad = np.argwhere(got_d[..., f] != want_d[..., f])
            assert np.array_equal(got_d[..., f], want_d[..., f]), (name, field, bad[:4].tolist())


def test_draw_awkward_pitch_pool_and_borders():
    """H = 50, W = 94: rows of 282 bytes (the byte path), two tiles each way (a tile is 256 bytes x 32 rows: the
    borders cut pixel 85 and lie under row 31).  A pool of 2 sources feeds 6 outputs; primitives straddle the tile
    borders and leave the image on all four sides; output 4 has nothing to draw.  Then the same poses stretched
    over H = 70, W = 96 (rows of 288 bytes: the vector path, a partial second tile, three tile rows)."""
    import torch
    from mqhip.geometry import CameraGroup
    from mqhip.overlay import OverlayRenderer
    H, W, B, A = 50, 94, 6, 5
    cam = _plane_camera()
    rng = np.random.default_rng(5)
    pool = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    src = np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)
    kp3d = np.ones((B, A, J, 3))
    kp3d[..., 0] = rng.uniform(-12.0, W + 12.0, (B, A, J))
    kp3d[..., 1] = rng.uniform(-12.0, H + 12.0, (B, A, J))
    kp3d[0, 0, 0, :2] = (85.2, 31.7)         # on both tile borders
    kp3d[0, 1, 5, :2] = (-2.7, -1.2)         # corners and edges, negative centres
    kp3d[0, 1, 6, :2] = (95.9, 51.4)
    kp3d[1, 0, 7, :2] = (40.0, -3.0)
    kp3d[1, 0, 9, :2] = (40.0, 52.9)
    kp3d[1, 2, 8, :2] = (-3.0, 25.0)
    kp3d[1, 2, 10, :2] = (96.5, 25.0)
    kp3d[2, 3, 11, :2] = kp3d[2, 3, 13, :2]  # a zero-length limb
    kp3d[3, :, :, 0] = 1e4                   # everything outside the gates but animal 2
    kp3d[3, 2, :, 0] = rng.uniform(80.0, 92.0, J)
    score = np.ones((B, A, J))
    score[4] = 0.0                           # nothing to draw: the output is its source
    pairs, radius, flags = _skeleton("v1")
    want = ref.render(pool, [cam], np.zeros(B, dtype=int), kp3d, score, pairs, radius, flags, 3, src)
    assert np.array_equal(want[4], pool[1]) and (want[0] != pool[0]).any()
    r = OverlayRenderer(CameraGroup.from_dicts([cam]), H, W)
    pool_d = torch.from_numpy(pool).cuda()
    got = r.render(pool_d, 0, kp3d, score, src_index=src)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, H, W, 3)
    assert np.array_equal(pool_d.cpu().numpy(), pool), "the source pool was written"
    got = got.cpu().numpy()
    for b in range(B):
        bad = np.argwhere((got[b] != want[b]).any(axis=2))
        assert len(bad) == 0, (b, len(bad), bad[:5].tolist())
    # the vector path: the poses stretched to 70 rows, one joint on the corner of the four lowest tiles
    kp3d[..., 1] *= 70.0 / H
    kp3d[0, 0, 0, :2] = (85.2, 63.7)
    pool96 = rng.integers(0, 256, (2, 70, 96, 3), dtype=np.uint8)
    want96 = ref.render(pool96, [cam], np.zeros(B, dtype=int), kp3d, score, pairs, radius, flags, 3, src)
    got96 = OverlayRenderer(CameraGroup.from_dicts([cam]), 70, 96).render(pool96, 0, kp3d, score, src_index=src)
    assert np.array_equal(got96.cpu().numpy(), want96)


def test_render_rejects_bad_arguments():
    from mqhip.geometry import CameraGroup
    from mqhip.overlay import OverlayRenderer
    r = OverlayRenderer(CameraGroup.from_dicts([_plane_camera()]), 8, 16)
    frames = np.zeros((1, 8, 16, 3), dtype=np.uint8)
    with pytest.raises(ValueError):
        r.render(frames, 0, np.ones((1, 9, J, 3)), np.ones((1, 9, J)))          # more than 8 animals
    with pytest.raises(ValueError):
        r.render(frames, 0, np.ones((2, 1, J, 3)), np.ones((2, 1, J)), src_index=[0, 1])
    with pytest.raises(ValueError):
        r.render(frames, 1, np.ones((1, 1, J, 3)), np.ones((1, 1, J)))          # no such camera


@pytest.mark.parametrize("name", ["v1", "v2"])
def test_draw_full_size_vector_path(name):
    """One 1536 x 2048 image (rows of 6144 bytes: 16-byte accesses), 4 animals."""
    from mqhip import synth
    from mqhip.geometry import CameraGroup
    from mqhip.overlay import OverlayRenderer
    cams = synth.make_cameras(1)
    kp3d = np.ascontiguousarray(synth.make_skeletons(4, 1, seed=2).transpose(1, 0, 2, 3))
    score = np.ones((1, 4, J))
    frame = np.random.default_rng(3).integers(0, 256, (1, 1536, 2048, 3), dtype=np.uint8)
    pairs, radius, flags = _skeleton(name)
    want = ref.render(frame, cams, [0], kp3d, score, pairs, radius, flags, 3)
    changed = int((want != frame).any(axis=3).sum())
    assert changed > 500, "the scene draws (almost) nothing"
    got = OverlayRenderer(CameraGroup.from_dicts(cams), 1536, 2048, skeleton=name).render(frame, 0, kp3d, score)
    got = got.cpu().numpy()
    bad = np.argwhere((got[0] != want[0]).any(axis=2))
    assert len(bad) == 0, (len(bad), bad[:5].tolist())


# ----------------------------------------------------------------------------------------------- the stage
N_FRAMES, N_VIEWS, N_ANIMALS, H, W = 12, 3, 2, 120, 160


def _expected_store(cam_dict, raw, res, cam_i, data, skeleton="v1"):
    """The oracle composition of one camera's overlay store: (frame numbers, frames)."""
    from mqhip import io as mqio
    name = str(cam_dict["name"])
    store = mqio.FrameStore(os.path.join(raw, f"clip.{name}"))
    frame_num = np.load(os.path.join(res, "clip", name, "frame_num.npy"))
    X, S = np.asarray(data["kp3d"]), np.asarray(data["kp3d_score"])
    have = set(int(n) for n in store.frame_number)
    rows = [(i, int(frame_num[i])) for i in range(X.shape[1]) if int(frame_num[i]) in have]
    idx = [i for i, _ in rows]
    pairs, radius, flags = _skeleton(skeleton)
    imgs = np.stack([store.image(fn) for _, fn in rows])
    frames = ref.render(imgs, [cam_dict], np.zeros(len(rows), dtype=int), X[:, idx].transpose(1, 0, 2, 3),
                        S[:, idx].transpose(1, 0, 2), pairs, radius, flags, 3)
    return [fn for _, fn in rows], frames, imgs


def test_stage_visualize_result_and_run_demo(tmp_path, capsys):
    import torch
    import run_demo
    from mqhip import io as mqio
    from mqhip import synth
    from mqhip.apis import PoseModelHip
    from mqhip.weights import VIT_TINY, make_random_weights
    from src.pipeline import visualize_result as vis
    cams, raw, res, cfg, truth = synth.write_clip(str(tmp_path), "clip", n_frames=N_FRAMES, n_views=N_VIEWS,
                                                  n_animals=N_ANIMALS, height=H, width=W)
    sx, sy = W / 2048.0, H / 1536.0
    for c in cams:      # the clip's cameras see 2048 x 1536: scale them, and the tracker boxes, to the small frames
        c["K"] = np.asarray(c["K"], dtype=np.float64) * np.array([[sx], [sy], [1.0]])
        d = os.path.join(raw, f"clip.{c['name']}")
        st = mqio.FrameStore(d)
        imgs, times, nums, fidx = np.array(st.frames), st.frame_time, st.frame_number, st.frame_index
        tracks = [[[r[0] * sx, r[1] * sy, r[2] * sx, r[3] * sy] + list(r[4:]) for r in t] for t in st.tracks]
        del st
        mqio.write_frame_store(d, imgs, times, nums, tracks, c["name"], frame_index=fidx)
    synth.write_calibration_toml(cams, os.path.join(res, "clip", "calibration.toml"))
    w = synth.confident_head(make_random_weights(VIT_TINY, seed=0, device=torch.device("cuda", 0)))
    pose = PoseModelHip(VIT_TINY, w, 0)
    run = lambda **kw: run_demo.proc("clip", 24, res, "cuda:0", cfg, raw, 17, n_animal=N_ANIMALS, pose_model=pose,
                                     id_model="random", **kw)
    rd = os.path.join(res, "clip")

    # the default chain renders nothing and makes no output directory
    out_none = str(tmp_path / "out_none")
    data = run(out_dir=out_none)
    assert not os.path.exists(out_none) and os.path.exists(os.path.join(rd, "kp3d.pickle"))

    # visualize_result.proc on step 4's kp3d.pickle
    out_a = str(tmp_path / "out_a")
    path = vis.proc("clip", 0, cfg, raw, results_dir_root=res, out_dir=out_a, batch=5)
    assert path == os.path.join(out_a, f"clip_{cams[0]['name']}")
    store = mqio.FrameStore(path)
    numbers, want, _ = _expected_store(cams[0], raw, res, 0, mqio.load_array_pickle(os.path.join(rd, "kp3d.pickle")))
    assert store.frame_number.tolist() == numbers and len(numbers) == data["kp3d"].shape[1]
    assert np.array_equal(np.asarray(store.frames), want)
    assert store.tracks == [[] for _ in numbers]

    # run_demo with visualize=[0] yields the same store (and only camera 0's)
    out_b = str(tmp_path / "out_b")
    run(visualize=[0], out_dir=out_b)
    assert sorted(os.listdir(out_b)) == [f"clip_{cams[0]['name']}"]
    again = mqio.FrameStore(os.path.join(out_b, f"clip_{cams[0]['name']}"))
    assert again.frame_number.tolist() == numbers and np.array_equal(np.asarray(again.frames), want)

    # a pose that is certainly in view (the clip's own skeletons) through the preferred pickle; camera 1's store
    # loses a frame number, which is skipped with a warning; a second call returns early
    skel = synth.make_skeletons(N_ANIMALS, N_FRAMES + 1, seed=2)[:, :data["kp3d"].shape[1]]
    fixed = {"kp3d": skel, "kp3d_score": np.ones(skel.shape[:3])}
    mqio.dump_pickle(fixed, os.path.join(rd, "kp3d_fxdJointLen.pickle"))
    name1 = str(cams[1]["name"])
    full = mqio.FrameStore(os.path.join(raw, f"clip.{name1}"))
    lost = int(np.load(os.path.join(rd, name1, "frame_num.npy"))[4])
    keep = [i for i, n in enumerate(full.frame_number) if int(n) != lost]
    raw2 = str(tmp_path / "videos2")
    mqio.write_frame_store(os.path.join(raw2, f"clip.{name1}"), np.asarray(full.frames), full.frame_time[keep],
                           full.frame_number[keep], [full.tracks[i] for i in keep], name1,
                           frame_index=full.frame_index[keep])
    capsys.readouterr()
    path1 = vis.proc("clip", 1, cfg, raw2, results_dir_root=res, out_dir=out_a)
    assert f"[warning] Skipping frame {lost}" in capsys.readouterr().out
    store1 = mqio.FrameStore(path1)
    numbers1, want1, src1 = _expected_store(cams[1], raw2, res, 1, fixed)
    assert lost not in numbers1 and len(numbers1) == len(numbers) - 1
    assert store1.frame_number.tolist() == numbers1 and np.array_equal(np.asarray(store1.frames), want1)
    assert int((want1 != src1).any(axis=3).sum()) > 50, "the in-view pose draws (almost) nothing"
    assert vis.proc("clip", 1, cfg, raw2, results_dir_root=res, out_dir=out_a) is None
    assert "already exists:" in capsys.readouterr().out
