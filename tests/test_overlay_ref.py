"""CPU: the pose-overlay oracle (tests/overlay_ref.py) pinned by known answers, the skeleton tables against the
reference's lists, the C ABI additions, and ``visualize_result.proc``'s file logic with the oracle injected as
the renderer."""
import os

import numpy as np
import pytest
import yaml

import overlay_ref as ref

J = 17


class PlaneCam:
    """A camera whose projection is (X, Y): the tests place the joints in pixels directly."""

    def project(self, p3d):
        return np.asarray(p3d, dtype=np.float64)[:, :2].copy()


def v1():
    from mqhip.overlay import SKELETONS
    sk = SKELETONS["v1"]
    return sk.pairs, sk.radius(3), sk.flags


def pose(default=(-500.0, -500.0)):
    """(J, 3) joints far off the image (still inside the gates) and scores of 1."""
    x = np.zeros((J, 3))
    x[:, 0], x[:, 1], x[:, 2] = default[0], default[1], 1.0
    return x, np.ones(J)


def table(discs=(), limbs=(), n_animals=1, animal=0, P=4):
    """Hand-made tables of one image: discs (cx, cy, r) and limbs (x1, y1, x2, y2) of one animal, mrksize 3."""
    prim_i = np.zeros((n_animals, J + 1 + P, 8), dtype=np.int32)
    prim_d = np.zeros((n_animals, P, 4))
    for k, (cx, cy, r) in enumerate(discs):
        prim_i[animal, k] = [1, cx, cy, r, cx - r, cy - r, cx + r, cy + r]
    for k, (x1, y1, x2, y2) in enumerate(limbs):
        prim_d[animal, k] = [x1, y1, x2, y2]
        prim_i[animal, J + 1 + k] = [1, 0, 0, 0, np.floor(min(x1, x2) - 1.5), np.floor(min(y1, y2) - 1.5),
                                     np.ceil(max(x1, x2) + 1.5), np.ceil(max(y1, y2) + 1.5)]
    return prim_i, prim_d


def drawn(img):
    """Boolean (H, W): pixels that differ from the grey 7 background."""
    return (img != 7).any(axis=2)


BG = np.full((32, 40, 3), 7, dtype=np.uint8)


def test_disc_r3_row_widths():
    m = ref.disc_mask(10, 10, 3, np.arange(0, 21), np.arange(0, 21))
    assert m.sum(axis=1)[7:14].tolist() == [3, 5, 7, 7, 7, 5, 3] and m.sum() == 37
    img = ref.draw_image(BG, *table(discs=[(10, 10, 3)]), J)
    assert np.array_equal(drawn(img)[:21, :21], m) and drawn(img).sum() == 37
    assert (img[10, 10] == (255, 0, 0)).all()


def test_horizontal_limb_covers_25_pixels():
    img = ref.draw_image(BG, *table(limbs=[(10, 10, 20, 10)]), J)
    want = np.zeros(BG.shape[:2], dtype=bool)
    want[10, 10:21] = True
    want[9, 12:19] = True
    want[11, 12:19] = True
    assert want.sum() == 25 and np.array_equal(drawn(img), want)


def test_vertical_limb_is_the_transpose():
    """ex == 0: the reference special-cases the angle; the rule needs no case."""
    img = ref.draw_image(BG, *table(limbs=[(10, 10, 10, 20)]), J)
    want = np.zeros(BG.shape[:2], dtype=bool)
    want[10:21, 10] = True
    want[12:19, 9] = True
    want[12:19, 11] = True
    assert np.array_equal(drawn(img), want)


def test_zero_length_limb_draws_nothing():
    img = ref.draw_image(BG, *table(limbs=[(10.25, 10.5, 10.25, 10.5)]), J)
    assert np.array_equal(img, BG)
    assert not ref.limb_mask(10, 10, 10, 10, 3, np.arange(5, 15), np.arange(5, 15)).any()


def test_higher_animal_wins_and_the_fifth_is_black():
    pi0, pd0 = table(discs=[(10, 10, 3)], n_animals=5, animal=0)
    pi3, pd3 = table(discs=[(13, 10, 3)], n_animals=5, animal=3)
    pi4, pd4 = table(discs=[(30, 20, 2)], n_animals=5, animal=4)
    img = ref.draw_image(BG, pi0 + pi3 + pi4, pd0 + pd3 + pd4, J)
    assert (img[10, 11] == (255, 255, 255)).all()      # overlap: animal 3 over animal 0
    assert (img[10, 8] == (255, 0, 0)).all()           # animal 0 alone
    assert (img[20, 30] == (0, 0, 0)).all()            # the fifth animal
    assert [ref.colour_of(a) for a in range(6)] == [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255),
                                                    (0, 0, 0), (0, 0, 0)]


def test_cnt_zero_draws_nothing():
    pairs, radius, flags = v1()
    x, s = pose((20.0, 15.0))
    pi, pd = ref.animal_primitives(PlaneCam(), x, np.zeros(J), pairs, radius, flags, 3)
    assert not pi.any() and not pd.any()
    pi, pd = ref.animal_primitives(PlaneCam(), x, s, pairs, radius, flags, 3)
    assert pi[:J + 1, 0].all() and pi[J + 1:, 0].all()


def test_zero_x_joint_is_still_drawn():
    """The accident the kernel keeps: X == 0 clears the joint's flag only, so with cnt > 0 it is drawn."""
    pairs, radius, flags = v1()
    x, s = pose((20.0, 15.0))
    x[9, 0] = 0.0
    pi, _ = ref.animal_primitives(PlaneCam(), x, s, pairs, radius, flags, 3)
    assert pi[9].tolist() == [1, 0, 15, 3, -3, 12, 3, 18]
    x[:, 0] = 0.0                                        # every flag clear: cnt == 0
    pi, _ = ref.animal_primitives(PlaneCam(), x, s, pairs, radius, flags, 3)
    assert not pi.any()


def test_nan_joint_drops_its_disc_and_limbs():
    pairs, radius, flags = v1()
    x, s = pose((20.0, 15.0))
    x[7] = np.nan                                        # left elbow: limbs (5,7) and (7,9)
    pi, pd = ref.animal_primitives(PlaneCam(), x, s, pairs, radius, flags, 3)
    gone = [k for k, p in enumerate(pairs) if 7 in p]
    assert len(gone) == 2 and pi[7, 0] == 0
    assert [int(pi[J + 1 + k, 0]) for k in range(len(pairs))] == [0 if k in gone else 1 for k in range(len(pairs))]
    assert not pd[gone].any()
    for j in (5, 6):                                     # a NaN shoulder drops the neck and its five limbs
        x, s = pose((20.0, 15.0))
        x[j] = np.nan
        pi, _ = ref.animal_primitives(PlaneCam(), x, s, pairs, radius, flags, 3)
        assert pi[J, 0] == 0 and pi[j, 0] == 0
        assert all(pi[J + 1 + k, 0] == 0 for k, p in enumerate(pairs) if J in p or j in p)
        assert sum(int(pi[J + 1 + k, 0]) for k in range(len(pairs))) == len(pairs) - 6


@pytest.mark.parametrize("axis", [0, 1])
def test_gates_at_their_boundaries(axis):
    pairs, radius, flags = v1()
    for value, kept in ((3000.0, True), (np.nextafter(3000.0, 4000.0), False), (-1000.0, True),
                        (np.nextafter(-1000.0, -2000.0), False), (np.inf, False)):
        x, s = pose((20.0, 15.0))
        x[9, axis] = value
        pi, _ = ref.animal_primitives(PlaneCam(), x, s, pairs, radius, flags, 3)
        assert bool(pi[9, 0]) == kept, (axis, value)
        assert pi[10, 0] == 1


def test_negative_centre_truncates_toward_zero_and_borders_clip():
    pairs, radius, flags = v1()
    x, s = pose()
    x[9, :2] = (-2.7, -0.5)
    x[10, :2] = (41.9, 33.2)
    pi, _ = ref.animal_primitives(PlaneCam(), x, s, pairs, radius, flags, 3)
    assert pi[9, 1:4].tolist() == [-2, 0, 3] and pi[10, 1:4].tolist() == [41, 33, 3]
    # discs over all four borders and corners, a limb through the whole image: only inside pixels, all correct
    discs = [(-2, 0, 3), (41, 33, 3), (20, -1, 3), (20, 32, 3), (-1, 16, 3), (40, 16, 3)]
    img = ref.draw_image(BG, *table(discs=discs, limbs=[(-20.0, -10.0, 60.0, 45.0)]), J)
    want = np.zeros(BG.shape[:2], dtype=bool)
    ys, xs = np.mgrid[0:32, 0:40]
    for cx, cy, r in discs:
        want |= (xs - cx) ** 2 + (ys - cy) ** 2 <= r * r + r
    want |= ref.limb_mask(-20.0, -10.0, 60.0, 45.0, 3, np.arange(40), np.arange(32))
    assert np.array_equal(drawn(img), want)
    assert drawn(img)[0, 0] and drawn(img)[31, 39] and drawn(img)[0, 20] and drawn(img)[16, 0]


def test_skeleton_tables_match_the_reference_lists():
    from mqhip.overlay import JOINT_DISC, JOINT_NULLED, SKELETONS
    v1_pairs = [(0, 2), (0, 1), (2, 4), (1, 3), (6, 8), (5, 7), (8, 10), (7, 9), (12, 14), (11, 13), (14, 16),
                (13, 15), (0, 17), (17, 6), (17, 5), (17, 12), (17, 11)]
    v2_pairs = [(1, 2), (0, 1), (0, 2), (1, 3), (2, 4), (3, 4), (0, 17), (3, 17), (4, 17), (17, 5), (17, 6), (5, 6),
                (17, 11), (17, 12), (11, 12), (5, 7), (7, 9), (6, 8), (8, 10), (11, 13), (13, 15), (12, 14),
                (14, 16), (5, 11), (6, 12), (5, 12), (6, 11)]
    a, b = SKELETONS["v1"], SKELETONS["v2"]
    assert list(a.pairs) == v1_pairs and len(a.pairs) == 17
    assert list(b.pairs) == v2_pairs and len(b.pairs) == 27
    assert a.radius(3).tolist() == [3, 4, 4] + [3] * 15             # eyes mrksize + 1
    assert all(f == JOINT_DISC for f in a.flags)
    assert b.radius(3).tolist() == [3] * 18
    assert [f for f in b.flags] == [JOINT_DISC, JOINT_NULLED, JOINT_NULLED] + [JOINT_DISC] * 15
    # v2's clean_kp nulls the eyes: no eye disc, and none of the five limbs that end at an eye
    x, s = pose((20.0, 15.0))
    pi, _ = ref.animal_primitives(PlaneCam(), x, s, b.pairs, b.radius(3), b.flags, 3)
    assert pi[1, 0] == 0 and pi[2, 0] == 0 and pi[0, 0] == 1
    eye_limbs = [k for k, p in enumerate(v2_pairs) if 1 in p or 2 in p]
    assert len(eye_limbs) == 5
    assert [int(pi[J + 1 + k, 0]) for k in range(27)] == [0 if k in eye_limbs else 1 for k in range(27)]
    for sk in (a, b):
        assert J + 1 + len(sk.pairs) <= 64


def test_entry_points_are_bound():
    from mqhip import _lib
    for name in ("mq_overlay_primitives", "mq_overlay_render"):
        assert name in _lib.EXPORTED and name in _lib._SIGS
    assert len(_lib._SIGS["mq_overlay_primitives"][1]) == 17 and len(_lib._SIGS["mq_overlay_render"][1]) == 24
    assert _lib.ABI_VERSION == 8


def test_oversized_skeleton_is_rejected():
    from mqhip.overlay import Skeleton, check_skeleton
    big = Skeleton(pairs=tuple((0, 1) for _ in range(47)), radius_add=(0,) * 18, flags=(1,) * 18)
    with pytest.raises(ValueError):
        check_skeleton(big)
    ok = Skeleton(pairs=tuple((0, 1) for _ in range(46)), radius_add=(0,) * 18, flags=(1,) * 18)
    check_skeleton(ok, 8)
    with pytest.raises(ValueError):
        check_skeleton(ok, 9)


# ----------------------------------------------------------------------------- visualize_result.proc's file logic
N_FRAMES, H, W = 6, 48, 64


def _scene(tmp_path):
    from mqhip import io as mqio
    from mqhip import synth
    cams = synth.make_cameras(2)
    for c in cams:                                       # a small image: scale the projection to it
        c["K"] = np.asarray(c["K"], dtype=np.float64) * np.array([[W / 2048.0], [H / 1536.0], [1.0]])
    res = tmp_path / "results3D"
    rd = res / "clip"
    rd.mkdir(parents=True)
    synth.write_calibration_toml(cams, str(rd / "calibration.toml"))
    cfg = tmp_path / "config.yaml"
    with open(cfg, "w") as f:
        yaml.safe_dump({"camera_id": [int(c["name"]) for c in cams]}, f)
    skel = synth.make_skeletons(2, N_FRAMES, seed=3)     # (A, F, J, 3)
    score = np.ones(skel.shape[:3])
    raw = tmp_path / "videos"
    rng = np.random.default_rng(0)
    pool = rng.integers(0, 255, (2, H, W, 3), dtype=np.uint8)
    cam = str(cams[1]["name"])
    numbers = np.array([10, 11, 12, 14, 15, 16])         # frame 13 is not in the store
    mqio.write_frame_store(str(raw / f"clip.{cam}"), pool, 100.0 + numbers / 24.0, numbers,
                           [[] for _ in numbers], cam, frame_index=np.arange(len(numbers)) % 2)
    (rd / cam).mkdir()
    np.save(rd / cam / "frame_num.npy", np.array([10, 11, 12, 13, 14, 15], dtype=np.int32))
    return cams, str(res), str(cfg), str(raw), skel, score, pool, numbers


def test_proc_file_logic_with_the_oracle_renderer(tmp_path, capsys):
    from mqhip import io as mqio
    from mqhip.overlay import SKELETONS
    from src.pipeline import visualize_result as vis
    from src.pipeline import visualize_result_2 as vis2
    cams, res, cfg, raw, skel, score, pool, numbers = _scene(tmp_path)
    rd = os.path.join(res, "clip")
    out = str(tmp_path / "output")
    calls = []
    factory = ref.oracle_renderer_factory(os.path.join(rd, "calibration.toml"), calls)
    kw = dict(results_dir_root=res, out_dir=out, renderer=factory, batch=4)

    # no kp3d file: the early return, and nothing is written
    assert vis.proc("clip", 1, cfg, raw, **kw) is None
    assert "no kp3d file: clip" in capsys.readouterr().out and not os.path.exists(out)

    # kp3d_fxdJointLen.pickle is preferred over kp3d.pickle
    mqio.dump_pickle({"kp3d": np.full_like(skel, np.nan), "kp3d_score": score}, os.path.join(rd, "kp3d.pickle"))
    mqio.dump_pickle({"kp3d": skel, "kp3d_score": score}, os.path.join(rd, "kp3d_fxdJointLen.pickle"))
    cam = str(cams[1]["name"])
    path = vis.proc("clip", 1, cfg, raw, **kw)
    assert path == os.path.join(out, f"clip_{cam}")
    assert "[warning] Skipping frame 13" in capsys.readouterr().out
    store = mqio.FrameStore(path)
    kept = [0, 1, 2, 4, 5]                               # kp3d rows whose frame number the store has
    assert store.frame_number.tolist() == [10, 11, 12, 14, 15]
    np.testing.assert_array_equal(store.frame_time, 100.0 + np.array([10, 11, 12, 14, 15]) / 24.0)
    assert store.tracks == [[]] * 5 and store.frames.shape == (5, H, W, 3)
    sk = SKELETONS["v1"]
    src = np.array([0, 1, 0, 1, 0])                      # frame numbers 10, 11, 12, 14, 15 -> pool image
    want = ref.render(pool, [cams[1]], np.zeros(5, dtype=int), skel[:, kept].transpose(1, 0, 2, 3),
                      score[:, kept].transpose(1, 0, 2), sk.pairs, sk.radius(3), sk.flags, 3, src)
    assert np.array_equal(np.asarray(store.frames), want)
    assert (want != pool[src]).any(), "the scene draws nothing: the comparison would be empty"
    # the pool images of a batch are handed over once each: batches of 4 + 1 frames over a pool of 2
    assert [n for n, _ in calls] == [2, 1] and calls[0][1].tolist() == [0, 1, 0, 1]

    # already exists: the early return leaves the store alone
    before = os.path.getmtime(os.path.join(path, "frames.npy"))
    assert vis.proc("clip", 1, cfg, raw, **kw) is None
    assert "already exists:" in capsys.readouterr().out
    assert os.path.getmtime(os.path.join(path, "frames.npy")) == before

    # step / range bound the rows; visualize_result_2 draws its own skeleton
    out2 = str(tmp_path / "output2")
    path2 = vis2.proc("clip", 1, cfg, raw, results_dir_root=res, out_dir=out2, renderer=factory, step=2,
                      frame_range=(1, 6))
    store2 = mqio.FrameStore(path2)
    assert store2.frame_number.tolist() == [11, 15]      # rows 1, 3 (frame 13: skipped), 5
    sk2 = SKELETONS["v2"]
    want2 = ref.render(pool, [cams[1]], np.zeros(2, dtype=int), skel[:, [1, 5]].transpose(1, 0, 2, 3),
                       score[:, [1, 5]].transpose(1, 0, 2), sk2.pairs, sk2.radius(3), sk2.flags, 3, np.array([1, 0]))
    assert np.array_equal(np.asarray(store2.frames), want2)
    assert not np.array_equal(want2[0], want[1])


def test_frame_store_writer_refuses_a_short_store(tmp_path):
    from mqhip import io as mqio
    w = mqio.FrameStoreWriter(str(tmp_path / "s"), 2, 4, 6, 7)
    w.append(np.zeros((1, 4, 6, 3), dtype=np.uint8), [3], [0.5])
    with pytest.raises(ValueError):
        w.close()
    assert not os.path.exists(tmp_path / "s" / "metadata.yaml")
    with pytest.raises(ValueError):
        w.append(np.zeros((2, 4, 6, 3), dtype=np.uint8), [4, 5], [0.6, 0.7])
    w.append(np.ones((1, 4, 6, 3), dtype=np.uint8), [4], [0.6])
    w.close()
    s = mqio.FrameStore(str(tmp_path / "s"))
    assert s.frame_number.tolist() == [3, 4] and s.image(4).min() == 1
