"""GPU: step 3's tracking video -- the labelled overlay kernels (csrc/overlay.hip), the bilinear resize
(csrc/resize.hip) and ``step3.proc(save_vid=True)`` -- against the NumPy oracle tests/track_video_ref.py.  The
projection is bit-exact and every coverage and resize rule is in integers (or float32 in a fixed order), so tables
are compared field by field and images and JPEG streams byte for byte: nothing has a tolerance."""
import ctypes
import io
import os

import numpy as np
import pytest

import overlay_ref
import track_video_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

J = 17


def _skeleton(name="v1"):
    from mqhip.overlay import SKELETONS
    sk = SKELETONS[name]
    return sk.pairs, sk.radius(3), sk.flags


def _plane_camera(name="0"):
    """f = 1, c = 0, R = I, t = 0, no distortion: (X, Y, 1) projects to pixel (X, Y) exactly."""
    return dict(name=name, size=[200, 96], matrix=np.eye(3), distortions=np.zeros(5), rotation=np.zeros(3),
                translation=np.zeros(3), rvec=np.zeros(3), tvec=np.zeros(3), fisheye=False, omnidir=False)


def _renderer(H, W, cam=None):
    from mqhip.geometry import CameraGroup
    from mqhip.overlay import OverlayRenderer
    return OverlayRenderer(CameraGroup.from_dicts([cam or _plane_camera()]), H, W)


def _pose_at(x, y, spread=6.0, seed=0):
    """(J, 3) joints scattered over [x, x + spread] x [y, y + spread] with the minimum exactly at (x, y)."""
    rng = np.random.default_rng(seed)
    p = np.ones((J, 3))
    p[:, 0] = x + rng.uniform(0.5, spread, J)
    p[:, 1] = y + rng.uniform(0.5, spread, J)
    p[3, 0], p[8, 1] = x, y
    return p


def test_labelled_primitive_tables_match_the_oracle_field_by_field():
    from mqhip.overlay import label_tables
    B, A = 2, 5
    kp3d = np.ones((B, A, J, 3))
    for b in range(B):
        for a in range(A):
            kp3d[b, a] = _pose_at(20.0 + 30 * a, 15.0 + 10 * b, seed=10 * b + a)
    kp3d[0, 0] = _pose_at(-7.9, -3.2, seed=1)           # an origin at negative coordinates: (int) truncates to (-7, -3)
    kp3d[0, 1] = np.nan                                 # an all-NaN animal: no skeleton, no label
    kp3d[0, 2] = _pose_at(3000.25, 40.0, seed=2)        # x_min just over 3000: no label (and no joint inside the gates)
    kp3d[0, 4, :, 0] = np.nan                           # every x NaN, y fine: no label
    kp3d[1, 0, 2] = np.nan                              # one NaN joint is ignored by the minimum
    kp3d[1, 1] = _pose_at(3000.0, -1000.0, seed=3)      # exactly on both gates: labelled
    kp3d[1, 2] = _pose_at(10.0, 20.0, seed=4)
    kp3d[1, 2, 3, 0] = -1000.5                          # x_min just under -1000: no label, the other joints stay
    labels = [["0", "11", "7", None, "5"], ["23", "-1", "4", "888888", "9"]]       # label_n = 0 at [0][3]
    seg, n = label_tables(labels, B, A, 2.0, 5)
    pairs, radius, flags = _skeleton()
    cam = _plane_camera()
    want_i, want_d = ref.primitives([cam], np.zeros(B, dtype=int), kp3d, np.ones((B, A, J)), pairs, radius, flags, 3,
                                    seg, n, 5)
    lab = want_i[:, :, -1]
    assert lab[0, 0, :3].tolist() == [1, -7, -3] and lab[1, 1, :3].tolist() == [1, 3000, -1000]
    assert lab[:, :, 0].tolist() == [[1, 0, 0, 0, 0], [1, 1, 0, 1, 1]]           # the plants took
    assert want_i[1, 2, :J + 1, 0].sum() >= J - 1 and want_i[0, 2, :-1].sum() == 0
    got_i, got_d = _renderer(96, 200).primitives_labelled(0, kp3d, np.ones((B, A, J)), labels=labels)
    assert got_i.shape == want_i.shape == (B, A, J + 2 + len(pairs), 8) and got_d.shape == want_d.shape
    for f, field in enumerate(("valid", "cx", "cy", "r", "x0", "y0", "x1", "y1")):
        bad = np.argwhere(got_i[..., f] != want_i[..., f])
        assert len(bad) == 0, (field, bad[:4].tolist())
    assert np.array_equal(got_d, want_d)
    # without labels the label slot is all zero and the rest is mq_overlay_primitives' table
    plain_i, plain_d = _renderer(96, 200).primitives(0, kp3d, np.ones((B, A, J)))
    none_i, none_d = _renderer(96, 200).primitives_labelled(0, kp3d, np.ones((B, A, J)), colour=np.zeros((B, A)))
    assert np.array_equal(none_i[:, :, :-1], plain_i) and not none_i[:, :, -1].any() and np.array_equal(none_d, plain_d)


def _label_scene(H, W, seed):
    """Four animals: 0 with a label whose glyphs cross the corner of four tiles (pixel 85.3, row 32) and lie under
    animal 1's skeleton; 1 right over it; 2 with its label cut by the left and top borders; 3 elsewhere."""
    rng = np.random.default_rng(seed)
    B, A = 2, 4
    kp3d = np.ones((B, A, J, 3))
    kp3d[..., 0] = rng.uniform(-10.0, W + 10.0, (B, A, J))
    kp3d[..., 1] = rng.uniform(-10.0, H + 10.0, (B, A, J))
    fx, fy = min(1.0, W / 200.0), min(1.0, H / 96.0)
    kp3d[0, 0] = _pose_at(70.0 * fx, 52.0 * fy, spread=30.0, seed=seed + 1)     # label "47": x 70..150, y 10..52
    kp3d[0, 1] = _pose_at(72.0 * fx, 2.0, spread=50.0 * fy + 8, seed=seed + 2)  # its limbs cross animal 0's label
    kp3d[0, 2] = _pose_at(-9.6, 6.4, spread=25.0, seed=seed + 3)                # origin (-9, 6): cut left and top
    kp3d[0, 3] = _pose_at(W - 30.0, H - 8.0, spread=12.0, seed=seed + 4)        # runs off the right border
    labels = [["47", "3", "-8", "15"], ["0", None, "62", "9"]]
    colour = np.array([[2, -1, 0, 3], [3, 0, 7, 1]], dtype=np.int32)
    return kp3d, labels, colour


@pytest.mark.parametrize("H,W", [(96, 200), (33, 47), (96, 208)])
def test_labelled_draw_is_bit_exact(H, W):
    """96 x 200: rows of 600 bytes, three tile rows and 2.3 tile columns (a tile is 256 bytes x 32 rows), the byte
    path; 33 x 47: an odd pitch, two tile rows; 96 x 208: rows of 624 bytes, the 16-byte path."""
    import torch
    from mqhip.overlay import label_tables
    kp3d, labels, colour = _label_scene(H, W, seed=H + W)
    B, A = kp3d.shape[:2]
    score = np.ones((B, A, J))
    pool = np.random.default_rng(9).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    src = np.array([1, 0], dtype=np.int32)
    seg, n = label_tables(labels, B, A, 2.0, 5)
    pairs, radius, flags = _skeleton()
    cam = _plane_camera()
    args = ([cam], np.zeros(B, dtype=int), kp3d, score, pairs, radius, flags, 3, src)
    want = ref.render(pool, *args, colour, seg, n, 5)
    if (H, W) != (33, 47):
        # what the scene is for: animal 0's label crosses the tile corner, animal 1 paints over it, animal 2's is cut
        args0 = ([cam], [0], kp3d[:1, :1], score[:1, :1], pairs, radius, flags, 3, src[:1])
        only0 = ref.render(pool, *args0, colour[:1, :1], seg[:1, :1], n[:1, :1], 5)
        skel0 = ref.render(pool, *args0, colour[:1, :1], seg[:1, :1], n[:1, :1] * 0, 5)
        lab0 = (only0[0] != skel0[0]).any(axis=2)            # animal 0's label where its own skeleton is not
        assert lab0[:32, :85].any() and lab0[:32, 86:].any() and lab0[32:, :85].any() and lab0[32:, 86:].any()
        assert (lab0 & (want[0] == 0).all(axis=2)).any(), "animal 1 (black) does not cross animal 0's label"
        cut = ref.primitives(*args[:8], seg, n, 5)[0][0, 2, -1]
        assert cut[0] == 1 and cut[4] < 0 and cut[5] < 0 and (want[0][0, :40] == (255, 0, 0)).all(axis=1).any()
    r = _renderer(H, W)
    pool_d = torch.from_numpy(pool).cuda()
    got = r.render(pool_d, 0, kp3d, score, src_index=src, colour=colour, labels=labels).cpu().numpy()
    assert np.array_equal(pool_d.cpu().numpy(), pool), "the source pool was written"
    for b in range(B):
        bad = np.argwhere((got[b] != want[b]).any(axis=2))
        assert len(bad) == 0, (b, len(bad), bad[:5].tolist())
    # other stroke widths, even and odd, and another scale
    for t, scale in ((1, 1.0), (8, 1.5)):
        seg2, n2 = label_tables(labels, B, A, scale, t)
        want2 = ref.render(pool, *args, colour, seg2, n2, t)
        got2 = r.render(pool_d, 0, kp3d, score, src_index=src, colour=colour, labels=labels, label_scale=scale,
                        label_thickness=t).cpu().numpy()
        assert np.array_equal(got2, want2), (t, scale)


def test_unlabelled_render_is_unchanged_and_the_labelled_path_reduces_to_it():
    """test_gpu_overlay.py's border scene (H = 50, W = 94, a pool of 2 feeding 6 outputs): ``render`` without the
    new arguments equals the parent's composition (overlay_ref), and so does the labelled entry point with
    colour = animal index and no labels."""
    H, W, B, A = 50, 94, 6, 5
    rng = np.random.default_rng(5)
    pool = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    src = np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)
    kp3d = np.ones((B, A, J, 3))
    kp3d[..., 0] = rng.uniform(-12.0, W + 12.0, (B, A, J))
    kp3d[..., 1] = rng.uniform(-12.0, H + 12.0, (B, A, J))
    kp3d[0, 0, 0, :2] = (85.2, 31.7)
    kp3d[0, 1, 5, :2] = (-2.7, -1.2)
    kp3d[0, 1, 6, :2] = (95.9, 51.4)
    kp3d[1, 0, 7, :2] = (40.0, -3.0)
    kp3d[1, 0, 9, :2] = (40.0, 52.9)
    kp3d[1, 2, 8, :2] = (-3.0, 25.0)
    kp3d[1, 2, 10, :2] = (96.5, 25.0)
    kp3d[2, 3, 11, :2] = kp3d[2, 3, 13, :2]
    kp3d[3, :, :, 0] = 1e4
    kp3d[3, 2, :, 0] = rng.uniform(80.0, 92.0, J)
    score = np.ones((B, A, J))
    score[4] = 0.0
    pairs, radius, flags = _skeleton()
    cam = _plane_camera()
    want = overlay_ref.render(pool, [cam], np.zeros(B, dtype=int), kp3d, score, pairs, radius, flags, 3, src)
    r = _renderer(H, W)
    got = r.render(pool, 0, kp3d, score, src_index=src).cpu().numpy()
    assert np.array_equal(got, want)
    same = r.render(pool, 0, kp3d, score, src_index=src, colour=np.tile(np.arange(A), (B, 1))).cpu().numpy()
    assert np.array_equal(same, want)
    none = r.render(pool, 0, kp3d, score, src_index=src, labels=[[None] * A] * B).cpu().numpy()
    assert np.array_equal(none, want)


def test_nine_tracklets_in_two_passes_equal_one_composition():
    from mqhip.overlay import label_tables
    H, W, A = 64, 96, 9
    rng = np.random.default_rng(12)
    kp3d = np.ones((1, A, J, 3))
    for a in range(A):                                   # overlapping skeletons, so the order matters
        kp3d[0, a] = _pose_at(8.0 + 7 * a, 18.0 + 3 * (a % 3), spread=30.0, seed=a)
    colour = np.array([[0, 1, 2, 3, -1, 0, 1, 2, 3]], dtype=np.int32)
    labels = [[str(10 + a) for a in range(A)]]
    frame = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    pairs, radius, flags = _skeleton()
    seg, n = label_tables(labels, 1, A, 1.0, 3)
    want = ref.render(frame, [_plane_camera()], [0], kp3d, np.ones((1, A, J)), pairs, radius, flags, 3, None, colour,
                      seg, n, 3)
    last = ref.render(frame, [_plane_camera()], [0], kp3d[:, :8], np.ones((1, 8, J)), pairs, radius, flags, 3, None,
                      colour[:, :8], seg[:, :8], n[:, :8], 3)
    assert (want != last).any(), "the ninth tracklet draws nothing"
    r = _renderer(H, W)
    kw = dict(label_scale=1.0, label_thickness=3)
    with pytest.raises(ValueError):
        r.render(frame, 0, kp3d, np.ones((1, A, J)), colour=colour, labels=labels, **kw)
    one = r.render(frame, 0, kp3d[:, :8], np.ones((1, 8, J)), colour=colour[:, :8], labels=[labels[0][:8]], **kw)
    two = r.render(one, 0, kp3d[:, 8:], np.ones((1, 1, J)), colour=colour[:, 8:], labels=[labels[0][8:]], **kw)
    assert np.array_equal(two.cpu().numpy(), want)


@pytest.mark.parametrize("src,dst", [((48, 64), (19, 25)), ((37, 53), (16, 24)), ((20, 30), (40, 45)),
                                      ((16, 16), (16, 16)), ((1, 1), (3, 3)), ((40, 64), (30, 48))])
def test_resize_is_bit_exact(src, dst):
    """n = 3 images taken out of a pool of 6 with a stride of two images.  Source rows of 192 and 48 bytes take the
    dword loads, 159 / 90 / 3 the byte loads; output rows of 48 and 144 bytes the 16-byte stores."""
    import torch
    from mqhip.resize import resize_bilinear
    pool = np.random.default_rng(src[0] + dst[1]).integers(0, 256, (6, src[0], src[1], 3), dtype=np.uint8)
    want = ref.resize_bilinear(pool[::2], *dst)
    pool_d = torch.from_numpy(pool).cuda()
    view = pool_d[::2]
    assert view.stride(0) == 2 * src[0] * src[1] * 3
    got = resize_bilinear(view, *dst)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, dst[0], dst[1], 3)
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist())
    assert np.array_equal(pool_d.cpu().numpy(), pool)
    assert np.array_equal(resize_bilinear(pool[1:2], *dst).cpu().numpy(), ref.resize_bilinear(pool[1:2], *dst))
    if src == dst:
        assert np.array_equal(got, pool[::2])


def test_entry_points_reject_bad_arguments_without_writing():
    import torch
    from mqhip import _lib as L
    from mqhip.geometry import CameraGroup
    ctx = L.Context.get(0)
    lib = ctx.lib
    dev = torch.device("cuda", 0)
    cams = CameraGroup.from_dicts([_plane_camera()]).cams_tensor()
    pairs, radius, flags = _skeleton()
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32))
    radius = np.ascontiguousarray(radius, dtype=np.int32)
    flags = np.ascontiguousarray(np.asarray(flags, dtype=np.int32))
    P, H, W, A = len(pairs), 8, 16, 2
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    cam_d, kp, sc = z((1,), torch.int32), torch.ones((1, A, J, 3), dtype=torch.float64, device=dev), z((1, A, J), torch.float64)
    frames, src_d = z((1, H, W, 3), torch.uint8), z((1,), torch.int32)
    seg, n, col = z((1, A, 96, 4), torch.int32), z((1, A), torch.int32), z((1, A), torch.int32)
    prim_i, prim_d = z((1, A, J + 2 + P, 8), torch.int32), z((1, A, P, 4), torch.float64)
    out = torch.full((1, H, W, 3), 7, dtype=torch.uint8, device=dev)
    p, s = L.ptr, L.stream_ptr(dev)

    def render(S=96, t=5, seg_p=p(seg), n_p=p(n), frames_p=p(frames), out_p=p(out), A_=A, h=H):
        return lib.mq_overlay_render_labelled(
            ctx.handle, p(cams), 1, p(cam_d), p(kp), p(sc), 1, A_, J, pairs.ctypes.data, P, radius.ctypes.data,
            flags.ctypes.data, 3, frames_p, H * W * 3, 1, p(src_d), h, W, p(col), seg_p, n_p, S, t, p(prim_i),
            p(prim_d), out_p, s)

    def prims(S=96, t=5, seg_p=p(seg), n_p=p(n)):
        return lib.mq_overlay_primitives_labelled(
            ctx.handle, p(cams), 1, p(cam_d), p(kp), p(sc), 1, A, J, pairs.ctypes.data, P, radius.ctypes.data,
            flags.ctypes.data, 3, p(col), seg_p, n_p, S, t, p(prim_i), p(prim_d), s)

    for call in (render, prims):
        assert call(S=97) == -2 and call(S=-1) == -2
        assert call(t=0) == -2 and call(t=33) == -2
        assert call(seg_p=None) < 0 and call(n_p=None) < 0
        assert call(seg_p=ctypes.c_void_p(seg.data_ptr() + 4)) == -2          # not 16-byte aligned
    assert render(frames_p=None) < 0 and render(out_p=None) < 0 and render(A_=9) == -2 and render(h=0) == -2
    assert render(out_p=p(frames)) == -2                                      # in place
    torch.cuda.synchronize()
    assert int(prim_i.abs().sum()) == 0 and bool((out == 7).all()), "a rejected call wrote its outputs"
    assert render() == 0 and prims() == 0 and render(S=0, seg_p=None, n_p=None) == 0

    src_img = z((2, 6, 10, 3), torch.uint8)
    dst = torch.full((2, 4, 5, 3), 7, dtype=torch.uint8, device=dev)

    def resize(src_p=p(src_img), ss=180, n_=2, H_=6, W_=10, dst_p=p(dst), ds=60, h=4, w=5):
        return lib.mq_resize_bilinear(ctx.handle, src_p, ss, n_, H_, W_, dst_p, ds, h, w, s)

    for bad in (dict(H_=0), dict(W_=-1), dict(h=0), dict(w=0), dict(n_=-1), dict(n_=65536), dict(ss=179), dict(ds=59)):
        assert resize(**bad) == -2, bad
    assert resize(src_p=None) < 0 and resize(dst_p=None) < 0
    assert resize(dst_p=p(src_img), ds=180, h=6, w=10) == -2                  # overlap
    assert lib.mq_resize_bilinear(None, p(src_img), 180, 2, 6, 10, p(dst), 60, 4, 5, s) < 0
    torch.cuda.synchronize()
    assert bool((dst == 7).all()), "a rejected call wrote its output"
    assert resize(n_=0, src_p=None, dst_p=None) == 0 and resize() == 0
    torch.cuda.synchronize()
    assert bool((dst == 0).all())


# ----------------------------------------------------------------------------------------------- end to end
H, W, SIZE, VIS_CAM = 96, 128, (50, 38), 1


def test_proc_save_vid_end_to_end(tmp_path):
    """main_proc on the small scene, then the video of camera 1 at 50 x 38: every AVI frame equals the oracle chain
    (NumPy renderer -> NumPy resize -> jpeg_ref) fed with the joints the GPU lift returned (the lift itself is
    pinned by test_gpu_tracklets.py; feeding its own output keeps last-bit differences of the triangulation from
    flipping a truncated pixel)."""
    Image = pytest.importorskip("PIL.Image")
    from mqhip import io as mqio
    from mqhip.association import StepTwoCameras
    from mqhip.tracklets import TrackletLift
    from src.pipeline import step3_crossframematching as s3
    sc = ref.write_scene(tmp_path, ref.SMALL_RECIPE, H, W, VIS_CAM)
    lifts = []

    def lift(rows):
        lifts.append(ref.RecordingLift(TrackletLift(StepTwoCameras(sc["camparam"]), rows, 0)))
        return lifts[-1]
    name = sc["cams"][VIS_CAM]["name"]
    Trk, Cid, T = s3.proc("clip", os.path.dirname(sc["rd"]), sc["raw"], sc["cfg"], save_vid=True, save_vid_cam=VIS_CAM,
                          vidfile_prefix=str(tmp_path / "out" / "trk_"), n_animal=3, camparam=sc["camparam"],
                          size=SIZE, batch=5, lift=lift)
    assert len(Trk) >= 3 and os.path.exists(os.path.join(sc["rd"], "track.pickle"))
    path = str(tmp_path / "out" / f"trk_{name}.avi")
    assert sorted(os.listdir(tmp_path / "out")) == [f"trk_{name}.avi", f"trk_{name}.frame_number.npy",
                                                    f"trk_{name}.frame_time.npy"]
    n_frame = Trk[list(Trk)[0]].shape[0]
    rows = list(range(0, n_frame, 3))
    assert np.load(tmp_path / "out" / f"trk_{name}.frame_number.npy").tolist() == [100 + f for f in rows]
    assert len(lifts) == 1 and lifts[0].calls <= -(-len(rows) // 5), "one lift launch per batch"
    want = ref.oracle_video(sc["cams"][VIS_CAM], sc["pool"], Trk, Cid, lifts[0].p3d, SIZE)
    r = mqio.MjpegAviReader(path)
    assert len(r) == len(rows) and (r.height, r.width) == (SIZE[1], SIZE[0]) and r.fps == 24.0
    plain = [ref.jpeg_ref.encode(ref.resize_bilinear(sc["pool"][i], SIZE[1], SIZE[0]), 90, 16)[0] for i in (0, 1)]
    drawn = 0
    for i, (f, colours, labels, jpg) in enumerate(want):
        assert r.frame_bytes(i) == jpg, (i, f, labels)
        drawn += jpg != plain[f % 2]
        img = Image.open(io.BytesIO(r.frame_bytes(i)))
        assert img.size == SIZE and np.asarray(img.convert("RGB")).shape == (SIZE[1], SIZE[0], 3)
    assert drawn >= len(rows) // 2, "the video draws (almost) nothing"


def test_run_demo_step3_video(tmp_path, monkeypatch):
    """``run_demo.proc(association="match", step3_video=1, video_size=(80, 60))``: the chain of
    test_gpu_step3.py's clip hands step 3's rows to ``visualize`` with the documented options, and the video lands
    where the documentation says (the clip's random pose weights may link nobody: then no video is written)."""
    Image = pytest.importorskip("PIL.Image")
    import torch
    import run_demo
    from mqhip import io as mqio
    from mqhip import synth
    from mqhip.apis import PoseModelHip
    from mqhip.weights import VIT_TINY, make_random_weights
    cams, raw, res, cfg, truth = synth.write_clip(str(tmp_path), "clip", n_frames=40, n_views=4, n_animals=2)
    w = synth.confident_head(make_random_weights(VIT_TINY, seed=0, device=torch.device("cuda", 0)))
    pose = PoseModelHip(VIT_TINY, w, 0)
    out = str(tmp_path / "output")
    kw = dict(n_animal=2, pose_model=pose, id_model="random", out_dir=out, step3_video=1, video_size=(80, 60))
    with pytest.raises(ValueError):
        run_demo.proc("clip", 24, res, "cuda:0", cfg, raw, 17, **kw)          # the known assignment has no tracklets
    from src.pipeline import step3_crossframematching as s3
    calls, real = [], s3.visualize

    def spy(*a, **k):
        calls.append((a, k))
        return real(*a, **k)
    monkeypatch.setattr(s3, "visualize", spy)
    run_demo.proc("clip", 24, res, "cuda:0", cfg, raw, 17, association="match", **kw)
    assert len(calls) == 1
    (vis_cam, cfg_path, result_dir, raw_dir), opts = calls[0]
    assert vis_cam == 1 and cfg_path == cfg and result_dir == res + "/clip" and raw_dir == raw
    assert opts["size"] == (80, 60) and opts["fps"] == 24.0 and opts["quality"] == 90 and opts["device"] == 0
    assert opts["vidfile_prefix"] == os.path.join(out, "clip_track_") and len(opts["T"]) == 4
    name = cams[1]["name"]
    Trk = mqio.load_array_pickle(os.path.join(res, "clip", "track.pickle"))
    print("tracklets:", len(Trk))
    if not Trk:         # the clip's keyframes link nobody (test_gpu_step3.py allows for it): no video is written
        assert not os.path.exists(out)
        return
    assert sorted(os.listdir(out)) == [f"clip_track_{name}.avi", f"clip_track_{name}.frame_number.npy",
                                       f"clip_track_{name}.frame_time.npy"]
    n_frame = Trk[list(Trk)[0]].shape[0]
    r = mqio.MjpegAviReader(os.path.join(out, f"clip_track_{name}.avi"))
    assert len(r) == len(range(0, n_frame, 3)) and (r.height, r.width) == (60, 80) and r.fps == 24.0
    frame_num = np.load(os.path.join(res, "clip", str(name), "frame_num.npy"))
    assert np.load(os.path.join(out, f"clip_track_{name}.frame_number.npy")).tolist() == \
        [int(frame_num[f]) for f in range(0, n_frame, 3)]
    for i in range(len(r)):
        assert Image.open(io.BytesIO(r.frame_bytes(i))).size == (80, 60)
