"""GPU: the chessboard-corner detector (mq_chess_response, mq_chess_candidates, mq_chess_grid, mq_corner_subpix,
mq_find_chessboard; csrc/chessboard.hip) against the numpy restatement tests/chessboard_ref.py on rendered views.

The response, the candidates and the grid are integer or index-valued: equality.  The refinement is float64 summed in
another order than numpy's: within 2e-3 px at criteria (30, 1e-3), since two correct summation orders may stop one
iteration apart, each within eps of the fixed point; the difference at criteria (100, 1e-9) is printed."""
import os
import sys

import numpy as np
import pytest

import chessboard_ref as cr
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "macaque-3d-pose-estimation_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

SUBPIX_TOL = 2e-3
SUBPIX_CAP = 0.5


def _np(t):
    return t.cpu().numpy()


# ----------------------------------------------------------------------------- 2. response
def test_response_equals_the_restatement():
    """333 x 241: no multiple of the 64 x 16 tile, several blocks each way; a board crop and an all-equal image."""
    from mqhip import chessboard
    gray = np.stack([cr.make_view("frontal")[0][100:341, 150:483], np.full((241, 333), 77, np.uint8)])
    got = _np(chessboard.response(gray))
    assert got.dtype == np.int32 and got.shape == (2, 241, 333)
    want = np.stack([cr.chess_response(g) for g in gray])
    assert (got == want).all()
    assert want[0].max() > 3000 and (got[1] == 0).all()
    border = np.ones((241, 333), bool)
    border[5:-5, 5:-5] = False
    assert (got[0][border] == 0).all() and (got[0][~border] > 0).any()


# ----------------------------------------------------------------------------- 3. candidates
def _resp_cases():
    rng = np.random.default_rng(3)
    noise = rng.integers(1, 1_000_000, size=(200, 300)).astype(np.int32)      # several hundred 9 x 9 maxima
    flat = np.zeros((200, 300), np.int32)
    tied = np.zeros((200, 300), np.int32)
    patch = rng.integers(1, 5000, size=(30, 40)).astype(np.int32)
    for y, x in ((10, 20), (10, 200), (120, 20), (150, 230)):                  # the same maxima four times
        tied[y:y + 30, x:x + 40] = patch
    plateau = np.full((200, 300), 7, np.int32)                                 # every pixel equals its maximum
    return {"noise": noise, "flat": flat, "tied": tied, "plateau": plateau}


@pytest.mark.parametrize("K", (256, 100, 7))
def test_candidates_equal_the_restatement(K):
    """More survivors than K (noise, and a plateau where every pixel survives and only the position bits of the key
    decide), none (flat), and tied responses (a patch pasted four times): positions, responses and counts equal the
    restatement's first K under (R descending, y ascending, x ascending)."""
    from mqhip import chessboard
    cases = _resp_cases()
    resp = np.stack(list(cases.values()))
    pos, val, cnt = (_np(t) for t in chessboard.candidates(resp, K))
    for i, (name, r) in enumerate(cases.items()):
        wp, wv, wn = cr.chess_candidates(r, K)
        assert cnt[i] == wn, name
        assert (pos[i] == wp).all() and (val[i] == wv).all(), name
    total = {name: cr.chess_candidates(r, 100000)[2] for name, r in cases.items()}
    assert total["noise"] > 256 and total["plateau"] == 200 * 300 and total["flat"] == 0
    assert cnt[1] == 0 and cnt[3] == K and (pos[3][:K, 1] == 0).all()
    if K == 7:
        assert len(set(val[2][:4].tolist())) == 1, "the tie must straddle the cut"


# ----------------------------------------------------------------------------- 4-5. grid
def _chain(grays, K=256, scale=1.0):
    from mqhip import chessboard
    pos, val, cnt = chessboard.candidates(chessboard.response(np.stack(grays)), K)
    found, corners, index = chessboard.grid(pos, val, cnt, scale)
    return _np(pos), _np(val), _np(cnt), found, corners, index


@pytest.mark.parametrize("names", (("frontal", "empty", "rot170", "cut"), ("small_a", "small_cut", "small_b", "empty320")))
def test_grid_equals_the_restatement(names):
    """Batches of four: two boards, a frame without a board and a board cut by the edge, at 640 x 480 and at
    320 x 240 (spacing 16-19 px, where the gate on weak maxima matters).  Found flags, candidate indices and corner
    positions equal the restatement."""
    grays = [cr.make_empty() if n == "empty" else cr.make_empty(320, 240, 12) if n == "empty320" else cr.make_view(n)[0]
             for n in names]
    pos, val, cnt, found, corners, index = _chain(grays)
    assert found.tolist() == [True, False, True, False]
    for i, g in enumerate(grays):
        wp, wv, wn = cr.chess_candidates(cr.chess_response(g), 256)
        assert cnt[i] == wn and (pos[i] == wp).all() and (val[i] == wv).all()
        wf, wc, wi, _ = cr.chess_grid(wp, wv, wn, 1.0)
        assert found[i] == wf and (index[i] == wi).all()
        assert np.array_equal(corners[i], wc, equal_nan=True)
        if wf:
            truth = cr.make_view(names[i])[1]
            assert np.linalg.norm(corners[i] - truth, axis=1).max() <= 1.0


# ----------------------------------------------------------------------------- 6. cornerSubPix
def _subpix_cases():
    frontal, ft, _ = cr.make_view("frontal")
    small, st, _ = cr.make_view("small_b")
    edge, et = cr.subpix_edge_case()
    return [("frontal w 11", frontal, np.rint(ft), 11), ("w 11 wider than the 16 px spacing", small, np.rint(st), 11),
            ("starts 6 px off, w 5: resets", small, np.rint(st[:18]) + 6.0, 5),
            ("corner 3 px from the edge, w 11", edge, np.rint(et[[0, 1, 9, 10]]), 11),
            ("corner 3 px from the edge, w 5", edge, np.rint(et[[0, 1, 9, 10]]), 5)]


def test_corner_subpix_matches_the_restatement():
    """Within 2e-3 px at criteria (30, 1e-3), reset corners exactly at their start.  At criteria (100, 1e-9) the
    difference is printed (measured: see DESIGN.md section 8.14)."""
    from mqhip import chessboard
    resets = 0
    for name, gray, start, win in _subpix_cases():
        got = chessboard.corner_subpix(gray, start, win, (30, 1e-3))
        want = cr.corner_subpix(gray, start, win, (30, 1e-3))
        d = np.abs(got - want).max()
        tight = np.abs(chessboard.corner_subpix(gray, start, win, (100, 1e-9)) -
                       cr.corner_subpix(gray, start, win, (100, 1e-9))).max()
        print(f"{name}: kernel against the restatement {d:.3g} px at (30, 1e-3), {tight:.3g} px at (100, 1e-9)")
        assert d <= SUBPIX_TOL, name
        back = (want == start).all(axis=1)
        assert ((got == start).all(axis=1) == back).all(), name
        resets += int(back.sum())
    assert resets > 0
    edge = _subpix_cases()[3]
    assert edge[2][0].tolist() == [3.0, 3.0]
    nan = chessboard.corner_subpix(edge[1], np.array([[np.nan, 5.0], [3.0, 3.0]]), 5)
    assert np.isnan(nan[0, 0]) and nan[0, 1] == 5.0 and np.isfinite(nan[1]).all()      # a NaN corner is left alone


def test_empty_batches():
    from mqhip import chessboard
    assert tuple(chessboard.response(np.zeros((0, 24, 32), np.uint8)).shape) == (0, 24, 32)
    pos, val, cnt = chessboard.candidates(np.zeros((0, 24, 32), np.int32), 64)
    assert tuple(pos.shape) == (0, 64, 2) and tuple(cnt.shape) == (0,)
    found, corners, index = chessboard.grid(pos, val, cnt)
    assert found.shape == (0,) and corners.shape == (0, 54, 2) and index.shape == (0, 54)
    assert chessboard.corner_subpix(np.zeros((0, 24, 32), np.uint8), np.zeros((0, 54, 2))).shape == (0, 54, 2)
    assert chessboard.corner_subpix(np.zeros((24, 32), np.uint8), np.zeros((0, 2))).shape == (0, 2)
    found, corners = chessboard.find_chessboard_corners(np.zeros((0, 48, 64, 3), np.uint8))
    assert found.shape == (0,) and corners.shape == (0, 54, 2)


# ----------------------------------------------------------------------------- the chain
def test_find_chessboard_at_half_scale():
    """One 1280 x 960 frame, detected at scale 0.5 and refined at full size, through mq_find_chessboard: the
    restatement's corners within 2e-3 px, the analytic corners within the 0.5 px cap; gray and BGR input agree."""
    from mqhip import chessboard
    gray, truth, win = cr.make_view("big")
    found, corners, info = chessboard.find_chessboard_corners(gray[None], win=win, return_info=True)
    assert info["scale"] == 0.5 and found.tolist() == [True]
    wf, wc = cr.find_chessboard(gray, None, win, (30, 1e-3))
    assert wf
    d = np.abs(corners[0] - wc).max()
    err = np.linalg.norm(corners[0] - truth, axis=1)
    print(f"big: kernel against the restatement {d:.3g} px; against the truth max {err.max():.3f} rms "
          f"{np.sqrt((err ** 2).mean()):.3f} px")
    assert d <= SUBPIX_TOL and err.max() <= SUBPIX_CAP
    bgr = np.repeat(gray[None, :, :, None], 3, axis=3)
    f2, c2 = chessboard.find_chessboard_corners(bgr, win=win)
    assert f2.tolist() == [True] and np.array_equal(c2, corners)
    f3, c3 = chessboard.find_chessboard_corners(np.stack([cr.make_empty(), cr.make_view("frontal")[0]]))
    assert f3.tolist() == [False, True] and np.isnan(c3[0]).all() and np.isfinite(c3[1]).all()


def test_detected_views_calibrate_the_camera():
    """Eight rendered 640 x 480 views -> analyze_chessboardvid(stores=...) -> calibrate_intrinsic: the pinhole fit
    converges with rms <= 0.5 px (a mirrored or mis-ordered view gives tens of px).  The recovered focal length is
    printed against the renderer's 520 (measured: see DESIGN.md section 8.14)."""
    from src.utils import multicam_toolbox as mt
    frames, truth, f = cr.calibration_views()
    pad = np.zeros((10,) + frames[0].shape, np.uint8)                 # the reference starts at frame 10
    pts = mt.analyze_chessboardvid(None, frame_intv=1, stores={"cam0": np.concatenate([pad, np.stack(frames)])},
                                   square_size=1.0)
    imp, objp = pts["cam0"]["imp"], pts["cam0"]["objp"]
    assert imp.shape == (8, 54, 1, 2) and imp.dtype == np.float32 and objp.shape == (8, 54, 3)
    assert objp.dtype == np.float64 and (objp[3] == mt.chessboard_objp(1.0)).all()
    err = np.linalg.norm(imp[:, :, 0, :] - np.stack(truth), axis=2)
    assert err.max() <= SUBPIX_CAP
    cam = mt.calibrate_intrinsic(None, chessboard_points=pts, img_size=(640, 480))
    fx, fy = cam["mtx"][0][0, 0], cam["mtx"][0][1, 1]
    print(f"corners max {err.max():.3f} px; pinhole rms {cam['rms_pinhole'][0]:.3f} px, omnidir rms {cam['rms'][0]:.3f} "
          f"px; fx {fx:.2f} fy {fy:.2f} against {f} ({100 * (fx / f - 1):+.2f} %, {100 * (fy / f - 1):+.2f} %)")
    assert cam["rms_pinhole"][0] <= 0.5


def test_analyze_chessboardvid_reads_the_configs_frame_store(tmp_path):
    """The reference's call: camera ids, square size and the video folder come from the config; the camera's frame
    store (a pool of three images behind a frame index) is read at frames range(10, n, frame_intv)."""
    import yaml

    from mqhip.io import write_frame_store
    from src.utils import multicam_toolbox as mt
    pool = np.stack([cr.make_view("small_a")[0], cr.make_view("small_b")[0], cr.make_empty(320, 240, 12)])
    pool = np.repeat(pool[..., None], 3, axis=3)
    index = [2] * 10 + [0, 1, 2, 1, 0, 2, 0]                     # frames 10, 12, 14, 16 show views 0, 2, 0, 0
    n = len(index)
    write_frame_store(str(tmp_path / "chess" / "7.store"), pool, np.arange(n) / 24.0, np.arange(n), [[]] * n, 7,
                      frame_index=index)
    cfg = tmp_path / "config.yaml"
    cfg.write_text(yaml.safe_dump({"camera_id": [7], "chessboard_square_size": 30.0, "chessboard_vid_folder": "chess",
                                   "img_size": [320, 240]}))
    pts = mt.analyze_chessboardvid(str(cfg), frame_intv=2, win=5, batch=3)
    shown = [index[k] for k in range(10, n, 2)]                  # 0, 2, 0, 0
    assert shown == [0, 2, 0, 0]
    imp, objp = pts[7]["imp"], pts[7]["objp"]
    assert imp.shape == (3, 54, 1, 2) and objp.shape == (3, 54, 3) and objp[0, 1, 0] == 30.0
    truth = cr.make_view("small_a")[1]
    assert np.linalg.norm(imp[:, :, 0, :] - truth[None], axis=2).max() <= SUBPIX_CAP
    assert (imp[0] == imp[1]).all()
