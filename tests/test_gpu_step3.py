"""GPU: step 3's ``main_proc`` (host stages on the mq_tracklet_* kernels) on the recorded scenes of the
reference (tests/golden/step3_scene_*.npz), and ``run_demo.proc(association="match")`` end to end."""
import json
import os
import pickle

import numpy as np
import pytest
import yaml

import step3_scenes as scenes
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]


@pytest.mark.parametrize("name", sorted(scenes.RECIPES))
def test_main_proc_reproduces_the_reference(tmp_path, name):
    from mqhip import io as mqio
    from mqhip import synth
    from src.pipeline import step3_crossframematching as s3
    fx = scenes.load_fixture(name)
    cams, T, keyframes = scenes.build_scene(fx["recipe"])
    assert scenes.scene_digest(T, keyframes) == fx["digest"], "the scene generator drifted from the fixture"
    rd = tmp_path / "res"
    cfg = tmp_path / "config.yaml"
    with open(cfg, "w") as f:
        yaml.safe_dump({"camera_id": [int(c["name"]) for c in cams]}, f)
    for c, cam in enumerate(cams):
        (rd / str(cam["name"])).mkdir(parents=True)
        with open(rd / str(cam["name"]) / "alldata.json", "w") as f:
            json.dump(T[c], f)
    with open(rd / "match_keyframe.pickle", "wb") as f:
        pickle.dump(keyframes, f)
    Trk, Cid, T2 = s3.main_proc(str(cfg), str(rd), camparam=synth.camparam_from_cams(cams))
    assert sorted(Trk) == sorted(fx["trk_final"]) and sorted(Cid) == sorted(fx["cid_final"])
    for k in Trk:
        np.testing.assert_array_equal(Trk[k], fx["trk_final"][k], err_msg=f"Trk[{k}]")
        np.testing.assert_array_equal(Cid[k], fx["cid_final"][k], err_msg=f"Cid[{k}]")
    for fn in ("kp2d.pickle", "track.pickle", "collar_id.pickle", "keyframe_connection.pickle"):
        assert (rd / fn).exists(), fn
    conn = mqio.load_array_pickle(str(rd / "keyframe_connection.pickle"))
    assert [[[int(p), int(q)] for p, q in c] for c in conn] == fx["connection"]
    # kp2d.pickle is the writer's array on the fixture's tracks (what the host test checks on the CPU)
    want = s3.assemble_kp2d(T2, fx["trk_final"], fx["cid_final"])
    got = mqio.load_array_pickle(str(rd / "kp2d.pickle"))
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


def test_calc_3dpose_and_calc_3dtrace_match_the_oracle():
    """The two per-pose entry points of the reference's surface: calc_3dpose (threshold 0.3) through the
    undistort + pinv-DLT launches, calc_3dtrace through the tracklet kernel."""
    from mqhip import synth
    from mqhip.association import StepTwoCameras
    from mqhip.tracklets import TrackletLift
    from oracle.association import calc_3dpose as oracle_pose
    from src.pipeline import step3_crossframematching as s3
    cams = synth.make_cameras(8)
    T = synth.make_alldata(cams, synth.make_skeletons(2, 8, seed=5), seed=6)
    camparam = synth.camparam_from_cams(cams)
    stc = StepTwoCameras(camparam)
    ref = scenes.OracleLift(camparam, T)
    trk = np.zeros((8, 8), dtype=int)                    # individual 0's box id in every camera
    trk[6:] = -1
    kp = np.full((8, 17, 3), np.nan)
    for c in range(8):
        for tt in T[c][2]:
            if tt[0] == 0:
                kp[c] = np.array(tt[5])
    want = oracle_pose(kp, camparam, thr_kp=0.3)
    got = s3.calc_3dpose(kp, camparam=stc)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isfinite(want).any()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6, equal_nan=True)
    frames = np.array([1, 2, 5, 7])
    trace = s3.calc_3dtrace(TrackletLift(stc, T), trk, frames)
    want = np.full((8, 3), np.nan)
    want[frames] = ref.traces({0: trk}, np.stack([np.zeros(4, dtype=int), frames], axis=1))[0]
    assert np.isnan(trace[7]).all() and np.isfinite(trace[[1, 2, 5]]).all()
    assert np.array_equal(np.isnan(trace), np.isnan(want))
    np.testing.assert_allclose(trace, want, rtol=0, atol=1e-6, equal_nan=True)


def test_run_demo_with_matching(tmp_path):
    """A 40-frame clip (step 2 has the keyframes 1, 13, 25), 4 views, 2 animals through steps 1-2-3-4."""
    import torch
    import run_demo
    from mqhip import io as mqio
    from mqhip import synth
    from mqhip.apis import PoseModelHip
    from mqhip.weights import VIT_TINY, make_random_weights
    n_frames, n_views, n_animals = 40, 4, 2
    cams, raw, res, cfg, truth = synth.write_clip(str(tmp_path), "clip", n_frames=n_frames, n_views=n_views,
                                                  n_animals=n_animals)
    w = synth.confident_head(make_random_weights(VIT_TINY, seed=0, device=torch.device("cuda", 0)))
    pose = PoseModelHip(VIT_TINY, w, 0)
    data = run_demo.proc("clip", 24, res, "cuda:0", cfg, raw, 17, n_animal=n_animals, pose_model=pose,
                         id_model="random", association="match")
    rd = os.path.join(res, "clip")
    assert os.path.exists(os.path.join(rd, "match_keyframe.pickle"))
    assert os.path.exists(os.path.join(rd, "track.pickle"))
    keyframes = mqio.load_array_pickle(os.path.join(rd, "match_keyframe.pickle"))
    assert [k["frame"] for k in keyframes] == [1, 13, 25]
    kp2d = mqio.load_array_pickle(os.path.join(rd, "kp2d.pickle"))
    n_frame = keyframes[-1]["frame"]                 # step 3 takes the clip length from the last keyframe
    assert kp2d.shape == (n_animals, n_frame, n_views, 17, 3)
    assert data["kp3d"].shape == (n_animals, n_frame, 17, 3)
    Cid = mqio.load_array_pickle(os.path.join(rd, "collar_id.pickle"))
    if all((c < 0).all() for c in Cid.values()):
        # the clip's ID scores leave every tracklet unassigned: nobody is written
        assert not kp2d.any()
    else:
        assert np.nansum(np.abs(kp2d)) > 0
