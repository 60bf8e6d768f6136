"""CPU: the reference of ``CameraGroup.bundle_adjust`` / ``bundle_adjust_iter`` (tests/cg_ba_ref.py), the host
side of the new surface in mqhip.geometry (get_params / set_params, resample_points, get_error_dict, what raises),
the plumbing of ``mq_bundle_adjust_group`` and the derivative blocks of csrc/bundle_dev.hpp's mode 2 against
central differences (a stand-alone host program under the address and undefined-behaviour sanitizers).  The GPU
solve runs in tests/test_gpu_cg_bundle.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cg_ba_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "macaque-3d-pose-estimation_amd", "csrc")

# The scenes of tests/test_gpu_cg_bundle.py and scipy's final cost on them with the reference's call (ftol 1e-4,
# start = cg_ba_ref.start_params), measured once on the CPU: scipy converges on every one of them (status 2,
# ftol, after 4 evaluations; the cost falls from about 2e4 to 1/2 sigma^2 (m - n)).
SCENES = {
    "pinhole": (("pinhole",) * 3, 24, 0, False),
    "fisheye": (("fisheye",) * 4, 40, 0, False),
    "mixed": (("pinhole", "omnidir", "pinhole", "omnidir"), 40, 0, False),
    "pinhole_k2": (("pinhole",) * 4, 40, 0, True),
}
SCIPY_COST = {"pinhole": 5.235518, "fisheye": 15.008958, "mixed": 15.728846, "pinhole_k2": 14.615963}


def scene(name, **kw):
    models, N, seed, extra_dist = SCENES[name]
    return ref.make_scene(list(models), N, seed, extra_dist=extra_dist, **kw)


# ----------------------------------------------------------------------------- cameras
def _camera(cls, extra_dist):
    from mqhip import geometry as geo
    kw = dict(matrix=[[900.0, 2.0, 640.0], [0.0, 920.0, 512.0], [0.0, 0.0, 1.0]], rvec=[0.1, -0.2, 0.3],
              tvec=[10.0, 20.0, 1500.0], extra_dist=extra_dist)
    if cls == "Camera":
        return geo.Camera(dist=[0.05, 0.02, 1e-3, 2e-3, 5e-3], **kw)
    if cls == "FisheyeCamera":
        return geo.FisheyeCamera(dist=[0.05, 0.02, 1e-3, 2e-3], **kw)
    return geo.OmnidirCamera(dist=[0.05, 0.02, 1e-3, 2e-3], xi=[1.1], K=np.diag([1100.0, 1110.0, 1.0]),
                             D=[0.1, 0.01, 1e-3, 1e-3], **kw)


@pytest.mark.parametrize("extra_dist", [False, True])
@pytest.mark.parametrize("cls", ["Camera", "FisheyeCamera", "OmnidirCamera"])
def test_get_set_params_round_trip(cls, extra_dist):
    cam = _camera(cls, extra_dist)
    p = cam.get_params()
    want = [0.1, -0.2, 0.3, 10.0, 20.0, 1500.0, 910.0, 0.05] + ([0.02] if extra_dist else [])
    np.testing.assert_array_equal(p, want)                        # f = (fx + fy) / 2
    q = p.copy()
    q[:8] += [0.01, 0.02, 0.03, 1.0, 2.0, 3.0, 5.0, 0.001]
    cam.set_params(q)
    np.testing.assert_array_equal(cam.get_params(), q)
    m, d = cam.get_camera_matrix(), cam.get_distortions()
    assert m[0, 0] == m[1, 1] == q[6] and m[0, 1] == 2.0 and m[0, 2] == 640.0     # fx = fy = f, the rest kept
    assert d.size == (5 if cls == "Camera" else 4)
    np.testing.assert_array_equal(d[1:], [0.02 if extra_dist else 0.0] + [0.0] * (d.size - 2))   # the others zeroed
    np.testing.assert_array_equal(cam.get_rotation(), q[:3])
    np.testing.assert_array_equal(cam.get_translation(), q[3:6])
    if cls == "OmnidirCamera":                                    # what project() uses is not touched
        assert cam.get_K()[0, 0] == 1100.0 and cam.get_xi()[0] == 1.1 and cam.get_D()[0] == 0.1
    row = cam._group_fixed_row()
    assert row.shape == (11,) and row[0] == cam.model
    if cls == "OmnidirCamera":
        np.testing.assert_array_equal(row[1:], [1100.0, 0.0, 0.0, 1110.0, 0.0, 1.1, 0.1, 0.01, 1e-3, 1e-3])
    else:
        np.testing.assert_array_equal(row[1:], [640.0, 512.0] + [0.0] * 8)


def test_free_mask_follows_the_parametrisation():
    from mqhip.bundle import group_free_mask
    m = group_free_mask([1, 2, 0], False)
    assert m[:, :6].all() and m[:2, 6:8].all() and not m[:, 8].any() and not m[2, 6:].any()
    m = group_free_mask([1, 2, 0], True)
    assert m[:2].all() and m[2, :6].all() and not m[2, 6:].any()


def test_scene_group_matches_the_rows():
    """cg_ba_ref.camera_group builds the cameras the rows describe: get_params gives the rows back."""
    for name in SCENES:
        sc = scene(name)
        g = ref.camera_group(sc)
        np.testing.assert_array_equal(ref.group_params(g), sc["params"])
        np.testing.assert_array_equal(np.stack([c._group_fixed_row() for c in g.cameras]), sc["fixed"])


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", sorted(SCENES))
def test_scipy_reaches_the_recorded_cost(name):
    sc = scene(name)
    g = ref.ref_group(sc)
    res = g.bundle_adjust(sc["p2ds"], start_params=ref.start_params(sc))
    assert res.status > 0 and abs(res.cost - SCIPY_COST[name]) <= 1e-5 * SCIPY_COST[name], res.cost
    P = g.n_cam_params
    assert abs(ref.cost(sc, g.params, res.x[sc["C"] * P:].reshape(-1, 3)) - res.cost) <= 1e-12 * res.cost
    if name == "mixed":                                # scipy never moves an omnidir camera's f, k1
        np.testing.assert_array_equal(g.params[[1, 3], 6:], sc["params"][[1, 3], 6:])
        assert np.all(g.params[[0, 2], 6] != sc["params"][[0, 2], 6])
    if not sc["extra_dist"]:
        assert np.all(g.params[:, 8] == 0.0)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_restatement_converges_on_noise_free_scenes(name):
    sc = scene(name, noise=0.0)
    g = ref.ref_group(sc)
    res = g.bundle_adjust(sc["p2ds"], start_params=ref.start_params(sc), ftol=1e-12)
    assert res.cost < 1e-12 * ref.cost(sc, sc["params"], sc["pts"])
    rot, base = ref.gauge_distance(g.params, sc["params_true"])
    assert rot < 1e-6 and base < 1e-6


def test_jacobian_sparsity_covers_the_jacobian():
    sc = scene("mixed")
    g = ref.ref_group(sc)
    x0 = ref.start_params(sc)
    A = g.jac_sparsity(sc["p2ds"]).toarray()
    f0 = g.error_fun(x0.copy(), sc["p2ds"])
    assert A.shape == (f0.size, x0.size) and A.sum(axis=1).min() == 8 + 3
    for k in range(x0.size):
        x = x0.copy()
        x[k] += 1e-3 * max(1.0, abs(x[k]))
        moved = g.error_fun(x, sc["p2ds"]) != f0
        assert not np.any(moved & (A[:, k] == 0))
        if k < 32 and k % 8 >= 6 and (k // 8) % 2 == 1:            # an omnidir camera's f, k1: structurally zero
            assert not moved.any()


# ----------------------------------------------------------------------------- the helpers of bundle_adjust_iter
def _sparse_points(seed=3):
    """4 cameras x 60 points; cameras 2 and 3 share exactly 10 points, cameras 0 and 3 none."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 1000, (4, 60, 2))
    p[rng.uniform(size=(4, 60)) < 0.2] = np.nan
    p[3, :] = np.nan
    p[3, 40:50] = rng.uniform(0, 1000, (10, 2))
    p[2, 40:50] = rng.uniform(0, 1000, (10, 2))
    p[2, 50:] = np.nan
    p[0, 40:50] = np.nan
    return p


def test_resample_points_equals_the_reference_under_a_seed():
    from mqhip import geometry as geo
    p = _sparse_points()
    for n_samp in (5, 25, 1000):
        np.random.seed(11)
        want, want_next = ref.resample_points(p, n_samp), np.random.random()
        np.random.seed(11)
        (got, extra), got_next = geo.resample_points(p, None, n_samp=n_samp), np.random.random()
        assert extra is None and got.shape == want.shape and got.shape[1] > 0
        np.testing.assert_array_equal(got, want)
        assert got_next == want_next            # the two leave numpy's stream at the same place
    seen_by_a_pair = int((np.sum(~np.isnan(p[:, :, 0]), axis=0) >= 2).sum())
    assert geo.resample_points(p, n_samp=5)[0].shape[1] < seen_by_a_pair
    assert geo.resample_points(p, n_samp=1000)[0].shape[1] == seen_by_a_pair


def test_get_error_dict_equals_the_reference_and_drops_thin_pairs():
    from mqhip import geometry as geo
    p = _sparse_points()
    err = np.random.default_rng(5).normal(0, 2.0, p.shape)
    err[np.isnan(p)] = np.nan
    got, want = geo.get_error_dict(err), ref.get_error_dict(err)
    assert sorted(got) == sorted(want)
    assert (2, 3) not in got and (0, 3) not in got and (1, 3) not in got and (0, 1) in got      # <= 10 common points
    for k in want:
        assert got[k][0] == want[k][0]
        np.testing.assert_array_equal(got[k][1], want[k][1])
    n01 = int((~np.isnan(p[0, :, 0]) & ~np.isnan(p[1, :, 0])).sum())
    assert got[(0, 1)][0] == n01
    assert (2, 3) in geo.get_error_dict(err, min_points=9)


def test_subset_extra():
    from mqhip import geometry as geo
    assert geo.subset_extra(None, [1, 2]) is None
    extra = dict(objp=np.arange(12.0).reshape(4, 3), ids=np.arange(4), rvecs=np.zeros((2, 4, 3)),
                 tvecs=np.ones((2, 4, 3)))
    sub = geo.subset_extra(extra, [0, 2])
    assert sub["objp"].shape == (2, 3) and list(sub["ids"]) == [0, 2] and sub["rvecs"].shape == (2, 2, 3)


# ----------------------------------------------------------------------------- what raises (before any GPU call)
def test_unsupported_arguments_raise():
    sc = scene("pinhole")
    g = ref.camera_group(sc)
    with pytest.raises(NotImplementedError):
        g.bundle_adjust(sc["p2ds"], loss='huber', verbose=False)
    with pytest.raises(NotImplementedError):
        g.bundle_adjust(sc["p2ds"], extra={"ids": np.zeros(24)}, verbose=False)
    with pytest.raises(NotImplementedError):
        g.bundle_adjust_iter(sc["p2ds"], extra={"ids": np.zeros(24)})
    g.cameras[1].extra_dist = True
    with pytest.raises(ValueError, match="extra_dist"):
        g.bundle_adjust(sc["p2ds"], verbose=False)
    with pytest.raises(AssertionError):
        ref.camera_group(sc).bundle_adjust(sc["p2ds"][:2], verbose=False)


def test_shim_exports_the_surface():
    from src.third_party.aniposelib import cameras
    for name in ("get_error_dict", "check_errors", "subset_extra", "resample_points", "CameraGroup", "Camera"):
        assert name in cameras.__all__ and hasattr(cameras, name)
    for name in ("bundle_adjust", "bundle_adjust_iter"):
        assert callable(getattr(cameras.CameraGroup, name))
    for cls in (cameras.Camera, cameras.FisheyeCamera, cameras.OmnidirCamera):
        assert callable(cls.get_params) and callable(cls.set_params)


# ----------------------------------------------------------------------------- plumbing
def test_entry_point_is_declared_and_exported():
    from mqhip import _lib
    assert "mq_bundle_adjust_group" in _lib.EXPORTED and "mq_bundle_adjust_group" in _lib._SIGS
    with open(os.path.join(ROOT, "include", "mq_hip.h")) as f:
        header = f.read()
    m = re.search(r"int mq_bundle_adjust_group\(([^;]*)\);", header)
    assert m, "mq_bundle_adjust_group is not declared in include/mq_hip.h"
    assert len(m.group(1).split(",")) == len(_lib._SIGS["mq_bundle_adjust_group"][1])
    assert "cameras.py:894-980" in header
    assert "#define MQ_ABI_VERSION 8" in header and _lib.ABI_VERSION == 8       # purely additive
    lib = os.path.join(ROOT, "macaque-3d-pose-estimation_amd", "lib", "libmq_hip.so")
    if os.path.exists(lib):
        import ctypes
        assert hasattr(ctypes.CDLL(lib), "mq_bundle_adjust_group")


# ----------------------------------------------------------------------------- derivatives
def test_mode2_jacobian_against_central_differences(tmp_path):
    """ba_obs_jac<2> (csrc/bundle_dev.hpp compiles for the host) against central differences of ba_obs_res<2>, for
    each camera model, at generic points and on the optical axis (r -> 0), under -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the derivative check needs a host C++ compiler"
    exe = str(tmp_path / "cg_ba_jac_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cg_ba_jac_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count(" ok") == 3 and "runtime error" not in out.stderr
