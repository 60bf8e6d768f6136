"""CPU: the reference of the view calibration (tests/calib_ref.py), the golden file the GPU tests read, the entry
points' declarations, the host build of csrc/calib_dev.hpp under sanitizers, and the argument handling and file
round trip of multicam_toolbox.calibrate_intrinsic / get_extrinsic_from_cagekeypoints with the solve stubbed by
scipy (the GPU solve itself is tests/test_gpu_calib.py's)."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import calib_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "macaque-3d-pose-estimation_amd")
CSRC = os.path.join(PKG, "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", cr.GOLDEN)
if PKG not in sys.path:
    sys.path.insert(0, PKG)


@pytest.fixture(scope="module")
def golden():
    return cr.load_golden(GOLDEN)


# ----------------------------------------------------------------------------- scenes, starts, scipy
def test_golden_file_holds_the_seeded_scenes(golden):
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert set(golden) == set(cr.SCENES)
    for name in cr.SCENES:
        sc, d = cr.scene(name), golden[name]
        assert len(sc["obj"]) == len(d["obj"]) and d["model"] == sc["model"]
        for a, b in zip(sc["img"] + sc["obj"], d["img"] + d["obj"]):
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-9)      # libm's last bits may differ between hosts
        k0, p0, free = cr.scene_start(name, sc)
        np.testing.assert_allclose(k0, d["k0"], rtol=1e-9)
        np.testing.assert_allclose(p0, d["poses0"], rtol=1e-8, atol=1e-9)
        assert (free == d["free"]).all()
    w, h = cr.IMAGE_SIZE
    for name, d in golden.items():
        uv = np.concatenate(d["img"])
        assert uv[:, 0].min() > 0 and uv[:, 0].max() < w and uv[:, 1].min() > 0 and uv[:, 1].max() < h
    assert [len(o) for o in golden["pin_mixed"]["obj"]] == [65, 54, 54, 54]
    tz = np.concatenate([golden[n]["poses_true"][:, 5] for n in golden if n.startswith(("pin_V", "omni"))])
    assert tz.min() >= 450 and tz.max() <= 900
    for xi in (0.84, 2.0, 4.43):                                            # the true centre is the fixed one
        np.testing.assert_array_equal(golden[f"omni_xi{xi}"]["k_true"][3:5], [w / 2 - 0.5, h / 2 - 0.5])


@pytest.mark.parametrize("name", ["pin_V3_s0", "pin_V5_s1", "pin_mixed", "omni_xi2.0", "cage6", "plane4",
                                  "board_pose1"])
def test_scipy_costs_are_pinned(golden, name):
    """scipy's cost at the tight tolerance on the seeded scenes, pinned to 1e-6 relative by the golden file."""
    d = golden[name]
    k, poses, cost, res = cr.solve_scipy(d["model"], d["k0"], d["poses0"], d["obj"], d["img"], free_mask=d["free"],
                                         tol=cr.TIGHT)
    print(f"\n[{name}] cost {cost:.12e} golden {float(d['cost_tight']):.12e} nfev {res.nfev}")
    assert abs(cost - float(d["cost_tight"])) <= 1e-6 * float(d["cost_tight"])
    assert abs(cost - cr.cost(d["model"], k, poses, d["obj"], d["img"])) <= 1e-12 * cost
    assert float(d["cost_loose"]) >= float(d["cost_tight"]) * (1 - 1e-12)


def test_noise_free_recovery():
    """Known answers: without distortion Zhang's start is the camera itself; scipy recovers a distorted pinhole
    camera and the omnidir camera (xi = 2) from noise-free corners."""
    sc = cr.make_scene(cr.MODEL_PINHOLE, 5, 3, noise=0.0)
    k_plain = np.array([1800.0, 1750.0, 1023.5, 767.5, 0, 0, 0, 0, 0, 0])
    img = cr.project_views(cr.MODEL_PINHOLE, k_plain, sc["poses_true"], sc["obj"])
    k0, p0 = cr.init_numpy(cr.MODEL_PINHOLE, sc["obj"], img)
    np.testing.assert_allclose(k0, k_plain, rtol=1e-9, atol=1e-12)
    assert cr.rotation_distance(p0[:, :3], sc["poses_true"][:, :3]).max() < 1e-9
    np.testing.assert_allclose(p0[:, 3:], sc["poses_true"][:, 3:], rtol=1e-8, atol=1e-6)
    ko, _ = cr.init_numpy(cr.MODEL_OMNIDIR, sc["obj"], img)                 # the omnidir start: doubled f, xi = 1
    np.testing.assert_allclose(ko, [3600.0, 3500.0, 0, 1023.5, 767.5, 1, 0, 0, 0, 0], rtol=1e-9, atol=1e-12)
    k0, p0 = cr.init_numpy(cr.MODEL_PINHOLE, sc["obj"], sc["img"])
    k, poses, cost, _ = cr.solve_scipy(cr.MODEL_PINHOLE, k0, p0, sc["obj"], sc["img"])
    assert cost < 1e-18
    np.testing.assert_allclose(k, sc["k_true"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(poses, sc["poses_true"], rtol=1e-7, atol=1e-7)


def test_omnidir_noise_free_recovery(golden):
    d = golden["omni_clean"]
    assert float(d["cost_tight"]) < 1e-18
    np.testing.assert_allclose(d["k_tight"], d["k_true"], rtol=1e-8, atol=1e-10)


def test_fronto_parallel_start_is_an_error():
    o = cr.board_points()
    k = np.array([1800.0, 1800.0, 1023.5, 767.5, 0, 0, 0, 0, 0, 0])
    poses = np.array([[0, 0, 0.3 * v, -120.0 + 10 * v, -75.0, 500.0 + 60 * v] for v in range(1, 5)])
    img = cr.project_views(cr.MODEL_PINHOLE, k, poses, [o] * 4)
    with pytest.raises(ValueError, match="singular"):
        cr.init_numpy(cr.MODEL_PINHOLE, [o] * 4, img)


# ----------------------------------------------------------------------------- plumbing
def test_entry_points_are_declared_and_exported():
    from mqhip import _lib
    with open(os.path.join(ROOT, "include", "mq_hip.h")) as f:
        header = f.read()
    for name in ("mq_calib_init", "mq_calibrate_views"):
        assert name in _lib.EXPORTED and name in _lib._SIGS
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in include/mq_hip.h"
        assert len(m.group(1).split(",")) == len(_lib._SIGS[name][1])
    assert "multicam_toolbox.py:74-116" in header and ":213-242" in header
    assert "#define MQ_ABI_VERSION 8" in header and _lib.ABI_VERSION == 8       # purely additive
    lib = os.path.join(PKG, "lib", "libmq_hip.so")
    if os.path.exists(lib):
        import ctypes
        so = ctypes.CDLL(lib)
        assert hasattr(so, "mq_calib_init") and hasattr(so, "mq_calibrate_views")


def test_binding_constants_match_the_reference_calls():
    from mqhip import calib
    assert calib.DEFAULT_CRITERIA[calib.MODEL_OMNIDIR] == (200, 1e-8)                       # :111
    assert calib.DEFAULT_CRITERIA[calib.MODEL_PINHOLE] == (30, np.finfo(float).eps)
    assert [s for s, f in zip(calib.SLOTS[0], calib.DEFAULT_FREE[0]) if not f] == ["s", "cx", "cy"]   # :100
    assert sum(calib.DEFAULT_FREE[1]) == 9 and calib.DEFAULT_FREE[1][9] == 0
    assert (np.array(calib.DEFAULT_FREE[0], bool) == cr.DEFAULT_FREE[0]).all()
    assert (np.array(calib.DEFAULT_FREE[1], bool) == cr.DEFAULT_FREE[1]).all()
    k = np.arange(1.0, 11.0)
    mtx, dist = calib.pinhole_from_slots(k)
    assert mtx.shape == (3, 3) and dist.shape == (1, 5)
    np.testing.assert_array_equal(calib.pinhole_slots(mtx, dist)[:9], k[:9])
    K, xi, D = calib.omnidir_from_slots(k)
    assert K.shape == (3, 3) and xi.shape == (1, 1) and D.shape == (1, 4)
    assert K[0, 1] == 3.0 and K[0, 2] == 4.0 and K[1, 2] == 5.0 and xi[0, 0] == 6.0
    with pytest.raises(ValueError, match="fewer than 4"):
        calib._pack([np.zeros((3, 3))], [np.zeros((3, 2))], [1])
    with pytest.raises(ValueError, match="views_per_problem"):
        calib._pack([np.zeros((4, 3))], [np.zeros((4, 2))], [2])
    with pytest.raises(ValueError, match="at most 5"):
        calib.pinhole_slots(np.eye(3), np.zeros(8))


# ----------------------------------------------------------------------------- derivatives and closed forms
def test_jacobian_and_starts_on_the_host(tmp_path):
    """csrc/calib_dev.hpp compiles for the host: cal_obs_jac of both models against central differences (50 generic
    points, the optical axis, rvec = 0), rvec <-> R, Zhang's start and the DLT pose on known answers, under
    -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the derivative check needs a host C++ compiler"
    exe = str(tmp_path / "calib_jac_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, os.path.join(ROOT, "tests", "calib_jac_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count(" ok") == 5 and "runtime error" not in out.stderr
    worst = float(re.search(r"largest relative jacobian error (\S+)", out.stdout).group(1))
    assert worst < 1e-6


# ----------------------------------------------------------------------------- the reference's surface
class _WritableH5:
    """h5py.File(path, 'w') for the surface tests: collects create_dataset('/cam/name', data=...) into
    ``store[path]``."""

    def __init__(self, store, path):
        self._store, self._path = store, str(path)
        store[self._path] = {}

    def create_dataset(self, name, data):
        cam, key = name.strip("/").split("/")
        self._store[self._path].setdefault(cam, {})[key] = np.array(data)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class _Dataset:
    def __init__(self, a):
        self._a = np.asarray(a)

    def __getitem__(self, key):
        assert key == ()
        return self._a.copy()


class _ReadableH5:
    """``f[cam][name][()]`` for a group, ``f[cam][()]`` for a dataset directly under the camera's name (:227)."""

    def __init__(self, store, path):
        self._d = store[str(path)]

    def __getitem__(self, k):
        v = self._d[k]
        return {kk: _Dataset(vv) for kk, vv in v.items()} if isinstance(v, dict) else _Dataset(v)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _install_h5(monkeypatch, store):
    """tests/_fakes.py's h5py module with a File that also writes."""
    from _fakes import install_fake_h5py
    mod = install_fake_h5py(monkeypatch, store)
    mod.File = lambda path, mode="r": _WritableH5(store, path) if mode == "w" else _ReadableH5(store, path)
    return mod


def _scipy_calibrate_views(pose_starts=None):
    """A stand-in for mqhip.calib.calibrate_views with its signature and return layout, solved by calib_ref."""
    def stub(model, obj, img, views_per_problem, image_size, free_mask=None, intrinsics0=None, poses0=None,
             ftol=0.0, xtol=None, max_iter=None, return_residuals=False, device=0):
        ks, ps, rms, infos = [], [], [], []
        at = 0
        for p, V in enumerate(views_per_problem):
            o, i = obj[at:at + V], img[at:at + V]
            free = cr.DEFAULT_FREE[model] if free_mask is None else np.asarray(free_mask, bool).reshape(-1, 10)[-1]
            if intrinsics0 is None:
                k0, p0 = cr.init_numpy(model, o, i, image_size)
            else:
                k0 = np.asarray(intrinsics0)[p]
                p0 = pose_starts[at:at + V] if pose_starts is not None else cr.init_numpy(model, o, i, image_size)[1]
            k, poses, c, _ = cr.solve_scipy(model, k0, p0, o, i, free_mask=free, tol=1e-10)
            ks.append(k), ps.append(poses), rms.append(np.sqrt(2 * c / sum(len(x) for x in o))), infos.append({"cost": c})
            at += V
        return np.array(ks), np.concatenate(ps), np.array(rms), infos
    return stub


def _chessboards(n_cams=2, V=4):
    out, truth = {}, {}
    for c in range(n_cams):
        sc = cr.make_scene(cr.MODEL_OMNIDIR, V, 10 + c, noise=0.1)
        out[101 + c] = {"imp": np.stack(sc["img"])[:, :, None, :], "objp": np.stack(sc["obj"])}
        truth[101 + c] = sc
    return out, truth


def test_calibrate_intrinsic_arrays_in_arrays_out(monkeypatch):
    from mqhip import calib
    from src.utils import multicam_toolbox as mt
    monkeypatch.setattr(calib, "calibrate_views", _scipy_calibrate_views())
    boards, truth = _chessboards()
    cp, info = mt.calibrate_intrinsic("unused.yaml", chessboard_points=boards, img_size=cr.IMAGE_SIZE,
                                      return_info=True)
    assert cp["camera_id"] == [101, 102] and set(info) == {"pinhole", "omnidir"}
    for c in range(2):
        assert cp["mtx"][c].shape == (3, 3) and cp["dist"][c].shape == (1, 5)
        assert cp["K"][c].shape == (3, 3) and cp["xi"][c].shape == (1, 1) and cp["D"][c].shape == (1, 4)
        assert len(cp["view_rvecs"][c]) == 4 and cp["view_tvecs"][c][0].shape == (3, 1)
        np.testing.assert_array_equal(cp["idx"][c], [[0, 1, 2, 3]])
        assert cp["K"][c][0, 1] == 0.0 and tuple(cp["K"][c][:2, 2]) == (1023.5, 767.5)       # skew and centre frozen
        assert cp["rms"][c] < 0.2 and cp["rms_pinhole"][c] < 0.2                              # 0.1 px noise
    assert "rvecs" not in cp                          # the rig's extrinsics are get_extrinsic_from_cagekeypoints'
    # mtx_init / dist_init replace the closed-form pinhole start: the same minimum from a nearby start
    cp2 = mt.calibrate_intrinsic("unused.yaml", cp["mtx"][0] * [[1.01, 1, 1], [1, 0.99, 1], [1, 1, 1]], np.zeros(5),
                                 chessboard_points=boards, img_size=cr.IMAGE_SIZE)
    np.testing.assert_allclose(cp2["mtx"][0], cp["mtx"][0], rtol=1e-5)
    with pytest.raises(ValueError, match="img_size"):
        mt.calibrate_intrinsic("unused.yaml", chessboard_points=boards)
    with pytest.raises(ValueError, match="dist_init needs mtx_init"):
        mt.calibrate_intrinsic("unused.yaml", None, np.zeros(5), chessboard_points=boards, img_size=cr.IMAGE_SIZE)
    with pytest.raises(ValueError, match="imp must be"):
        mt.calibrate_intrinsic("unused.yaml", chessboard_points={1: {"imp": np.zeros((2, 54)), "objp": np.zeros((2, 54, 3))}},
                               img_size=cr.IMAGE_SIZE)


def test_without_arrays_and_without_h5py_the_functions_raise(monkeypatch):
    from src.utils import multicam_toolbox as mt
    monkeypatch.setitem(sys.modules, "h5py", None)                # import h5py -> ImportError
    with pytest.raises(NotImplementedError, match="needs h5py"):
        mt.calibrate_intrinsic("config.yaml")
    with pytest.raises(NotImplementedError, match="needs h5py"):
        mt.get_extrinsic_from_cagekeypoints("config.yaml")
    with pytest.raises(NotImplementedError, match="needs h5py"):
        mt.get_extrinsic_from_cagekeypoints("config.yaml", cagepoints={})     # camparam is missing
    for name in ("fix_extrinsic_optim", "label_cagekeypoints", "analyze_aruco_marker_vid"):
        assert not hasattr(mt, name)                              # what needs images or file surgery stays absent


def _cage_rows(k_pin, pose, seed):
    """(12, 6) annotation rows: flag, u, v on the 640-wide preview, X, Y, Z; two rows are flagged unused."""
    rng = np.random.default_rng(seed)
    o = np.array([[x, y, z] for x in (0, 1200.0) for y in (0, 900.0) for z in (0, 800.0)] +
                 [[600, 450, 0], [600, 0, 400.0], [0, 450, 400], [1200, 450, 400]])
    uv = cr.project(cr.MODEL_PINHOLE, k_pin, pose[None], o[None])[0] + 0.1 * rng.normal(size=(12, 2))
    rows = np.concatenate([np.ones((12, 1)), uv * 640 / 2048, o], axis=1)
    rows[[3, 9], 0] = 0
    rows[[3, 9], 1:3] = -1
    return rows


def test_h5_round_trip(monkeypatch, tmp_path, capsys):
    """chessboard_points.h5 -> cam_intrinsic.h5 -> (cagepoints_annotation.h5) -> cam_extrinsic.h5 through a stand-in
    h5py, in the shapes the reference writes (:90-116, :236-237)."""
    from mqhip import calib
    from mqhip.calib import pinhole_slots
    from src.utils import multicam_toolbox as mt
    base = str(tmp_path)
    cfg = os.path.join(base, "config.yaml")
    with open(cfg, "w") as f:
        f.write("camera_id: [101, 102]\nimg_size: [2048, 1536]\n")
    boards, _ = _chessboards()
    store = {os.path.join(base, "chessboard_points.h5"): {str(k): v for k, v in boards.items()}}
    _install_h5(monkeypatch, store)
    monkeypatch.setattr(calib, "calibrate_views", _scipy_calibrate_views())
    cp = mt.calibrate_intrinsic(cfg)
    intr = store[os.path.join(base, "cam_intrinsic.h5")]
    assert set(intr) == {"101", "102"} and set(intr["101"]) == {"mtx", "dist", "K", "xi", "D"}
    assert intr["102"]["dist"].shape == (1, 5) and intr["102"]["xi"].shape == (1, 1)
    np.testing.assert_array_equal(intr["101"]["K"], cp["K"][0])
    # cage annotations seen through the fitted pinhole cameras at known poses
    true = np.array([[0.3, -0.2, 0.1, -500.0, -400.0, 2600.0], [-0.2, 0.4, -0.1, -650.0, -380.0, 2900.0]])
    ks = [pinhole_slots(intr[c]["mtx"], intr[c]["dist"]) for c in ("101", "102")]
    store[os.path.join(base, "cagepoints_annotation.h5")] = {
        "101": _cage_rows(ks[0], true[0], 0), "102": _cage_rows(ks[1], true[1], 1)}
    monkeypatch.setattr(calib, "calibrate_views", _scipy_calibrate_views(pose_starts=true + 1e-3))
    out = mt.get_extrinsic_from_cagekeypoints(cfg)
    extr = store[os.path.join(base, "cam_extrinsic.h5")]
    assert extr["101"]["rvec"].shape == (3, 1) and extr["102"]["tvec"].shape == (3, 1)
    got = np.array([np.concatenate([np.ravel(r), np.ravel(t)]) for r, t in zip(out["rvecs"], out["tvecs"])])
    assert cr.rotation_distance(got[:, :3], true[:, :3]).max() < 1e-3 and np.abs(got[:, 3:] - true[:, 3:]).max() < 2.0
    assert "3D pos of camera 101" in capsys.readouterr().out
    assert out["camera_id"] == [101, 102] and "mtx" in out
    # the arrays-in path gives the same poses and writes nothing
    del store[os.path.join(base, "cam_extrinsic.h5")]
    rows = {101: _cage_rows(ks[0], true[0], 0), 102: _cage_rows(ks[1], true[1], 1)}
    out2 = mt.get_extrinsic_from_cagekeypoints(cfg, cagepoints=rows, camparam=cp)
    np.testing.assert_allclose(np.ravel(out2["rvecs"][1]), np.ravel(out["rvecs"][1]), rtol=1e-9)
    assert os.path.join(base, "cam_extrinsic.h5") not in store
    with pytest.raises(ValueError, match=r"\(n, 6\)"):
        mt.get_extrinsic_from_cagekeypoints(cfg, cagepoints={101: np.zeros((5, 5)), 102: rows[102]}, camparam=cp)
