"""Step 3's host stages (tracklets, trimming, ID votes, stitching, clean-up) on the CPU, with the 3D traces
and ID votes injected from the oracle's per-cell lift (``step3_scenes.OracleLift``) through the stages' only
seam, against the recorded runs of the reference (tests/golden/step3_scene_*.npz, written by
tests/golden/make_step3_golden.py): integers exactly, graph weights to 1e-6, kp2d bit for bit."""
import numpy as np
import pytest

import step3_scenes as scenes

SCENES = sorted(scenes.RECIPES)


@pytest.fixture(scope="module")
def runs():
    """Per scene: the fixture and one run of the host stages on the oracle lift."""
    from mqhip import synth
    from src.pipeline import step3_crossframematching as s3
    out = {}
    for name in SCENES:
        fx = scenes.load_fixture(name)
        cams, T, keyframes = scenes.build_scene(fx["recipe"])
        camparam = synth.camparam_from_cams(cams)
        digest = scenes.scene_digest(T, keyframes)
        rec = {}
        Trk, Cid, T2, C, n_frame = s3.run_stages(T, keyframes, fx["recipe"]["n_cam"],
                                                 lambda rows: scenes.OracleLift(camparam, rows), record=rec)
        out[name] = dict(fx=fx, Trk=Trk, Cid=Cid, T2=T2, C=C, rec=rec, digest=digest)
    return out


def _same_tracks(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"tracklet {k}")


@pytest.mark.parametrize("name", SCENES)
def test_fixture_inputs_match_the_recipe(runs, name):
    assert scenes.RECIPES[name] == runs[name]["fx"]["recipe"]
    assert runs[name]["digest"] == runs[name]["fx"]["digest"], "the scene generator drifted from the fixture"


@pytest.mark.parametrize("name", SCENES)
def test_final_tracks_ids_and_connections(runs, name):
    r = runs[name]
    _same_tracks(r["Trk"], r["fx"]["trk_final"])
    _same_tracks(r["Cid"], r["fx"]["cid_final"])
    assert [[[int(p), int(q)] for p, q in c] for c in r["C"]] == r["fx"]["connection"]


@pytest.mark.parametrize("name", SCENES)
def test_intermediates(runs, name):
    r, fx = runs[name], runs[name]["fx"]
    _same_tracks(r["rec"]["trk_tracklets"], fx["trk_tracklets"])
    _same_tracks(r["rec"]["trk_trimmed"], fx["trk_trimmed"])
    _same_tracks(r["rec"]["cid_first"], fx["cid_first"])
    _same_tracks(r["rec"]["cid_second"], fx["cid_second"])
    np.testing.assert_allclose([x[2] for x in r["rec"]["trim_rmse"]], fx["trim_rmse"], rtol=0, atol=1e-6)
    g = r["rec"]["graph"]
    assert g.shape == fx["graph"].shape
    np.testing.assert_array_equal(g[:, :2], fx["graph"][:, :2])
    np.testing.assert_allclose(g[:, 2], fx["graph"][:, 2], rtol=0, atol=1e-6)
    assert r["rec"]["paths"] == fx["paths"]


@pytest.mark.parametrize("name", SCENES)
def test_kp2d_is_the_writer_on_the_fixture_tracks(runs, name):
    from src.pipeline import step3_crossframematching as s3
    r = runs[name]
    want = s3.assemble_kp2d(r["T2"], r["fx"]["trk_final"], r["fx"]["cid_final"])
    got = s3.assemble_kp2d(r["T2"], r["Trk"], r["Cid"])
    assert got.tobytes() == want.tobytes()
    assert np.nansum(np.abs(got), axis=(2, 3, 4)).astype(bool).sum() > 100      # kp2d holds NaN keypoints


@pytest.mark.parametrize("name", SCENES)
def test_calc_flow_on_the_recorded_graphs(runs, name):
    from src.pipeline.step3_crossframematching import calc_flow
    fx = runs[name]["fx"]
    assert len(fx["graph"]) > 0
    assert calc_flow(fx["graph"]) == fx["paths"]


# ----------------------------------------------------------------------------- calc_flow vs networkx

def _nx_solve(nx, nodes, links, n_track, skip=None):
    """The reference's network for one n_track, built here: (cost, flow dict) or None when infeasible."""
    G = nx.DiGraph()
    G.add_node("s", demand=-n_track)
    G.add_node("t", demand=n_track)
    for k in nodes:
        G.add_node(("in", k), demand=1)
        G.add_node(("out", k), demand=-1)
        for u, v, w in ((("in", k), ("out", k), 0), ("s", ("in", k), 100000), (("out", k), "t", 100000)):
            if (u, v) != skip:
                G.add_edge(u, v, capacity=1, weight=w)
    for (a, b), w in links.items():
        if (("out", a), ("in", b)) != skip:
            G.add_edge(("out", a), ("in", b), capacity=1, weight=w)
    try:
        return nx.min_cost_flow_cost(G), nx.min_cost_flow(G)
    except nx.NetworkXUnfeasible:
        return None


def _nx_reference(nx, g):
    """calc_flow's contract restated on networkx: sweep n_track in 1 .. n-1, reject an optimum with two units
    through a node, keep the cheapest (first on ties).  Also reports whether any n_track was rejected and
    whether every optimum of the sweep is unique (no used link or IN->OUT arc can be removed at equal cost;
    all link weights here are >= 1, so two optima always differ in such an arc)."""
    nodes = [int(k) for k in np.unique(g[:, :2])]
    links = {(int(a), int(b)): int(d * 100.0) for a, b, d in g}
    best, best_cost, rejected, unique, costs = None, 10 ** 8, False, True, {}
    for n_track in range(1, len(nodes)):
        res = _nx_solve(nx, nodes, links, n_track)
        if res is None:
            continue
        cost, flow = res
        costs[n_track] = cost
        used = [(u, v) for u in flow for v, f in flow[u].items() if f and u != "s" and v != "t"]
        for e in used:
            alt = _nx_solve(nx, nodes, links, n_track, skip=e)
            if alt is not None and alt[0] == cost:
                unique = False
        doubled = any(flow[("in", k)].get(("out", k), 0) for k in nodes)
        # the reference counts unit flows into IN_k and out of OUT_k; more than one of either is this arc
        assert doubled == any(sum(flow[u].get(("in", k), 0) for u in flow) > 1 for k in nodes)
        if doubled:
            rejected = True
            continue
        if cost < best_cost:
            best, best_cost = flow, cost
    paths = []
    if best is not None:
        for k in nodes:
            if best["s"].get(("in", k), 0):
                path = [k]
                while True:
                    nxt = [v[1] for v, f in best[("out", path[-1])].items() if f and v != "t"]
                    if not nxt:
                        break
                    path.append(nxt[0])
                paths.append(path)
    return paths, best_cost, rejected, unique, costs


def test_calc_flow_matches_a_networkx_formulation():
    nx = pytest.importorskip("networkx")
    from src.pipeline.step3_crossframematching import calc_flow, flow_sweep
    rng = np.random.default_rng(7)
    n_rejected = n_nonunique = 0
    for _ in range(200):
        n = int(rng.integers(2, 9))
        keys = np.sort(rng.choice(40, size=n, replace=False))
        g = [[keys[i], keys[j], rng.uniform(0.01, 300.0)] for i in range(n) for j in range(i + 1, n)
             if rng.random() < 0.45]
        if not g:
            g = [[keys[0], keys[1], rng.uniform(0.01, 300.0)]]
        g = np.array(g)
        paths, cost, rejected, unique, costs = _nx_reference(nx, g)
        n_rejected += rejected
        n_nonunique += not unique
        sweep = flow_sweep(g)
        assert {t: c for t, c, _, _ in sweep} == costs           # demands and the n_track sweep
        if unique:
            assert calc_flow(g) == paths
            accepted = [c for _, c, ok, _ in sweep if ok]
            assert min(accepted) == cost
    assert n_rejected > 0, "the draw never exercised the two-units rejection"
    assert n_nonunique <= 40, "more than 20 % of the draw has a non-unique optimum"


# ----------------------------------------------------------------------------- small known answers

def test_to_intv_known_answer():
    from src.pipeline.step3_crossframematching import to_intv
    np.testing.assert_array_equal(to_intv([0, 1, 1, 0, 0, 1, 0]), [[1, 3], [5, 6]])
    np.testing.assert_array_equal(to_intv([1, 1, 0, 1]), [[0, 2], [3, 4]])
    assert to_intv([0, 0, 0]).shape == (0, 2)


def test_set_id_known_answer():
    from src.pipeline.step3_crossframematching import set_id_for_each_frame_of_tracklets
    n_frame, wsize = 60, 20
    trk = {5: np.zeros((n_frame, 2), dtype=int), 6: np.zeros((n_frame, 2), dtype=int),
           7: np.zeros((n_frame, 2), dtype=int)}
    votes = {k: np.zeros((n_frame, 4), dtype=int) for k in trk}
    votes[5][0:25, 1] = 1           # class 1 early, class 3 late: cut midway between the last / first votes
    votes[5][35:60, 3] = 1
    votes[6][:, 2] = 1              # one class throughout
    votes[7][3:9, 0] = 1            # 6 votes: below the 12 a window or the whole tracklet needs
    cid = set_id_for_each_frame_of_tracklets(trk, votes, n_frame, wsize)
    np.testing.assert_array_equal(cid[6], np.full(n_frame, 2))
    np.testing.assert_array_equal(cid[7], np.full(n_frame, -1))
    # windows of 20 frames: class 1 is decisive (>= 12 votes, > 80 %) for centres 10..23, class 3 for 37..49;
    # last class-1 vote at frame 24, first class-3 vote at 35 -> cut at 24 + int(11 / 2) = 29
    np.testing.assert_array_equal(cid[5], np.r_[np.full(29, 1), np.full(31, 3)])


def test_div_3dtracklet_known_answer():
    from src.pipeline.step3_crossframematching import div_3dtracklet
    n_frame = 12
    trk = np.full((n_frame, 3), -1)
    trk[2:11] = [[4, 5, 6]] * 9
    cid = np.r_[np.full(6, 0), np.full(6, 2)]
    Trk, Cid, info = div_3dtracklet({3: trk.copy(), 9: trk.copy()}, {3: cid.copy(), 9: np.full(n_frame, 1)},
                                    {3: [[2, 4], [7, 10]]})
    assert sorted(Trk) == [9, 10, 11]           # 3 is split (labels 0 | 2 inside [2, 10)), 9 stays
    # a run [a, b) of equal labels becomes the piece a .. b inclusive, as in the reference
    np.testing.assert_array_equal(np.nonzero((Trk[10] >= 0).any(axis=1))[0], np.arange(2, 7))
    np.testing.assert_array_equal(np.nonzero((Trk[11] >= 0).any(axis=1))[0], np.arange(6, 11))
    np.testing.assert_array_equal(Cid[10], np.r_[np.full(2, -1), np.full(5, 0), np.full(5, -1)])
    np.testing.assert_array_equal(Cid[11], np.r_[np.full(6, -1), np.full(5, 2), np.full(1, -1)])
    assert info[10] == [[2, 4]] and info[11] == [[7, 10]]


def test_exports_carry_the_tracklet_entry_points():
    from mqhip import _lib
    assert "mq_tracklet_traces" in _lib.EXPORTED and "mq_tracklet_id_votes" in _lib.EXPORTED
    assert "mq_tracklet_traces" in _lib._SIGS and "mq_tracklet_id_votes" in _lib._SIGS
