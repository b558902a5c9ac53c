"""GPU: the fleet whose odometry drifts (UnknownEnvFleet(..., mapper=, drift_sigma=, matcher=ScanMatcher)).  The drift model
against its numpy replay over the device's own trajectory and readings (the match oracle and the map oracle per sample), bit for
bit; the plumbing against the plain mapped run; a graph run against an eager one.  The pose errors are printed, none is asserted:
whether the matcher helps is recorded in tests/golden/MAPPING_DRIFT.md, not tested."""
import numpy as np
import pytest

import map_oracle as M
import scan_match_cases as K
import scan_match_oracle as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

B, KMAX = 3, 12
START = np.array([[0.8, 0.65], [1.6, 0.7], [2.9, 0.9]])
GOAL = np.array([[3.2, 0.9], [1.6, 0.7], [1.0, 2.6]])       # the second robot stands on its goal: the stop rule stops it at once
MATCH = dict(clamp=8, min_score=10, min_gain=1)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _inputs(seed=5, sigma=0.04):
    st = np.zeros((B, 5)); st[:, 0] = START[:, 0]; st[:, 2] = START[:, 1]
    rng = np.random.default_rng(seed)
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
    return dict(st0=dev(st), goal=dev(GOAL), foot=torch.ones((B,), dtype=torch.int8, device="cuda"),
                noise=dev(0.01 * rng.standard_normal((KMAX, B, K.R, 2))), drift=dev(sigma * rng.standard_normal((KMAX, B, 2))))


def _fleet(per_robot=False, **kw):
    grid = lipmpc.GridMap(K.room(), K.ORIGIN, K.CELL)
    mapper = lipmpc.OccupancyMapper(K.W, K.H, K.ORIGIN, K.CELL, K.RANGE, K.R, per_robot=B if per_robot else None)
    # split_rays: the walls of a room are one cluster around the robot; cut into sectors of 40 degrees the robot can walk inside it
    return lipmpc.UnknownEnvFleet(grid=grid, N_horizon=3, lidar_range=K.RANGE, resolution=K.R, mapper=mapper, split_rays=10, **kw), mapper, grid


def _host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in r.items() if isinstance(v, torch.Tensor)}


def test_gpu_zero_drift_is_the_plain_mapped_run():
    """A run given an all-zero drift tensor takes the drift model's sample, and every number is the plain mapped run's."""
    i = _inputs()
    runs = {}
    for name, kw in (("plain", dict()), ("zero", dict(drift=torch.zeros_like(i["drift"])))):
        fleet, mapper, _ = _fleet()
        r = _host(fleet.run(i["st0"], i["goal"], i["foot"], KMAX, noise=i["noise"], **kw))
        runs[name] = dict(r, evidence=mapper.evidence.cpu().numpy().copy())
    for k in runs["plain"]:
        assert np.array_equal(_bits(runs["zero"][k]), _bits(runs["plain"][k])), k
    assert set(runs["zero"]) - set(runs["plain"]) == {"drift", "pose_error", "n_matched"}
    assert not runs["zero"]["drift"].any() and not runs["zero"]["pose_error"].any() and not runs["zero"]["n_matched"].any()
    print("plain: steps", runs["plain"]["n_steps"].tolist(), "status", runs["plain"]["last_status"].tolist())
    assert runs["plain"]["n_steps"].max() >= 6 and (runs["plain"]["evidence"] > 0).sum() > 50
    with pytest.raises(ValueError):
        lipmpc.UnknownEnvFleet(grid=_fleet()[2], lidar_range=K.RANGE, resolution=K.R, matcher=lipmpc.ScanMatcher(4, 4, **MATCH))
    with pytest.raises(ValueError):
        _fleet(matcher=lipmpc.ScanMatcher(4, 4, n_yaw=1, yaw_step=0.02, **MATCH))


def _replay(r, i, mapper, grid, matcher):
    """The drift model in numpy over the device's own X_pred: per sample the device's scan of X_pred[:, k] with noise[k] (what the
    captured sample read), then the match oracle and the map oracle."""
    X, n_steps = r["X_pred"], r["n_steps"]
    draws = i["drift"].cpu().numpy()
    sensor = lipmpc.LidarSensor.from_grid(grid, lidar_range=K.RANGE, resolution=K.R)
    per = mapper.per_robot is not None
    ev = np.zeros((B, K.W, K.H) if per else (K.W, K.H), np.int64)
    drift, n_matched, perr = np.zeros((B, 2)), np.zeros(B, np.int32), np.zeros((KMAX, B))
    table = lipmpc.ray_table(K.R)
    for k in range(KMAX):
        walking = (k <= n_steps).astype(np.int32)
        drift = drift + draws[k] * walking[:, None].astype(np.float64)
        st_k = torch.as_tensor(np.ascontiguousarray(X[:, k]), device="cuda")
        hits = sensor.sense(st_k, i["noise"][k], with_debug=True, c_eta=True)["hits"].cpu().numpy()
        bpos, bhits = X[:, k][:, (0, 2)] + drift, hits + drift[:, None, :]
        if matcher is not None:
            m = S.match(bpos, bhits, ev, K.ORIGIN, K.CELL, K.RANGE, mapper.depth, matcher.n_x, matcher.n_y, matcher.clamp,
                        matcher.min_score, matcher.min_gain, mask=walking)
            drift = drift + m["offset"]
            bpos, bhits = bpos + m["offset"], bhits + m["offset"][:, None, :]
            n_matched += m["matched"]
        M.update(ev, bpos, bhits, K.ORIGIN, K.CELL, K.RANGE, table, depth=mapper.depth, mask=walking)
        perr[k] = np.sqrt((drift * drift).sum(1))
    return dict(drift=drift, n_matched=n_matched, pose_error=perr, evidence=ev)


@pytest.mark.parametrize("case", ["matcher", "smear", "per_robot"])
def test_gpu_drift_model_equals_its_numpy_replay(case):
    """Given noise and drift tensors (sigma 0.04): drift, pose_error, n_matched and the final evidence, bit for bit.  ``smear``: no
    matcher, the drift goes into the map as it is."""
    i = _inputs()
    matcher = None if case == "smear" else lipmpc.ScanMatcher(4, 4, **MATCH)
    fleet, mapper, grid = _fleet(per_robot=case == "per_robot", matcher=matcher)
    r = _host(fleet.run(i["st0"], i["goal"], i["foot"], KMAX, noise=i["noise"], drift=i["drift"]))
    got_ev = mapper.evidence.cpu().numpy().copy()
    want = _replay(r, i, mapper, grid, matcher)
    print(case, "n_matched", r["n_matched"].tolist(), "final |drift|", r["pose_error"][-1].round(3).tolist(), "largest",
          r["pose_error"].max(0).round(3).tolist(), "sum of draws", np.abs(i["drift"].cpu().numpy().sum(0)).round(3).tolist())
    for name in ("drift", "pose_error", "n_matched"):
        assert np.array_equal(_bits(r[name]), _bits(want[name])), (name, r[name], want[name])
    assert np.array_equal(got_ev, want["evidence"]), int((got_ev != want["evidence"]).sum())
    assert r["n_steps"].max() >= 6 and r["drift"].any()
    if matcher is not None:
        assert r["n_matched"].sum() >= 1                      # the replay is no empty statement: offsets were accepted


def test_gpu_graph_run_equals_eager_run():
    i = _inputs(seed=6)
    runs = []
    for use_graph in (True, False, True):
        fleet, mapper, _ = _fleet(matcher=lipmpc.ScanMatcher(4, 4, **MATCH), drift_sigma=0.04)
        r = _host(fleet.run(i["st0"], i["goal"], i["foot"], KMAX, noise="seeded", noise_seed=3, drift="seeded", drift_seed=4, use_graph=use_graph))
        runs.append(dict(r, evidence=mapper.evidence.cpu().numpy().copy()))
    for other in runs[1:]:
        for k in runs[0]:
            assert np.array_equal(_bits(runs[0][k]), _bits(other[k])), k
    assert runs[0]["drift"].any() and runs[0]["pose_error"][-1].max() > 0.0


def test_gpu_exploring_with_drift_and_matcher_is_deterministic():
    i = _inputs()
    runs = []
    for _ in range(2):
        fleet, mapper, _ = _fleet(matcher=lipmpc.ScanMatcher(4, 4, **MATCH), drift_sigma=0.02)
        fleet.exploring_drift_seed = 1
        r = fleet.run_exploring(i["st0"], i["foot"], KMAX, lipmpc.FrontierPlanner(r_inflate=1, min_unknown=2), 4, 0.4, noise=i["noise"])
        n_replans = r["n_replans"]
        runs.append(dict(_host(r), evidence=mapper.evidence.cpu().numpy().copy()))
    assert n_replans == 3 and runs[0]["n_steps"].max() >= 4
    for k in runs[0]:
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), k
    print("exploring: steps", runs[0]["n_steps"].tolist(), "n_matched", runs[0]["n_matched"].tolist(), "pose error after each sample\n",
          runs[0]["pose_error"].round(3))
    assert runs[0]["pose_error"].shape == (KMAX, B) and runs[0]["drift"].any()
