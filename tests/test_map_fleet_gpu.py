"""GPU: the fleet that maps what it sees (UnknownEnvFleet(..., mapper=OccupancyMapper)) and re-plans on its map
(run_replanning).  The evidence of a mapped run against the map oracle replayed over the device's own trajectory and readings
(no closed-loop divergence can enter); the loop itself against the same run without a mapper, bit for bit."""
import numpy as np
import pytest

import grid_lidar_oracle as G
import map_oracle as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402


def _states(pos):
    st = np.zeros((len(pos), 5)); st[:, 0] = pos[:, 0]; st[:, 2] = pos[:, 1]
    return torch.as_tensor(st, device="cuda")


def test_gpu_mapped_run_leaves_the_robots_alone():
    """B = 16, k_max = 12, given noise, on the grid-scan fixture: X_pred / U_pred / n_steps / last_status equal the run without
    a mapper bit for bit; the final evidence equals the oracle replayed over X_pred with the device's own readings (the scan of
    X_pred[:, k] with noise[k]: what the captured sample handed to the update), robots masked once they have stopped."""
    fx = G.fixture()
    grid = lipmpc.GridMap(fx["occ"], fx["origin"], fx["cell"])
    B, K = 16, 12
    st0 = _states(fx["pos"][:B])
    goal = torch.tensor([[8.0, 8.0]] * B, dtype=torch.float64, device="cuda")
    foot = torch.ones((B,), dtype=torch.int8, device="cuda")
    noise = 0.01 * torch.randn((K, B, 360, 2), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    W, H, ev_origin, cell = 150, 140, (-0.3, 0.2), (0.05, 0.05)
    mapper = lipmpc.OccupancyMapper(W, H, ev_origin, cell, 1.5)
    mapper.evidence.fill_(5)                                 # a run adds to what the mapper holds; the warm-up sample adds nothing
    runs = {}
    for name, kw in (("mapped", dict(mapper=mapper)), ("plain", dict())):
        fleet = lipmpc.UnknownEnvFleet(grid=grid, N_horizon=3, lidar_range=1.5, **kw)
        r = fleet.run(st0, goal, foot, K, noise=noise)
        torch.cuda.synchronize()
        runs[name] = {k: v.cpu().numpy().copy() for k, v in r.items()}
    for k in runs["plain"]:
        assert np.array_equal(runs["mapped"][k].view(np.int64 if runs["plain"][k].dtype == np.float64 else runs["plain"][k].dtype),
                              runs["plain"][k].view(np.int64 if runs["plain"][k].dtype == np.float64 else runs["plain"][k].dtype)), k
    X, n_steps = runs["mapped"]["X_pred"], runs["mapped"]["n_steps"]
    assert n_steps.max() >= 5
    sensor = lipmpc.LidarSensor.from_grid(grid, lidar_range=1.5)
    want = np.full((W, H), 5, np.int64)
    table = lipmpc.ray_table(360)
    for k in range(K):
        st_k = torch.as_tensor(np.ascontiguousarray(X[:, k]), device="cuda")
        hits = sensor.sense(st_k, noise[k], with_debug=True, c_eta=True)["hits"].cpu().numpy()
        M.update(want, X[:, k][:, (0, 2)], hits, ev_origin, cell, 1.5, table, mask=(k <= n_steps).astype(np.int32))
    got = mapper.evidence.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    print(f"evidence: {int((got > 5).sum())} cells above, {int((got < 5).sum())} below their start; robots stopped early: {int((n_steps < K).sum())}")
    assert (got > 5).sum() > 100 and (got < 5).sum() > 5000
    with pytest.raises(ValueError):
        lipmpc.UnknownEnvFleet(grid=grid, lidar_range=1.5, mapper=lipmpc.OccupancyMapper(W, H, ev_origin, cell, 2.0))
    with pytest.raises(ValueError):
        fleet.run_replanning(st0, goal, foot, K, lipmpc.RrtStarPlanner(n=50), 4, 0.5)      # (a fleet without a mapper)


def test_gpu_goal_selection_equals_the_oracle_rule():
    from importlib import import_module
    select = import_module(lipmpc.UnknownEnvFleet.__module__).select_working_goals
    rng = np.random.default_rng(4)
    B, S = 64, 9
    pos, goal, sub = rng.uniform(0, 3, (B, 2)), rng.uniform(0, 3, (B, 2)), rng.uniform(0, 3, (B, S, 2))
    n_sub, status = rng.integers(0, S + 1, B), rng.choice([0, 0, 0, 1, 5, 7], B)
    sub[0, 0] = pos[0] + (0.3, 0.4)                          # (sqrt(0.09 + 0.16) against 0.5: the boundary case, whichever way it rounds)
    n_sub[0], status[0] = 3, 0
    dev = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device="cuda")
    for look in (0.0, 0.5, 1.5, 10.0):
        got = select(dev(pos), dev(goal), dev(sub), dev(n_sub, torch.int32), dev(status, torch.int32), look).cpu().numpy()
        assert np.array_equal(got, M.select_goals(pos, goal, sub, n_sub, status, look)), look


def test_gpu_run_replanning_follows_the_rule():
    """A short replanning run on the fixture: the plans are made on the mapper's map every ``replan_every`` samples, the working
    goals are the oracle rule's choice from the last plan at the positions it was made from, and robots keep walking."""
    fx = G.fixture()
    grid = lipmpc.GridMap(fx["occ"], fx["origin"], fx["cell"])
    B, K = 8, 12
    st0 = _states(fx["pos"][:B])
    goal = torch.tensor([[8.0, 8.0]] * B, dtype=torch.float64, device="cuda")
    foot = torch.ones((B,), dtype=torch.int8, device="cuda")
    noise = 0.01 * torch.randn((K, B, 360, 2), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    mapper = lipmpc.OccupancyMapper(128, 128, (-1.0, -1.0), 0.08, 1.5, per_robot=B)
    planner = lipmpc.RrtStarPlanner(n=200, r_rewire=30, seed=2, max_cells=1 << 14)
    fleet = lipmpc.UnknownEnvFleet(grid=grid, N_horizon=3, lidar_range=1.5, mapper=mapper)
    r = fleet.run_replanning(st0, goal, foot, K, planner, replan_every=4, lookahead=0.6, noise=noise)
    torch.cuda.synchronize()
    assert r["n_replans"] == 3 and tuple(r["rrt_status"].shape) == (B,)
    status = r["rrt_status"].cpu().numpy()
    assert set(status.tolist()) <= {0, 1, 2, 3, 5}, status
    last = planner.last
    X = r["X_pred"].cpu().numpy()
    want = M.select_goals(X[:, 8][:, (0, 2)], goal.cpu().numpy(), last["sub_goals"].cpu().numpy(), last["n_sub"].cpu().numpy(), status, 0.6)
    assert np.array_equal(r["working_goal"].cpu().numpy(), want)
    assert (status == 0).any() and not np.array_equal(want, goal.cpu().numpy())
    assert r["n_steps"].max().item() >= 5 and int(mapper.evidence.abs().sum()) > 0


def test_gpu_dead_end_needs_the_map():
    """The U-shaped wall of tests/golden/mapped_replanning.npz (chosen on the CPU by make_mapped_replanning.py, reasoning in
    MAPPED_REPLANNING.md), the recorded noise seeds as one batch, every robot with its own map: the reactive loop alone arrives
    for none of them; with run_replanning at most one seed misses (device and CPU chains may part at a flipped cell; the CPU
    chain itself misses none)."""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mapped_replanning.npz"))
    seeds, K = d["seeds"].tolist(), int(d["k_max"])
    B = len(seeds)
    assert B >= 8 and K <= 120 and d["plain_arrived"].sum() == 0 and d["replanning_arrived"].all()
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"]), tuple(d["cell"])
    occ = np.zeros((W, H), np.uint8)
    for i0, j0, i1, j1 in d["walls"]:
        occ[i0:i1, j0:j1] = 1
    grid = lipmpc.GridMap(occ, origin, cell)
    rng_range = float(d["lidar_range"])
    noise = np.stack([float(d["noise_std"]) * np.random.default_rng(s).standard_normal((K, 360, 2)) for s in seeds], 1)
    noise = torch.as_tensor(noise, device="cuda")
    st0 = _states(np.tile(d["start"], (B, 1)))
    goal = torch.as_tensor(np.tile(d["goal"], (B, 1)), device="cuda")
    foot = torch.ones((B,), dtype=torch.int8, device="cuda")
    solved = lambda r: (r["last_status"] == 0) | (r["last_status"] == 4)
    plain = lipmpc.UnknownEnvFleet(grid=grid, N_horizon=3, lidar_range=rng_range).run(st0, goal, foot, K, noise=noise)
    torch.cuda.synchronize()
    stopped_by_rule = solved(plain) & (plain["n_steps"] < K)
    print("plain: steps", plain["n_steps"].tolist(), "status", plain["last_status"].tolist(), "CPU chain", d["plain_steps"].tolist())
    assert int(stopped_by_rule.sum()) == 0
    n, r_rewire, rrt_seed, max_cells = (int(v) for v in d["rrt"])
    w_hit, w_miss = (int(v) for v in d["weights"])
    mapper = lipmpc.OccupancyMapper(W, H, origin, cell, rng_range, per_robot=B, w_hit=w_hit, w_miss=w_miss)
    planner = lipmpc.RrtStarPlanner(n=n, r_rewire=r_rewire, seed=rrt_seed, max_cells=max_cells)
    fleet = lipmpc.UnknownEnvFleet(grid=grid, N_horizon=3, lidar_range=rng_range, mapper=mapper)
    r = fleet.run_replanning(st0, goal, foot, K, planner, int(d["replan_every"]), float(d["lookahead"]), noise=noise)
    torch.cuda.synchronize()
    arrived = (r["walking"] == 0) & solved(r) & (r["working_goal"] == goal).all(1)
    X, ns = r["X_pred"].cpu().numpy(), r["n_steps"].cpu().numpy()
    dist = np.hypot(X[np.arange(B), -1, 0] - d["goal"][0], X[np.arange(B), -1, 2] - d["goal"][1])
    print("replanning: steps", ns.tolist(), "status", r["last_status"].tolist(), "arrived", arrived.tolist(), "final distance",
          np.round(dist, 3).tolist(), "CPU chain", d["replanning_steps"].tolist(), "replans", r["n_replans"])
    assert int(arrived.sum()) >= B - 1
    assert (dist[arrived.cpu().numpy()] < 0.25).all()
