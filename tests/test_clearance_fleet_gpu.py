"""GPU: the exploring fleet with a FrontierPlanner that prices clearance, on the recorded open-field scene of
tests/test_frontier_fleet_gpu.py (tests/golden/exploration.npz), through that file's helpers as tests/test_field_tiled_fleet_gpu.py
uses them: with w_clear = 0 every tensor of the run is the plain tiled run's, bit for bit; with w_clear > 0 two runs give the same
bits and the run's bookkeeping agrees with the weighted oracle on its final map.  Whether the walker fails less with clearance is
not asserted here: the finishing sample is printed.  And run_replanning with a GridFieldPlanner that prices clearance, likewise."""
import numpy as np
import pytest

import clearance_oracle as CO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402
import test_frontier_fleet_gpu as base  # noqa: E402

R_CLEAR, W_CLEAR = 4, 40                                      # the two-door example's setting


def _explorer(d, **kw):
    return lipmpc.FrontierPlanner(r_inflate=int(d["r_inflate"]), min_unknown=int(d["min_unknown"]), tiled=True, **kw)


def _same_runs(want, got):
    assert set(got) == set(want)
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v.view(np.int64) if v.dtype == np.float64 else v, got[k].view(np.int64) if v.dtype == np.float64 else got[k]), k
        else:
            assert v == got[k], k


def test_gpu_w_clear_zero_is_the_plain_tiled_run_bit_for_bit():
    d, occ, _ = base._scene()
    seed = d["seeds"].tolist()[0]
    fleet, mapper, _ = base._fleet(d, occ)
    want = base._explore(d, fleet, mapper, _explorer(d), seed)
    got = base._explore(d, fleet, mapper, _explorer(d, r_clear=R_CLEAR, w_clear=0), seed)
    _same_runs(want, got)
    assert want["n_frontier"][0, 0] > 0 and (want["n_steps"] > 0).all()


def test_gpu_weighted_runs_repeat_and_agree_with_the_oracle_on_the_final_map():
    d, occ, cells = base._scene()
    seed = d["seeds"].tolist()[0]
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    K, every = int(d["k_max"]), int(d["replan_every"])
    fleet, mapper, _ = base._fleet(d, occ)
    explorer = _explorer(d, r_clear=R_CLEAR, w_clear=W_CLEAR)
    r = base._explore(d, fleet, mapper, explorer, seed)
    _same_runs(r, base._explore(d, fleet, mapper, explorer, seed))
    assert r["n_replans"] == (K + every - 1) // every
    assert r["n_frontier"].shape == (r["n_replans"], 1) and r["known_free"].shape == (r["n_replans"], 1)
    assert r["n_frontier"][0, 0] > 0 and r["known_free"][-1, 0] > r["known_free"][0, 0]
    # the closing plan, restated: the weighted oracle on the run's final evidence and positions
    pos = r["X_pred"][:, -1][:, (0, 2)]
    layer = CO.clearance_cost_evidence(r["evidence"], w_hit, R_CLEAR, W_CLEAR)
    want = CO.frontier_plan_batch(r["evidence"], layer, w_miss, w_hit, origin, cell, pos, int(d["r_inflate"]), int(d["min_unknown"]))
    assert np.array_equal(r["explore_status"], want["status"]), (r["explore_status"], want["status"])
    last = explorer.last
    torch.cuda.synchronize()
    assert np.array_equal(last["cost"][0].cpu().numpy(), layer) and layer.any()
    assert np.array_equal(last["field"].view(torch.int32).cpu().numpy().view(np.uint32), want["field"])
    assert np.array_equal(last["n_sub"].cpu().numpy(), want["n_sub"]) and np.array_equal(last["target_cell"].cpu().numpy(), want["target_cell"])
    failed = ~np.isin(r["last_status"], base.SOLVED)
    assert np.array_equal(r["done"], (want["status"] == CO.NO_PATH) & ~failed), (r["done"], want["status"], r["last_status"])
    assert not r["walking"][r["done"]].any() and not r["walking"][want["status"] != CO.FOUND].any()
    assert r["known_free"][-1, 0] <= (r["evidence"] <= -w_miss).sum()
    steps = r["n_steps"].tolist()
    print(f"seed {seed}, r_clear {R_CLEAR}, w_clear {W_CLEAR}: coverage {base._coverage(d, cells, r['evidence']):.4f}, frontier cells left "
          f"{int(r['n_frontier'][-1, 0])}, done {r['done'].tolist()}, last status {r['last_status'].tolist()}, steps {steps} of {K}, "
          f"closing plan {r['explore_status'].tolist()}")


def test_gpu_replanning_takes_a_weighted_field_planner_as_it_is():
    """UnknownEnvFleet.run_replanning with a GridFieldPlanner that prices clearance, no change to the fleet: a wall within LiDAR range
    lies between the robots and their goals, so the map the fleet builds has solid cells and the layer is not empty.  With
    w_clear = 0 the run is the plain tiled planner's, bit for bit; with w_clear > 0 two runs give the same bits."""
    B, K = 4, 12
    occ = np.zeros((120, 120), np.uint8)
    occ[25:27, 5:32] = 1                                       # x in [1.5, 1.7), y in [-0.5, 2.2): seen from the starts
    grid = lipmpc.GridMap(occ, (-1.0, -1.0), 0.1)
    pos = np.array([[0.0, 0.0], [0.4, 0.9], [0.9, 0.2], [0.7, 1.6]])
    st = np.zeros((B, 5)); st[:, 0] = pos[:, 0]; st[:, 2] = pos[:, 1]
    st0 = torch.as_tensor(st, device="cuda")
    goal = torch.tensor([[3.0, 3.0], [3.5, 1.0], [0.5, 3.0], [3.0, 0.0]], dtype=torch.float64, device="cuda")
    foot = torch.ones((B,), dtype=torch.int8, device="cuda")
    noise = 0.01 * torch.randn((K, B, 360, 2), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    mapper = lipmpc.OccupancyMapper(128, 128, (-1.0, -1.0), 0.08, 1.5)
    fleet = lipmpc.UnknownEnvFleet(grid=grid, N_horizon=3, lidar_range=1.5, mapper=mapper)

    def run(planner):
        mapper.reset()
        r = fleet.run_replanning(st0, goal, foot, K, planner, replan_every=3, lookahead=1.0, noise=noise)
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy().copy() for k, v in r.items() if isinstance(v, torch.Tensor)}
        out["n_replans"] = r["n_replans"]
        return out

    plain = run(lipmpc.GridFieldPlanner(r_inflate=1, tiled=True))
    _same_runs(plain, run(lipmpc.GridFieldPlanner(r_inflate=1, tiled=True, r_clear=R_CLEAR, w_clear=0)))
    priced = lipmpc.GridFieldPlanner(r_inflate=1, tiled=True, r_clear=R_CLEAR, w_clear=W_CLEAR)
    first = run(priced)
    _same_runs(first, run(priced))
    assert plain["n_replans"] == first["n_replans"] == 4 and (first["rrt_status"] == lipmpc.RRT_FOUND).any()
    layer = priced.last["cost"]
    assert tuple(layer.shape) == (1, 128, 128) and int(layer.max()) == W_CLEAR and priced.last["settled"].tolist() == [1] * B
    print("replanning: rrt_status", first["rrt_status"].tolist(), "steps", first["n_steps"].tolist(), "priced cells", int((layer != 0).sum()))
