"""GPU: GridFieldPlanner as the ``planner=`` of UnknownEnvFleet.run_replanning, with no change to the fleet: on a map whose
walls stay out of LiDAR range the robots' map stays empty, every plan is the one sub-goal "the goal itself", and the run equals
the reactive ``run`` bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402


def test_gpu_replanning_with_the_field_planner_on_an_empty_map_is_the_reactive_run():
    B, K = 4, 12
    occ = np.zeros((120, 120), np.uint8)
    occ[100:104, :] = 1                                        # x in [9, 9.4): never within 1.5 m of a robot that starts near the origin
    grid = lipmpc.GridMap(occ, (-1.0, -1.0), 0.1)
    pos = np.array([[0.0, 0.0], [0.4, 0.9], [1.1, 0.2], [0.7, 1.6]])
    st = np.zeros((B, 5)); st[:, 0] = pos[:, 0]; st[:, 2] = pos[:, 1]
    st0 = torch.as_tensor(st, device="cuda")
    goal = torch.tensor([[3.0, 3.0], [3.5, 1.0], [0.5, 3.0], [1.25, 1.9]], dtype=torch.float64, device="cuda")     # (the last: nearer than the lookahead)
    foot = torch.ones((B,), dtype=torch.int8, device="cuda")
    noise = 0.01 * torch.randn((K, B, 360, 2), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    mapper = lipmpc.OccupancyMapper(128, 128, (-1.0, -1.0), 0.08, 1.5)
    fleet = lipmpc.UnknownEnvFleet(grid=grid, N_horizon=3, lidar_range=1.5, mapper=mapper)
    plain = {k: v.cpu().numpy().copy() for k, v in fleet.run(st0, goal, foot, K, noise=noise).items()}
    mapper.reset()
    planner = lipmpc.GridFieldPlanner()
    r = fleet.run_replanning(st0, goal, foot, K, planner, replan_every=3, lookahead=1.0, noise=noise)
    torch.cuda.synchronize()
    assert set(r) >= {"X_pred", "U_pred", "n_steps", "last_status", "overflow", "n_replans", "rrt_status", "working_goal", "walking"}
    for k in ("X_pred", "U_pred", "n_steps"):
        a, b = r[k].cpu().numpy(), plain[k]
        assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b), k
    assert plain["n_steps"].max() >= 5 and int((mapper.evidence > 0).sum()) == 0          # the robots walked, and saw nothing
    assert r["n_replans"] == 4 and r["rrt_status"].tolist() == [lipmpc.RRT_FOUND] * B
    last = planner.last
    assert last["n_sub"].tolist() == [1] * B and torch.equal(last["sub_goals"][:, 0], goal)   # the single sub-goal is the goal itself
    assert torch.equal(r["working_goal"], goal) and tuple(last["field"].shape) == (B, 128, 128)
    assert np.array_equal(last["path_cost"].cpu().numpy() > 0, [True] * B)
