"""warm_start=True in the closed loops that step from the host (-m gpu): the compat classes' step-by-step loop and
UnknownEnvFleet carry each robot's previous result in a warm-start record (lipmpc_set_warm_start)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402
import lipmpc_oracle as O  # noqa: E402
from helpers import IPOPT_LIKE_TOL, load_rings, unknown_env_scenario  # noqa: E402


def test_unknown_environment_class_warm_start(golden_dir):
    """The reference's unknown-environment scene (test_gpu_unknown_environment_class_against_the_reference_figure): the
    warm-started class takes fewer iterations per MPC step and ends where the cold one does.  (The clusters of one scan
    may come in another order in the next, so a record slot does not always hold the same obstacle's multipliers.)"""
    sc = unknown_env_scenario(golden_dir)
    runs = {}
    for warm in (False, True):
        mpc = lipmpc.HumanoidMPCUnknownEnvironment(goal=sc["goal"], obstacles=sc["env"], N_horizon=sc["N"], N_mpc_timesteps=300,
                                                   sampling_time=0.4, init_state=sc["init"], verbosity=0,
                                                   lidar_range=sc["lidar_range"], noise_seed=0, warm_start=warm)
        X, U, _ = mpc.run_simulation(None, make_fast_plot=False, fill_animator=False)
        runs[warm] = (X, np.array(mpc.solver_iters))
        if warm:
            assert mpc._ce_solver.warm_record is not None and mpc._ce_solver.params.n_obs_max >= 12
    (Xc, itc), (Xw, itw) = runs[False], runs[True]
    print(f"unknown environment: iterations per MPC step cold {itc.mean():.2f} ({len(itc)} steps), "
          f"warm {itw.mean():.2f} ({len(itw)} steps)")
    assert len(itc) > 10 and len(itw) > 10
    assert itw.mean() < itc.mean()
    assert np.hypot(Xw[0, -1] - Xc[0, -1], Xw[2, -1] - Xc[2, -1]) < 0.3


class _StockListsMPC(lipmpc.HumanoidMPC):
    """Overrides the hook with the stock lists: the class takes the step-by-step path through lipmpc_plan_step_batch_c_eta."""

    def _get_list_c_and_eta(self, x_k, y_k):
        return lipmpc.HumanoidMPC._get_list_c_and_eta(self, x_k, y_k)


def test_stepwise_c_eta_path_warm_start_matches_oracle(golden_dir):
    """The step-by-step c_eta path with warm_start=True tracks the oracle's warm-started closed loop on the circles scenario,
    under the bars of test_rollout_warm_start_matches_oracle_and_saves_iterations, and needs fewer iterations than cold."""
    obs = load_rings(os.path.join(golden_dir, "scenario_circles.npz"))
    kw = dict(N_horizon=3, N_mpc_timesteps=300, sampling_time=0.4, init_state=(0, 0, 3, 0, 0))
    its = {}
    for warm in (False, True):
        mpc = _StockListsMPC(goal=(6, -3), obstacles=obs, verbosity=0, warm_start=warm, **kw)
        X, U, _ = mpc.run_simulation(None, make_fast_plot=False, fill_animator=False)
        its[warm] = float(np.mean(mpc.solver_iters))
        if warm:
            Xw = X
    Xo, Uo = O.run_closed_loop((6, -3), obs, exact=False, params=O.Params(tol_interior=IPOPT_LIKE_TOL), warm_start=True, **kw)
    n = min(12, Xw.shape[1], Xo.shape[1])
    print(f"stepwise c_eta path: iterations per step cold {its[False]:.2f}, warm {its[True]:.2f}, "
          f"oracle warm {np.mean(O.run_closed_loop.last_iters):.2f}")
    assert abs(Xw.shape[1] - Xo.shape[1]) <= 3 and np.max(np.abs(Xw[:, :n] - Xo[:, :n])) < 1e-6
    assert np.hypot(Xw[0, -1] - 6, Xw[2, -1] + 3) < 0.3
    assert its[True] < its[False]


def test_fleet_warm_start_graph_equals_eager(golden_dir):
    """UnknownEnvFleet(warm_start=True): the captured graph replays the eager loop bit for bit (the record is part of the
    captured sample), and every run starts from a zeroed record (a second run of the same shape repeats the first)."""
    d = np.load(os.path.join(golden_dir, "lidar_golden.npz"))
    rings = [d["env"][0][j][: d["env_nv"][0][j]] for j in range(d["env"].shape[1]) if d["env_nv"][0][j] > 0]
    B, K = 8, 25
    noise = 0.01 * torch.randn((K, B, 360, 2), dtype=torch.float64, device="cuda",
                               generator=torch.Generator(device="cuda").manual_seed(5))
    st0 = torch.tensor([[-0.8, 0, -0.8, 0, 0.7]] * B, dtype=torch.float64, device="cuda")
    st0[:, 0] += torch.linspace(0.0, 0.3, B, dtype=torch.float64, device="cuda")
    goal = torch.tensor([[5.0, 5.0]] * B, dtype=torch.float64, device="cuda")
    foot = torch.ones((B,), dtype=torch.int8, device="cuda")
    res = {}
    for use_graph in (False, True):
        fleet = lipmpc.UnknownEnvFleet(rings, N_horizon=3, lidar_range=1.5, warm_start=True)
        for _ in range(2):                       # a second run of the same shape starts from a zeroed record again
            r = fleet.run(st0, goal, foot, K, noise=noise, use_graph=use_graph)
            torch.cuda.synchronize()
            res.setdefault(use_graph, []).append({k: v.cpu().numpy().copy() for k, v in r.items()})
    for a, b in ((res[False][0], res[True][0]), (res[False][1], res[True][1]), (res[True][0], res[True][1])):
        for k in a:      # (NaN: the outputs of a robot whose step failed)
            assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    cold = lipmpc.UnknownEnvFleet(rings, N_horizon=3, lidar_range=1.5).run(st0, goal, foot, K, noise=noise, use_graph=False)
    torch.cuda.synchronize()
    print("fleet n_steps warm", res[True][0]["n_steps"], "last_status", res[True][0]["last_status"],
          "cold", cold["n_steps"].cpu().numpy(), "last_status", cold["last_status"].cpu().numpy())
    assert res[True][0]["overflow"].sum() == 0 and res[True][0]["n_steps"].max() == K
    assert np.array_equal(res[True][0]["n_steps"], cold["n_steps"].cpu().numpy())      # the warm robots walk as far
