"""GPU: the exploring fleet with a CoordinatedFrontierPlanner (UnknownEnvFleet(recover=).run_exploring) on the scene of
tests/golden/exploration_assigned.npz -- recorded on the CPU by tests/golden/make_exploration_assigned.py, counts and bars in
EXPLORATION_ASSIGNED.md.  Four robots side by side, one shared map, one run per recorded noise seed: the closing plan, the done
flags and the n_claims rows are what the numpy oracle says on the run's final evidence and positions; two runs and the run without
a graph give the same bits; coverage is held against the CPU chain's.  Whether the assigned fleet finishes sooner than the
nearest-frontier fleet is recorded, not asserted: the CPU chains do not show it (EXPLORATION_ASSIGNED.md)."""
import functools
import os

import numpy as np
import pytest

import assign_oracle as A
import field_oracle as FO
import frontier_oracle as FR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

SOLVED = (0, 4)                                               # STATUS_SOLVED, STATUS_UNCERTIFIED
HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _scene():
    d = np.load(os.path.join(HERE, "golden", "exploration_assigned.npz"))
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    occ = np.zeros((W, H), np.uint8)
    for i0, j0, i1, j1 in d["walls"]:
        occ[i0:i1, j0:j1] = 1
    # the cells that count for the coverage (make_exploration.reachable): unblocked at r_inflate on the TRUE map and connected to
    # make_exploration.py's first start
    blocked = FO.blocked_cells(occ, int(d["r_inflate"]))
    s = FO.cell_of(np.load(os.path.join(HERE, "golden", "exploration.npz"))["starts"][0], origin, cell, W, H)
    seen, todo = {s}, [s]
    while todo:
        i, j = todo.pop()
        for a, b, _ in FO.moves_from(blocked, i, j):
            if (a, b) not in seen:
                seen.add((a, b))
                todo.append((a, b))
    cells = np.zeros((W, H), bool)
    cells[tuple(np.array(sorted(seen)).T)] = True
    return d, occ, cells


def _fleet():
    d, occ, _ = _scene()
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    rng = float(d["lidar_range"])
    mapper = lipmpc.OccupancyMapper(W, H, origin, cell, rng, w_hit=w_hit, w_miss=w_miss)          # one shared map
    fleet = lipmpc.UnknownEnvFleet(grid=lipmpc.GridMap(occ, origin, cell), N_horizon=3, lidar_range=rng, mapper=mapper,
                                   recover=int(d["max_recover"]))
    explorer = lipmpc.CoordinatedFrontierPlanner(int(d["r_claim"]), int(d["max_claims"]), r_inflate=int(d["r_inflate"]),
                                                 min_unknown=int(d["min_unknown"]))
    return fleet, mapper, explorer


def _explore(fleet, mapper, explorer, seed, **kw):
    d, _, _ = _scene()
    starts, K = d["starts"], int(d["k_max"])
    B = len(starts)
    st = np.zeros((B, 5)); st[:, 0] = starts[:, 0]; st[:, 2] = starts[:, 1]
    # make_exploration_assigned.noise_of: what the CPU chain of this seed read
    noise = torch.as_tensor(float(d["noise_std"]) * np.random.default_rng(seed).standard_normal((K, B, 360, 2)), device="cuda")
    mapper.reset()
    r = fleet.run_exploring(torch.as_tensor(st, device="cuda"), torch.ones((B,), dtype=torch.int8, device="cuda"), K, explorer,
                            int(d["replan_every"]), float(d["lookahead"]), noise=noise, **kw)
    torch.cuda.synchronize()
    out = {k: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
    out["evidence"] = mapper.evidence.cpu().numpy().copy()
    out["closing"] = {k: explorer.last[k].cpu().numpy().copy() for k in ("claim_round", "n_claims", "target_cell", "status", "n_sub")}
    return out


@functools.lru_cache(maxsize=None)
def _runs():
    """One exploring run per recorded seed (and, for the first seed, a second run of the same shape and one without a graph)."""
    d, _, _ = _scene()
    fleet, mapper, explorer = _fleet()
    seeds = d["seeds"].tolist()
    runs = {s: _explore(fleet, mapper, explorer, s) for s in seeds}
    return runs, _explore(fleet, mapper, explorer, seeds[0]), _explore(fleet, mapper, explorer, seeds[0], use_graph=False)


def test_gpu_the_recorded_scene_is_what_the_cpu_chains_ran():
    d, occ, cells = _scene()
    assert 3 <= len(d["starts"]) <= 6 and len(d["seeds"]) == 6 and int(d["r_claim"]) == 15 and int(d["max_claims"]) == 64
    assert np.ptp(d["starts"][:, 0]) == 0 and np.allclose(np.diff(d["starts"][:, 1]), 0.2)       # side by side
    near, asg = d["nearest/first_targets"], d["assigned/first_targets"]
    dist = lambda t: np.sqrt(((t[:, None] - t[None]) ** 2).sum(2))[np.triu_indices(len(t), 1)]
    assert dist(near).min() <= 2 and (d["assigned/n_claims"][:, 0] >= 3).all() and (d["nearest/n_claims"] <= 0).all()
    assert np.sort(dist(asg))[-3:].min() > 15                  # the claims spread the first targets over the ring


def test_gpu_bookkeeping_is_consistent_with_the_oracle_on_the_final_map():
    d, occ, cells = _scene()
    runs, _, _ = _runs()
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    K, every, B = int(d["k_max"]), int(d["replan_every"]), len(d["starts"])
    for seed, r in runs.items():
        n = r["n_replans"]
        assert n == (K + every - 1) // every and r["n_claims"].shape == (n,) and r["n_frontier"].shape == (n, 1)
        assert ((0 <= r["n_claims"]) & (r["n_claims"] <= B)).all() and (r["n_claims"][r["n_frontier"][:, 0] == 0] == 0).all()
        # the first replan sees the noise-free first scan, the same on every seed and on the CPU
        assert r["n_claims"][0] == d["assigned/n_claims"][0, 0]
        # the closing plan, restated: the numpy oracle on the run's final evidence and positions, the robots that may claim being
        # those whose last solve succeeded
        pos = r["X_pred"][:, -1][:, (0, 2)]                      # (every sample writes every robot's row, walking or not)
        failed = ~np.isin(r["last_status"], SOLVED)
        want = A.plan_batch(r["evidence"], w_miss, w_hit, origin, cell, pos, int(d["r_claim"]), int(d["max_claims"]), int(d["r_inflate"]),
                            int(d["min_unknown"]), None, 64, may_claim=~failed)
        assert np.array_equal(r["explore_status"], want["status"]), (seed, r["explore_status"], want["status"])
        for k in ("claim_round", "target_cell", "status", "n_sub"):
            assert np.array_equal(r["closing"][k], want[k]), (seed, k, r["closing"][k], want[k])
        assert int(r["closing"]["n_claims"][0]) == want["n_claims"] and (want["claim_round"][failed] == -1).all()
        assert np.array_equal(r["done"], (want["status"] == FR.NO_PATH) & ~failed), (seed, r["done"], want["status"], r["last_status"])
        assert not r["walking"][r["done"]].any() and not r["walking"][want["status"] != FR.FOUND].any()


def test_gpu_two_runs_and_the_run_without_a_graph_give_the_same_bits():
    runs, again, eager = _runs()
    first = runs[_scene()[0]["seeds"].tolist()[0]]
    same = lambda a, b: np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if a.dtype == np.float64 else b)
    for other in (again, eager):
        for k, v in first.items():
            if isinstance(v, np.ndarray):
                assert same(v, other[k]), k
            elif isinstance(v, dict):
                assert all(same(x, other[k][j]) for j, x in v.items()), k
            else:
                assert v == other[k], k


def test_gpu_coverage_against_the_cpu_chain_and_the_finishing_samples():
    """The bar is EXPLORATION_ASSIGNED.md's: the smallest coverage the CPU assigned chain recorded over its seeds minus the spread
    (max - min) of those seeds; at most one seed may miss it.  The finishing samples are printed beside the CPU chains' and not
    asserted: on the CPU the assigned fleet does not finish sooner than the nearest-frontier fleet by more than the seed spread."""
    d, occ, cells = _scene()
    runs, _, _ = _runs()
    w_miss, every = int(d["weights"][1]), int(d["replan_every"])
    cpu = d["assigned/coverage"]
    bar = float(cpu.min() - (cpu.max() - cpu.min()))
    cov = {s: float((r["evidence"][cells] <= -w_miss).sum() / cells.sum()) for s, r in runs.items()}
    at = {s: (int(np.argmax(r["n_frontier"][:, 0] == 0)) * every if (r["n_frontier"][:, 0] == 0).any() else -1) for s, r in runs.items()}
    print("coverage: device", {s: round(c, 4) for s, c in cov.items()}, "CPU assigned chain", np.round(cpu, 4).tolist(), "bar", round(bar, 4))
    print("finished at: device", at, "CPU assigned", np.where(d["assigned/finished"], d["assigned/finished_at"], -1).tolist(), "CPU nearest",
          np.where(d["nearest/finished"], d["nearest/finished_at"], -1).tolist(), "(recorded, not asserted)")
    print("device: claims per replan", {s: r["n_claims"].tolist() for s, r in runs.items()}, "last status",
          {s: r["last_status"].tolist() for s, r in runs.items()}, "steps", {s: r["n_steps"].tolist() for s, r in runs.items()})
    assert not bool(d["assigned_sooner_every_seed"])           # (were it true, the finishing sample would be asserted here)
    assert sum(c < bar for c in cov.values()) <= 1, (cov, bar)
