"""GPU: the fleet that explores (UnknownEnvFleet.run_exploring with a FrontierPlanner) on the scene of
tests/golden/exploration.npz -- chosen on the CPU by tests/golden/make_exploration.py, reasoning and counts in EXPLORATION.md --
one run per recorded noise seed: the run's own bookkeeping against the numpy oracle on its final map, two runs and the run
without a graph bit for bit, and the coverage against the CPU chain's."""
import functools
import os

import numpy as np
import pytest

import field_oracle as FO
import frontier_oracle as FR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

SOLVED = (0, 4)                                               # STATUS_SOLVED, STATUS_UNCERTIFIED


@functools.lru_cache(maxsize=None)
def _scene():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exploration.npz"))
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    occ = np.zeros((W, H), np.uint8)
    for i0, j0, i1, j1 in d["walls"]:
        occ[i0:i1, j0:j1] = 1
    r = int(d["r_inflate"])
    # the cells that count: unblocked at r_inflate on the TRUE map and connected to the first start
    blocked = FO.blocked_cells(occ, r)
    s = FO.cell_of(d["starts"][0], origin, cell, W, H)
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


def _states(pos):
    st = np.zeros((len(pos), 5)); st[:, 0] = pos[:, 0]; st[:, 2] = pos[:, 1]
    return torch.as_tensor(st, device="cuda")


def _noise(d, seed):
    """make_exploration.noise_of: what the CPU chain of this seed read."""
    K, B = int(d["k_max"]), len(d["starts"])
    return torch.as_tensor(float(d["noise_std"]) * np.random.default_rng(seed).standard_normal((K, B, 360, 2)), device="cuda")


def _fleet(d, occ):
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    rng = float(d["lidar_range"])
    mapper = lipmpc.OccupancyMapper(W, H, origin, cell, rng, w_hit=w_hit, w_miss=w_miss)          # one shared map
    fleet = lipmpc.UnknownEnvFleet(grid=lipmpc.GridMap(occ, origin, cell), N_horizon=3, lidar_range=rng, mapper=mapper)
    return fleet, mapper, lipmpc.FrontierPlanner(r_inflate=int(d["r_inflate"]), min_unknown=int(d["min_unknown"]))


def _explore(d, fleet, mapper, explorer, seed, **kw):
    mapper.reset()
    B = len(d["starts"])
    r = fleet.run_exploring(_states(d["starts"]), torch.ones((B,), dtype=torch.int8, device="cuda"), int(d["k_max"]), explorer,
                            int(d["replan_every"]), float(d["lookahead"]), noise=_noise(d, seed), **kw)
    torch.cuda.synchronize()
    out = {k: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
    out["evidence"] = mapper.evidence.cpu().numpy().copy()
    return out


def _coverage(d, cells, ev):
    return float((ev[cells] <= -int(d["weights"][1])).sum() / cells.sum())


@functools.lru_cache(maxsize=None)
def _runs():
    """One exploring run per recorded seed (and, for the first seed, a second run of the same shape and one without a graph)."""
    d, occ, cells = _scene()
    fleet, mapper, explorer = _fleet(d, occ)
    seeds = d["seeds"].tolist()
    runs = {s: _explore(d, fleet, mapper, explorer, s) for s in seeds}
    again = _explore(d, fleet, mapper, explorer, seeds[0])
    eager = _explore(d, fleet, mapper, explorer, seeds[0], use_graph=False)
    return runs, again, eager


def test_gpu_the_recorded_scene_is_what_the_cpu_chain_finished():
    d, occ, cells = _scene()
    assert 2 <= len(d["starts"]) <= 4 and int(d["k_max"]) <= 120 and len(d["seeds"]) >= 4
    assert d["exploring_finished"].all()                       # the CPU chain misses none at the chosen settings
    assert d["reactive_coverage"].max() < d["exploring_coverage"].min()
    assert 2500 < cells.sum() < 64 * 56


def test_gpu_bookkeeping_is_consistent_with_the_oracle_on_the_final_map():
    d, occ, cells = _scene()
    runs, _, _ = _runs()
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    K, every, B = int(d["k_max"]), int(d["replan_every"]), len(d["starts"])
    for seed, r in runs.items():
        assert r["n_replans"] == (K + every - 1) // every
        assert r["n_frontier"].shape == (r["n_replans"], 1) and r["known_free"].shape == (r["n_replans"], 1)
        assert r["n_frontier"][0, 0] > 0 and r["known_free"][-1, 0] > r["known_free"][0, 0]
        # the closing plan, restated: the numpy oracle on the run's final evidence and positions
        pos = r["X_pred"][:, -1][:, (0, 2)]                      # (every sample writes every robot's row, walking or not)
        want = FR.plan_batch(r["evidence"], w_miss, w_hit, origin, cell, pos, int(d["r_inflate"]), int(d["min_unknown"]))
        assert np.array_equal(r["explore_status"], want["status"]), (seed, r["explore_status"], want["status"])
        failed = ~np.isin(r["last_status"], SOLVED)
        assert np.array_equal(r["done"], (want["status"] == FR.NO_PATH) & ~failed), (seed, r["done"], want["status"], r["last_status"])
        assert not r["walking"][r["done"]].any() and not r["walking"][want["status"] != FR.FOUND].any()
        assert r["known_free"][-1, 0] <= (r["evidence"] <= -w_miss).sum()


def test_gpu_two_runs_and_the_run_without_a_graph_give_the_same_bits():
    runs, again, eager = _runs()
    first = runs[_scene()[0]["seeds"].tolist()[0]]
    for other in (again, eager):
        for k, v in first.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v.view(np.int64) if v.dtype == np.float64 else v, other[k].view(np.int64) if v.dtype == np.float64 else other[k]), k
            else:
                assert v == other[k], k


def test_gpu_coverage_against_the_cpu_chain():
    """The bar: the smallest coverage the CPU chain recorded over its seeds, minus the spread (max - min) of those seeds -- device
    and CPU chain part where a reading falls on the other side of a cell boundary.  At most one seed may miss it.  The reactive run
    toward the far corner covers less on every seed, as on the CPU."""
    d, occ, cells = _scene()
    runs, _, _ = _runs()
    cpu = d["exploring_coverage"]
    bar = float(cpu.min() - (cpu.max() - cpu.min()))
    cov = {s: _coverage(d, cells, r["evidence"]) for s, r in runs.items()}
    print("coverage: device", {s: round(c, 4) for s, c in cov.items()}, "CPU chain", np.round(cpu, 4).tolist(), "bar", round(bar, 4))
    print("device: frontier cells left", {s: int(r["n_frontier"][-1, 0]) for s, r in runs.items()}, "done", {s: r["done"].tolist() for s, r in runs.items()},
          "last status", {s: r["last_status"].tolist() for s, r in runs.items()}, "steps", {s: r["n_steps"].tolist() for s, r in runs.items()})
    assert sum(c < bar for c in cov.values()) <= 1, (cov, bar)
    # the reactive loop on the same seeds: the same fleet, every robot toward the far corner
    fleet, mapper, _ = _fleet(d, occ)
    B = len(d["starts"])
    goal = torch.as_tensor(np.tile(d["far_corner"], (B, 1)), device="cuda")
    for n, seed in enumerate(d["seeds"].tolist()):
        mapper.reset()
        fleet.run(_states(d["starts"]), goal, torch.ones((B,), dtype=torch.int8, device="cuda"), int(d["k_max"]), noise=_noise(d, seed))
        torch.cuda.synchronize()
        reactive = _coverage(d, cells, mapper.evidence.cpu().numpy())
        print(f"seed {seed}: reactive coverage {reactive:.4f} (CPU chain {d['reactive_coverage'][n]:.4f}), exploring {cov[seed]:.4f}")
        assert reactive < cov[seed] and reactive < bar
