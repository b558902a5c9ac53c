"""GPU: the exploring fleet with an InformedFrontierPlanner (UnknownEnvFleet(recover=).run_exploring) on the `field` scene of
tests/golden/exploration_informed.npz under its `pruned` rule -- recorded on the CPU by tests/golden/make_exploration_informed.py,
counts and bars in EXPLORATION_INFORMED.md.  Four robots side by side, one shared map, one run per recorded noise seed: the closing
plan is what the numpy oracle says on the run's final evidence and positions, its targets are sources worth seeing, two runs give
the same bits, and coverage is held against the CPU chain's.  The finishing sample is recorded, not asserted: the CPU chains do not
show the informed fleet sooner than the nearest-frontier fleet by more than the seed spread (EXPLORATION_INFORMED.md)."""
import functools
import os

import numpy as np
import pytest

import field_oracle as FO
import frontier_oracle as FR
import gain_oracle as G

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

SOLVED = (0, 4)                                               # STATUS_SOLVED, STATUS_UNCERTIFIED
HERE = os.path.dirname(os.path.abspath(__file__))
SCENE, RULE = "field", "pruned"


@functools.lru_cache(maxsize=None)
def _scene():
    d = np.load(os.path.join(HERE, "golden", "exploration_informed.npz"))
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


def _gain_args(d):
    return int(d["r_view"]), int(d["w_gain"]), int(d["g_cap"]), int(d["min_gain"])


def _fleet():
    d, occ, _ = _scene()
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    rng = float(d["lidar_range"])
    mapper = lipmpc.OccupancyMapper(W, H, origin, cell, rng, w_hit=w_hit, w_miss=w_miss)          # one shared map
    fleet = lipmpc.UnknownEnvFleet(grid=lipmpc.GridMap(occ, origin, cell), N_horizon=3, lidar_range=rng, mapper=mapper,
                                   recover=int(d["max_recover"]))
    explorer = lipmpc.InformedFrontierPlanner(*_gain_args(d), r_inflate=int(d["r_inflate"]), min_unknown=int(d["min_unknown"]))
    return fleet, mapper, explorer


def _explore(fleet, mapper, explorer, seed, **kw):
    d, _, _ = _scene()
    starts, K = d[f"{SCENE}/starts"], int(d[f"{SCENE}/k_max"])
    B = len(starts)
    st = np.zeros((B, 5)); st[:, 0] = starts[:, 0]; st[:, 2] = starts[:, 1]
    # make_exploration_informed.noise_of: what the CPU chain of this seed read
    noise = torch.as_tensor(float(d["noise_std"]) * np.random.default_rng(seed).standard_normal((K, B, 360, 2)), device="cuda")
    mapper.reset()
    r = fleet.run_exploring(torch.as_tensor(st, device="cuda"), torch.ones((B,), dtype=torch.int8, device="cuda"), K, explorer,
                            int(d["replan_every"]), float(d["lookahead"]), noise=noise, **kw)
    torch.cuda.synchronize()
    out = {k: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
    out["evidence"] = mapper.evidence.cpu().numpy().copy()
    out["closing"] = {k: explorer.last[k].cpu().numpy().copy() for k in ("target_cell", "target_gain", "status", "n_sub", "n_sources", "n_frontier",
                                                                         "gain", "frontier")}
    out["closing"]["ufield"] = explorer.last["ufield"].view(torch.int32).cpu().numpy().view(np.uint32).copy()
    return out


@functools.lru_cache(maxsize=None)
def _runs():
    """One exploring run per recorded seed and, for the first seed, a second run of the same shape."""
    d, _, _ = _scene()
    fleet, mapper, explorer = _fleet()
    seeds = d[f"{SCENE}/seeds"].tolist()
    runs = {s: _explore(fleet, mapper, explorer, s) for s in seeds}
    return runs, _explore(fleet, mapper, explorer, seeds[0])


def test_gpu_the_closing_plan_is_consistent_and_is_the_oracles():
    d, occ, cells = _scene()
    runs, _ = _runs()
    origin, cell = tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    r_view, w_gain, g_cap, min_gain = _gain_args(d)
    K, every = int(d[f"{SCENE}/k_max"]), int(d["replan_every"])
    for seed, r in runs.items():
        c = r["closing"]
        assert r["n_replans"] == (K + every - 1) // every and r["n_frontier"].shape == (r["n_replans"], 1)
        has = c["target_cell"] >= 0
        assert np.array_equal(has, np.isin(c["status"], (G.FOUND, G.PATH_OVERFLOW))) and (c["target_gain"][~has] == -1).all()
        assert (c["target_gain"][has] >= min_gain).all()
        t = c["target_cell"][has]
        flat = lambda a: a[0].reshape(-1)
        assert (flat(c["frontier"])[t] != 0).all() and np.array_equal(flat(c["gain"])[t], c["target_gain"][has])      # targets are source cells ...
        assert all(int(flat(c["ufield"])[x]) == G.seed(flat(c["gain"])[x], w_gain, g_cap) for x in t)                  # ... that nothing dominates
        failed = ~np.isin(r["last_status"], SOLVED)
        assert np.array_equal(r["done"], (c["status"] == G.NO_PATH) & ~failed & (r["walking"] == 0))
        if r["done"].any():                                    # done is reached only when nothing worth seeing is left
            assert c["n_sources"].tolist() == [0]
        assert c["n_sources"][0] <= c["n_frontier"][0]
        # the closing plan, restated: the numpy oracle on the run's final evidence and positions
        pos = r["X_pred"][:, -1][:, (0, 2)]                      # (every sample writes every robot's row, walking or not)
        want = G.plan_batch(r["evidence"], w_miss, w_hit, origin, cell, pos, r_view, w_gain, g_cap, min_gain, int(d["r_inflate"]),
                            int(d["min_unknown"]), None, 64)
        assert np.array_equal(r["explore_status"], want["status"]), (seed, r["explore_status"], want["status"])
        for k in ("target_cell", "target_gain", "status", "n_sub", "n_sources", "n_frontier", "gain", "ufield"):
            assert np.array_equal(c[k], want[k]), (seed, k)


def test_gpu_two_runs_give_the_same_bits():
    runs, again = _runs()
    first = runs[_scene()[0][f"{SCENE}/seeds"].tolist()[0]]
    same = lambda a, b: np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if a.dtype == np.float64 else b)
    for k, v in first.items():
        if isinstance(v, np.ndarray):
            assert same(v, again[k]), k
        elif isinstance(v, dict):
            assert all(same(x, again[k][j]) for j, x in v.items()), k
        else:
            assert v == again[k], k


def test_gpu_coverage_against_the_cpu_chain_and_the_finishing_samples():
    """The bar is EXPLORATION_INFORMED.md's: the smallest coverage the CPU chain of this rule recorded over its seeds minus the spread
    (max - min) of those seeds; at most one seed may miss it.  The finishing samples are printed beside the CPU chains' and not
    asserted."""
    d, occ, cells = _scene()
    runs, _ = _runs()
    w_miss = int(d["weights"][1])
    cpu = d[f"{SCENE}/{RULE}/coverage"]
    bar = float(cpu.min() - (cpu.max() - cpu.min()))
    cov = {s: float((r["evidence"][cells] <= -w_miss).sum() / cells.sum()) for s, r in runs.items()}
    print("coverage: device", {s: round(c, 4) for s, c in cov.items()}, "CPU chain", np.round(cpu, 4).tolist(), "bar", round(bar, 4))
    print("closing plan: sources left", {s: int(r["closing"]["n_sources"][0]) for s, r in runs.items()}, "frontier cells left",
          {s: int(r["closing"]["n_frontier"][0]) for s, r in runs.items()}, "CPU finished at",
          np.where(d[f"{SCENE}/{RULE}/finished"], d[f"{SCENE}/{RULE}/finished_at"], -1).tolist(), "CPU nearest",
          np.where(d[f"{SCENE}/nearest/finished"], d[f"{SCENE}/nearest/finished_at"], -1).tolist(), "(recorded, not asserted)")
    print("device: last status", {s: r["last_status"].tolist() for s, r in runs.items()}, "steps", {s: r["n_steps"].tolist() for s, r in runs.items()})
    assert sum(c < bar for c in cov.values()) <= 1, (cov, bar)
