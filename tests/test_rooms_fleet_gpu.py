"""GPU: the exploring fleet INSIDE rooms (UnknownEnvFleet(split_rays=).run_exploring) on the scene of
tests/golden/exploration_rooms.npz -- chosen on the CPU by tests/golden/make_exploration_rooms.py, counts in EXPLORATION_ROOMS.md.
B = 3 robots, one shared map, one run per recorded noise seed: with one hull per cluster two robots never take a step; with the
sector split none fails at sample 0, the run's bookkeeping agrees with the numpy oracle on its final map, two runs and the run
without a graph give the same bits, and coverage and finishing are held against the CPU chain's."""
import functools
import os

import numpy as np
import pytest

import field_oracle as FO
import frontier_oracle as FR
import lidar_split_oracle as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

SOLVED = (0, 4)                                               # STATUS_SOLVED, STATUS_UNCERTIFIED
INFEASIBLE = 2


@functools.lru_cache(maxsize=None)
def _scene():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exploration_rooms.npz"))
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    occ, o2, c2 = S.rooms_scene(tuple(d["door"].tolist()))
    assert occ.shape == (W, H) and o2 == origin and c2 == cell
    # the cells that count for the coverage: unblocked at r_inflate on the TRUE map and connected to the first start
    blocked = FO.blocked_cells(occ, int(d["r_inflate"]))
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
    """make_exploration_rooms.noise_of: what the CPU chain of this seed read."""
    K, B = int(d["k_max"]), len(d["starts"])
    return torch.as_tensor(float(d["noise_std"]) * np.random.default_rng(seed).standard_normal((K, B, 360, 2)), device="cuda")


def _fleet(d, occ, split_rays):
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    rng = float(d["lidar_range"])
    mapper = lipmpc.OccupancyMapper(W, H, origin, cell, rng, w_hit=w_hit, w_miss=w_miss)          # one shared map
    fleet = lipmpc.UnknownEnvFleet(grid=lipmpc.GridMap(occ, origin, cell), N_horizon=3, lidar_range=rng, mapper=mapper, split_rays=split_rays)
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


@functools.lru_cache(maxsize=None)
def _runs():
    """One exploring run per recorded seed with the recorded split_rays (and, for the first seed, a second run of the same shape
    and one without a graph)."""
    d, occ, cells = _scene()
    fleet, mapper, explorer = _fleet(d, occ, int(d["split_rays"]))
    seeds = d["seeds"].tolist()
    runs = {s: _explore(d, fleet, mapper, explorer, s) for s in seeds}
    again = _explore(d, fleet, mapper, explorer, seeds[0])
    eager = _explore(d, fleet, mapper, explorer, seeds[0], use_graph=False)
    return runs, again, eager


def test_gpu_the_recorded_rooms_scene_is_what_the_cpu_chain_finished():
    d, occ, cells = _scene()
    assert len(d["starts"]) == 3 and len(d["seeds"]) == 6 and int(d["split_rays"]) in (30, 45, 60)
    assert d["split_finished"].all()                           # the CPU chain finishes on all six seeds at the chosen setting
    assert ((d["unsplit_steps"] == 0).sum(1) == 2).all()       # ... and with one hull per cluster two robots never step, on every seed
    assert (d["split_steps"] > 0).all()
    assert 1500 < cells.sum() < 64 * 56


def test_gpu_without_the_split_two_robots_never_step():
    """One hull per cluster: a robot in the room stands inside the hull of its walls -- n_steps = 0, INFEASIBLE, for at least two
    of the three robots on every seed (the CPU chain: exactly two)."""
    d, occ, cells = _scene()
    fleet, mapper, explorer = _fleet(d, occ, 0)
    for seed in d["seeds"].tolist():
        r = _explore(d, fleet, mapper, explorer, seed)
        stuck = (r["n_steps"] == 0) & (r["last_status"] == INFEASIBLE)
        print(f"seed {seed}: steps {r['n_steps'].tolist()}, last status {r['last_status'].tolist()}")
        assert stuck.sum() >= 2, (seed, r["n_steps"], r["last_status"])


def test_gpu_with_the_split_no_robot_fails_at_sample_0():
    runs, _, _ = _runs()
    for seed, r in runs.items():
        print(f"seed {seed}: steps {r['n_steps'].tolist()}, last status {r['last_status'].tolist()}, done {r['done'].tolist()}")
        assert (r["n_steps"] > 0).all(), (seed, r["n_steps"], r["last_status"])


def test_gpu_rooms_bookkeeping_is_consistent_with_the_oracle_on_the_final_map():
    d, occ, cells = _scene()
    runs, _, _ = _runs()
    origin, cell = tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    K, every = int(d["k_max"]), int(d["replan_every"])
    for seed, r in runs.items():
        assert r["n_replans"] == (K + every - 1) // every
        assert r["n_frontier"][0, 0] > 0 and r["known_free"][-1, 0] > r["known_free"][0, 0]
        # the closing plan, restated: the numpy oracle on the run's final evidence and positions
        pos = r["X_pred"][:, -1][:, (0, 2)]
        want = FR.plan_batch(r["evidence"], w_miss, w_hit, origin, cell, pos, int(d["r_inflate"]), int(d["min_unknown"]))
        assert np.array_equal(r["explore_status"], want["status"]), (seed, r["explore_status"], want["status"])
        failed = ~np.isin(r["last_status"], SOLVED)
        assert np.array_equal(r["done"], (want["status"] == FR.NO_PATH) & ~failed), (seed, r["done"], want["status"], r["last_status"])
        assert not r["walking"][r["done"]].any() and not r["walking"][want["status"] != FR.FOUND].any()


def test_gpu_rooms_two_runs_and_the_run_without_a_graph_give_the_same_bits():
    runs, again, eager = _runs()
    first = runs[_scene()[0]["seeds"].tolist()[0]]
    for other in (again, eager):
        for k, v in first.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v.view(np.int64) if v.dtype == np.float64 else v, other[k].view(np.int64) if v.dtype == np.float64 else other[k]), k
            else:
                assert v == other[k], k


def test_gpu_rooms_coverage_and_finishing_against_the_cpu_chain():
    """Coverage of every run at least the CPU chain's minimum over its seeds minus its spread (max - min), both as recorded; the
    fleet finishes (no frontier cell left for the closing plan) on every seed on which the CPU chain finishes -- all six --
    except at most one.  Not asserted: that every robot ends done (late INFEASIBLE turns are the known turn-on-the-spot limit)."""
    d, occ, cells = _scene()
    runs, _, _ = _runs()
    cpu = d["split_coverage"]
    bar = float(cpu.min() - (cpu.max() - cpu.min()))
    w_miss = int(d["weights"][1])
    cov = {s: float((r["evidence"][cells] <= -w_miss).sum() / cells.sum()) for s, r in runs.items()}
    origin, cell = tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    left = {}
    for s, r in runs.items():
        pos = r["X_pred"][:, -1][:, (0, 2)]
        left[s] = int(FR.plan_batch(r["evidence"], w_miss, int(d["weights"][0]), origin, cell, pos, int(d["r_inflate"]), int(d["min_unknown"]))["n_frontier"][0])
    print("coverage: device", {s: round(c, 4) for s, c in cov.items()}, "CPU chain", np.round(cpu, 4).tolist(), "bar", round(bar, 4))
    print("device: frontier cells left", left, "done", {s: r["done"].tolist() for s, r in runs.items()},
          "last status", {s: r["last_status"].tolist() for s, r in runs.items()}, "steps", {s: r["n_steps"].tolist() for s, r in runs.items()})
    assert all(c >= bar for c in cov.values()), (cov, bar)
    finished = [left[s] == 0 for s, ok in zip(d["seeds"].tolist(), d["split_finished"]) if ok]
    assert len(finished) - sum(finished) <= 1, left
