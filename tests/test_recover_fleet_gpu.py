"""GPU: the exploring fleet with recovery (UnknownEnvFleet(recover=).run_exploring) on the scenes of
tests/golden/exploration_recover.npz -- recorded on the CPU by tests/golden/make_exploration_recover.py, counts and bars in
EXPLORATION_RECOVER.md.  B = 3-4 robots, one shared map, one run per recorded noise seed with and without recovery:
recover = 0 is the fleet built without the argument, bit for bit; two runs and the run without a graph give the same bits; the
counters agree with the trajectory; a robot only ends in a failed solve after it ran out of capture steps or its capture point
was unsafe; failed robots and coverage are held against the CPU chain's; and where the CPU chain loses a robot on every seed
that recovery keeps, so does the device."""
import functools
import os

import numpy as np
import pytest

import field_oracle as FO
import lidar_split_oracle as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

SOLVED = (0, 4)                                               # STATUS_SOLVED, STATUS_UNCERTIFIED
HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _record():
    d = np.load(os.path.join(HERE, "golden", "exploration_recover.npz"))
    return d, [str(s) for s in d["scenes"]]


SCENES = ("field_edge", "field_corner", "field_middle", "field_rest", "rooms")


@functools.lru_cache(maxsize=None)
def _scene(name):
    d, names = _record()
    assert tuple(names) == SCENES
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    if str(d[f"{name}/map"]) == "rooms":
        occ, o2, c2 = S.rooms_scene(tuple(d["door"].tolist()))
        assert occ.shape == (W, H) and o2 == origin and c2 == cell
    else:
        walls = np.load(os.path.join(HERE, "golden", "exploration.npz"))["walls"]
        occ = np.zeros((W, H), np.uint8)
        for i0, j0, i1, j1 in walls:
            occ[i0:i1, j0:j1] = 1
    # the cells that count for the coverage: unblocked at r_inflate on the TRUE map and connected to the recorded cell
    blocked = FO.blocked_cells(occ, int(d["r_inflate"]))
    s = FO.cell_of(d["coverage_start"], origin, cell, W, H)
    seen, todo = {s}, [s]
    while todo:
        i, j = todo.pop()
        for a, b, _ in FO.moves_from(blocked, i, j):
            if (a, b) not in seen:
                seen.add((a, b))
                todo.append((a, b))
    cells = np.zeros((W, H), bool)
    cells[tuple(np.array(sorted(seen)).T)] = True
    return occ, cells


def _fleet(name, **kw):
    d, _ = _record()
    occ, _ = _scene(name)
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    rng = float(d["lidar_range"])
    mapper = lipmpc.OccupancyMapper(W, H, origin, cell, rng, w_hit=w_hit, w_miss=w_miss)          # one shared map
    fleet = lipmpc.UnknownEnvFleet(grid=lipmpc.GridMap(occ, origin, cell), N_horizon=3, lidar_range=rng, mapper=mapper,
                                   split_rays=int(d[f"{name}/split_rays"]), **kw)
    return fleet, mapper, lipmpc.FrontierPlanner(r_inflate=int(d["r_inflate"]), min_unknown=int(d["min_unknown"]))


def _explore(name, fleet, mapper, explorer, seed, **kw):
    d, _ = _record()
    starts, K = d[f"{name}/starts"], int(d[f"{name}/k_max"])
    B = len(starts)
    st = np.zeros((B, 5)); st[:, 0] = starts[:, 0]; st[:, 2] = starts[:, 1]
    # make_exploration_recover.noise_of: what the CPU chain of this seed read
    noise = torch.as_tensor(float(d["noise_std"]) * np.random.default_rng(seed).standard_normal((K, B, 360, 2)), device="cuda")
    mapper.reset()
    r = fleet.run_exploring(torch.as_tensor(st, device="cuda"), torch.ones((B,), dtype=torch.int8, device="cuda"), K, explorer,
                            int(d["replan_every"]), float(d["lookahead"]), noise=noise, **kw)
    torch.cuda.synchronize()
    out = {k: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
    out["evidence"] = mapper.evidence.cpu().numpy().copy()
    return out


@functools.lru_cache(maxsize=None)
def _runs(name):
    """Per recorded seed one run with the recorded max_recover, one with recover = 0 and one of a fleet built without the
    argument, and with recovery a second run of the same shape and one without a graph."""
    d, _ = _record()
    seeds = d["seeds"].tolist()
    on, off, plain = _fleet(name, recover=int(d["max_recover"])), _fleet(name, recover=0), _fleet(name)
    with_rec = {s: _explore(name, *on, s) for s in seeds}
    without = {s: _explore(name, *off, s) for s in seeds}
    return dict(on=with_rec, off=without, plain={s: _explore(name, *plain, s) for s in seeds}, again={s: _explore(name, *on, s) for s in seeds},
                eager={s: _explore(name, *on, s, use_graph=False) for s in seeds})


def _same_bits(a, b):
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v.view(np.int64) if v.dtype == np.float64 else v, b[k].view(np.int64) if v.dtype == np.float64 else b[k]), k
        else:
            assert v == b[k], k


def test_gpu_the_recorded_scenes_are_what_the_cpu_chain_ran():
    d, names = _record()
    assert tuple(names) == SCENES and int(d["max_recover"]) == 6 and len(d["seeds"]) == 6
    for name in SCENES:
        assert len(d[f"{name}/starts"]) in (3, 4)
        assert d[f"{name}/r0/n_recover"].sum() == 0 and d[f"{name}/r6/n_recover"].sum() > 0
        if name == "field_rest":                                  # the scene on which recovery does not help: a robot uses every capture step
            assert (d[f"{name}/r6/longest_run"] == 6).sum() >= 4 and np.array_equal(d[f"{name}/r6/n_failed"], d[f"{name}/r0/n_failed"])
        else:
            assert d[f"{name}/r6/n_failed"].sum() < d[f"{name}/r0/n_failed"].sum() and d[f"{name}/r6/longest_run"].max() <= 2
        if str(d[f"{name}/map"]) == "field":                     # the premise of a start set: every seed loses a robot without recovery
            assert (d[f"{name}/r0/n_failed"] >= 1).all()
    assert int(d["longest_run"]) <= int(d["max_recover"])


@pytest.mark.parametrize("name", SCENES)
def test_gpu_recover_0_is_the_fleet_without_the_argument(name):
    r = _runs(name)
    for s, x in r["plain"].items():
        _same_bits(x, r["off"][s])
    for x in list(r["off"].values()) + list(r["plain"].values()):    # ... which returns what it always did, and no more
        assert not {"n_recover", "recover_run", "recover_margin"} & set(x)
    assert all({"n_recover", "recover_run", "recover_margin"} <= set(x) for x in r["on"].values())


@pytest.mark.parametrize("name", SCENES)
def test_gpu_recover_two_runs_and_the_run_without_a_graph_give_the_same_bits(name):
    r = _runs(name)
    for s, first in r["on"].items():
        _same_bits(first, r["again"][s])
        _same_bits(first, r["eager"][s])


@pytest.mark.parametrize("name", SCENES)
def test_gpu_recover_counters_agree_with_the_trajectory(name):
    """n_recover = the X_pred rows that changed without n_steps rising (a solved sample and a recovery sample both move the
    state; nothing else does); and a robot that ends stopped with a failed status ran out of capture steps or its last capture
    point was unsafe."""
    d, _ = _record()
    max_recover = int(d["max_recover"])
    for mode in ("on", "off"):
        for seed, r in _runs(name)[mode].items():
            X = r["X_pred"]
            changed = (X[:, 1:] != X[:, :-1]).any(2).sum(1)
            n_recover = r["n_recover"] if mode == "on" else np.zeros_like(r["n_steps"])
            assert np.array_equal(n_recover, changed - r["n_steps"]), (mode, seed, n_recover, changed, r["n_steps"])
            if mode == "on":
                failed = (r["walking"] == 0) & ~np.isin(r["last_status"], SOLVED)
                print(f"{name} seed {seed}: n_recover {r['n_recover'].tolist()} margin {np.round(r['recover_margin'], 4).tolist()} "
                      f"last status {r['last_status'].tolist()} steps {r['n_steps'].tolist()}")
                assert ((r["recover_run"][failed] == max_recover) | (r["recover_margin"][failed] < 0)).all(), (seed, r["recover_run"], r["recover_margin"])


@pytest.mark.parametrize("name", SCENES)
def test_gpu_recover_failed_robots_and_coverage_against_the_cpu_chain(name):
    """Both bars are EXPLORATION_RECOVER.md's: failed robots per seed at most the CPU chain's largest count over its seeds, on
    all seeds but at most one; coverage of every run at least the CPU chain's smallest minus its spread."""
    d, _ = _record()
    _, cells = _scene(name)
    w_miss = int(d["weights"][1])
    runs = _runs(name)["on"]
    failed = {s: int((~np.isin(r["last_status"], SOLVED)).sum()) for s, r in runs.items()}
    bar = int(d[f"{name}/r6/n_failed"].max())
    cpu = d[f"{name}/r6/coverage"]
    cov_bar = float(cpu.min() - (cpu.max() - cpu.min()))
    cov = {s: float((r["evidence"][cells] <= -w_miss).sum() / cells.sum()) for s, r in runs.items()}
    print(f"{name}: failed robots device {failed} CPU chain {d[f'{name}/r6/n_failed'].tolist()} bar {bar}; coverage device "
          f"{ {s: round(c, 4) for s, c in cov.items()} } CPU chain {np.round(cpu, 4).tolist()} bar {cov_bar:.4f}")
    assert sum(n > bar for n in failed.values()) <= 1, (failed, bar)
    assert all(c >= cov_bar for c in cov.values()), (cov, cov_bar)


@pytest.mark.parametrize("name", SCENES)
def test_gpu_without_recovery_a_robot_is_lost_that_recovery_keeps(name):
    """Asserted where the CPU chain shows it on every seed; printed everywhere."""
    d, _ = _record()
    r = _runs(name)
    kept = {s: bool((~np.isin(r["off"][s]["last_status"], SOLVED) & np.isin(r["on"][s]["last_status"], SOLVED)).any()) for s in r["on"]}
    print(f"{name}: a robot lost without recovery and kept with it, per seed {kept}; the CPU chain on every seed: {bool(d[f'{name}/kept_every_seed'])}")
    if bool(d[f"{name}/kept_every_seed"]):
        assert all(kept.values()), kept
