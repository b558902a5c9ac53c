"""RRT* sub-goal planner on the device (lipmpc_rrt_plan_batch, lipmpc.RrtStarPlanner) against the scipy golden grids
(tests/golden/rrt_grid_golden.npz), the numpy restatement of the contract (tests/rrt_oracle.py) and the closed loop.

The tree is compared BIT FOR BIT with the oracle fed the device's cost grid C: every quantity the tree compares is an
integer or a sum / product / correctly rounded sqrt of exact inputs, and only exp (C itself) may differ in the last bit
between the device and numpy, which is why C is held to 2 ulp separately."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402
import rrt_oracle as R  # noqa: E402
from rrt_checks import check_ring_plan  # noqa: E402
from helpers import IPOPT_LIKE_TOL  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = ("SimulationRRT", "SimulationMaze1", "SimulationMaze2")
# the first two seeds of 0..15 that arrive through the oracle chain (tests/golden/RRT_PLANNER.md, make_rrt_arrival.py)
ARRIVING = {"SimulationRRT": (4, 6), "SimulationMaze1": (0, 1), "SimulationMaze2": (1, 2)}


def _scene(name):
    sc = np.load(os.path.join(HERE, "golden", "pdf_scenarios.npz"))
    rings = [sc[name + "/rings"][j][: sc[name + "/nv"][j]] for j in range(len(sc[name + "/nv"]))]
    return rings, np.asarray(sc[name + "/goal"], float)


def _golden():
    d = np.load(os.path.join(HERE, "golden", "rrt_grid_golden.npz"))
    sets = []
    for s, name in enumerate(d["names"]):
        dims = tuple(int(v) for v in d["dims"][s])
        og = np.unpackbits(d["occ_packed"][d["occ_off"][s]: d["occ_off"][s + 1]])[: dims[0] * dims[1]].reshape(dims)
        d2 = np.cumsum(d["d2_dy"][d["d2_off"][s]: d["d2_off"][s + 1]].reshape(dims).astype(np.int64), axis=1)
        rings = [d["rings"][s, j, : d["nv"][s, j]] for j in range(d["nv"].shape[1]) if d["nv"][s, j] > 0]
        sets.append(dict(name=str(name), rings=rings, goal=d["goal"][s], bounds=d["bounds"][s], dims=dims,
                         og=og.astype(bool), d2=d2))
    return sets


def _pack(problems, n_obs=None, v_max=None):
    n_obs = n_obs or max(1, max(len(p["rings"]) for p in problems))
    v_max = v_max or max([3] + [len(r) for p in problems for r in p["rings"]])
    return lipmpc.pack_rings([p["rings"] for p in problems], n_obs, v_max)


def _plan(planner, problems, S_max=None, with_grids=False, n_obs=None, v_max=None):
    xy, nv = _pack(problems, n_obs, v_max)
    start = np.array([p.get("start", (0.0, 0.0)) for p in problems], float)
    out = planner.plan_batch(np.array([p["goal"] for p in problems], float), xy, nv, start=start,
                             seeds=[p["seed"] for p in problems], S_max=S_max, with_tree=True, with_grids=with_grids)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ulp_diff(a, b):
    ia, ib = a.view(np.int64), b.view(np.int64)
    return np.abs(ia - ib)


def test_grid_and_distance_match_golden():
    """Device occupancy and d2 equal scipy's (the reference's Delaunay.find_simplex / distance_transform_edt) bit for bit
    on the four scenes and 24 random sets; C within 2 ulp of np.exp(-np.sqrt(d2))."""
    sets = _golden()
    planner = lipmpc.RrtStarPlanner()
    out = _plan(planner, [dict(s, seed=1) for s in sets], with_grids=True)
    for b, s in enumerate(sets):
        W1, H1 = s["dims"]
        assert tuple(out["grid_dims"][b]) == (W1, H1), s["name"]
        d2 = out["occ_d2"][b, : W1 * H1].reshape(W1, H1)
        assert np.array_equal(d2 == 0, s["og"]), (s["name"], int(np.sum((d2 == 0) != s["og"])))
        assert np.array_equal(d2, s["d2"]), (s["name"], int(np.sum(d2 != s["d2"])))
        C = out["cost_grid"][b, : W1 * H1]
        ulp = _ulp_diff(C, np.exp(-np.sqrt(s["d2"].reshape(-1).astype(np.float64))))
        print(f"{s['name']}: C max ulp {int(ulp.max())}")
        assert ulp.max() <= 2, (s["name"], int(ulp.max()))


def _check_against_oracle(res, b, prob, n, S_max, label):
    """Problem b against the oracle on the device's C: everything tests/rrt_checks.py holds a plan to."""
    return check_ring_plan(res, b, prob, label, S_max=S_max, n=n)


def _random_problems(count, rng):
    """Random obstacle sets and goals, the starts partly off the origin; the first ones are the special cases."""
    probs = []
    for i in range(count):
        rings = []
        for _ in range(int(rng.integers(1, 8))):
            c = rng.uniform(-1.0, 7.0, 2)
            rad = rng.uniform(0.03, 1.5) if i % 3 else rng.uniform(0.03, 0.12)
            ang = np.sort(rng.uniform(0, 2 * np.pi, int(rng.integers(3, 9))))
            rings.append(c + rad * np.stack([np.cos(ang), np.sin(ang)], 1))
        start = (0.0, 0.0) if i % 2 else tuple(rng.uniform(-1.0, 7.0, 2))
        probs.append(dict(rings=rings, goal=rng.uniform(-1.0, 7.0, 2), start=start,
                          seed=int(rng.integers(0, 2 ** 63)) * 2 + 1))
    box = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], float)
    walls = [box(3, 3, 5, 3.3), box(3, 4.7, 5, 5), box(3, 3, 3.3, 5), box(4.7, 3, 5, 5)]
    probs[0].update(rings=[box(-0.5, -0.5, 0.5, 0.5), box(2, 2, 3, 3)], start=(0.0, 0.0))    # start occupied
    probs[1].update(rings=[box(2, 2, 3, 3)], goal=np.array([2.5, 2.5]))                     # goal occupied
    probs[2].update(rings=walls, goal=np.array([4.0, 4.0]), start=(0.0, 0.0))              # goal walled in: no path
    probs[3].update(rings=[box(1, 1, 1.5, 1.5)], goal=np.array([0.0, 400.0]))              # grid over max_cells
    probs[4].update(rings=[], goal=np.array([3.0, 2.0]))                                  # no obstacle at all
    probs[5].update(seed=2 ** 64 - 1)
    return probs


def test_tree_parity_scenes_full_size():
    """The three RRT scenes x seeds 0..3 at the reference's sizes: vertex list, parents, costs (bitwise), status, n_sub and
    sub-goals equal the oracle's on the device's C; vertex counts and n_sub as the contract's table."""
    probs = [dict(zip(("rings", "goal"), _scene(n)), seed=s, name=n) for n in SCENES for s in range(4)]
    planner = lipmpc.RrtStarPlanner()
    res = _plan(planner, probs, with_grids=True)
    table = {"SimulationRRT": ([1478, 1477, 1471, 1490], [35, 43, 36, 29]),
             "SimulationMaze1": ([331, 311, 297, 328], [7, 6, 5, 7]),
             "SimulationMaze2": ([366, 347, 317, 353], [13, 8, 12, 12])}
    for b, p in enumerate(probs):
        _check_against_oracle(res, b, p, 1500, 1501, (p["name"], p["seed"]))
        assert res["status"][b] == R.FOUND
        assert int(res["tree"][b, 0, 0]) == table[p["name"]][0][p["seed"]]
        assert res["n_sub"][b] == table[p["name"]][1][p["seed"]]


def test_tree_parity_random_small():
    """64 random problems at n = 200 (occupied start / goal, no path, a grid over max_cells, no obstacle, a seed of
    2^64 - 1, starts off the origin, S_max = 12 so that long paths overflow) against the oracle."""
    probs = _random_problems(64, np.random.default_rng(11))
    planner = lipmpc.RrtStarPlanner(n=200)
    res = _plan(planner, probs, S_max=12, with_grids=True, n_obs=8, v_max=8)
    seen = set()
    for b, p in enumerate(probs):
        o = _check_against_oracle(res, b, p, 200, 12, ("random", b))
        seen.add(o["status"])
    assert res["status"][0] == R.START_OCCUPIED and res["status"][1] == R.GOAL_OCCUPIED
    assert res["status"][2] == R.NO_PATH and res["status"][3] == R.GRID_TOO_LARGE
    assert res["status"][4] == R.NO_OBSTACLE_GRID
    assert R.FOUND in seen
    print("statuses:", sorted(R.STATUS_NAMES[s] for s in seen))


def _mixed_batch(core, fill, B, rng):
    """core problems at random positions of a batch of B, the rest drawn from fill."""
    pos = rng.permutation(B)[: len(core)]
    batch = [fill[int(rng.integers(0, len(fill)))] for _ in range(B)]
    for i, p in zip(pos, core):
        batch[i] = p
    return batch, pos


def _same(a, b, i, j, keys=("status", "n_sub", "sub_goals", "path_cost", "tree")):
    for k in keys:
        x, y = np.ascontiguousarray(a[k][i]), np.ascontiguousarray(b[k][j])
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (k, i, j)


def test_batch_independence():
    """Every problem of the two parity tests gives bit-identical output alone and inside a batch of 1024 mixed with other
    scenes, seeds and sizes; two launches of the batch are identical."""
    rng = np.random.default_rng(5)
    scenes = [dict(zip(("rings", "goal"), _scene(n)), seed=s) for n in SCENES for s in range(4)]
    circles = dict(zip(("rings", "goal"), _scene("Simulation1Circles")), seed=3)
    fill = ([dict(zip(("rings", "goal"), _scene(n)), seed=int(rng.integers(0, 10 ** 6))) for n in SCENES for _ in range(8)]
            + [circles] + _random_problems(24, np.random.default_rng(12))[6:])
    for n, core, S_max in ((1500, scenes, 64), (200, _random_problems(64, np.random.default_rng(11)), 12)):
        planner = lipmpc.RrtStarPlanner(n=n)
        batch, pos = _mixed_batch(core, fill, 1024, rng)
        a = _plan(planner, batch, S_max=S_max, n_obs=9, v_max=24)
        b = _plan(planner, batch, S_max=S_max, n_obs=9, v_max=24)
        for k in a:
            assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k
        for i, p in zip(pos, core):
            alone = _plan(planner, [p], S_max=S_max)
            _same(a, alone, i, 0)


def test_end_to_end_class():
    """HumanoidMPCWithRRT(planner=RrtStarPlanner(seed=s)) on each scene with the first two arriving seeds of the oracle
    chain: its sub-goals equal the oracle plan's, and the robot ends within 0.2 m of the goal cell."""
    kw = dict(N_horizon=3, N_mpc_timesteps=300, sampling_time=0.4)
    for name in SCENES:
        rings, goal = _scene(name)
        for seed in ARRIVING[name]:
            pl = lipmpc.RrtStarPlanner(seed=seed)
            dbg = pl.plan(goal, rings, with_grids=True)
            W1, H1 = (int(v) for v in dbg["grid_dims"][0].cpu())
            o = R.plan(rings, goal, seed=seed, C=dbg["cost_grid"][0, : W1 * H1].cpu().numpy().reshape(W1, H1))
            mpc = lipmpc.HumanoidMPCWithRRT(goal=goal, obstacles=rings, planner=pl, verbosity=0, **kw)
            X, _, _ = mpc.run_simulation(None)
            subs = pl.last["sub_goals"][0, : int(pl.last["n_sub"][0])].cpu().numpy()
            assert np.array_equal(subs, o["sub_goals"]), (name, seed)
            d = float(np.hypot(X[0, -1] - subs[-1, 0], X[2, -1] - subs[-1, 1]))
            print(f"{name} seed {seed}: {len(subs)} sub-goals, final distance {d:.4f} m")
            assert d < 0.2, (name, seed, d)


def test_plan_then_walk_batch():
    """plan_batch -> rollout_subgoals for 64 robots with different goals in the Maze1 map matches the class robot by robot
    (1e-5, the bar of the existing sub-goal test), whether a robot arrives or not."""
    rings, _ = _scene("SimulationMaze1")
    rng = np.random.default_rng(3)
    lo, hi = np.min(np.concatenate(rings), 0), np.max(np.concatenate(rings), 0)
    goals = []
    while len(goals) < 64:
        g = rng.uniform(lo, hi)
        if not any(_inside(g, r) for r in rings):
            goals.append(g)
    goals = np.array(goals)
    B = 64
    planner = lipmpc.RrtStarPlanner()
    v_max = max(len(r) for r in rings)
    xy, nv = lipmpc.pack_rings([rings] * B, len(rings), v_max)
    out = planner.plan_batch(goals, xy, nv, seeds=np.arange(B) + 100, S_max=48)
    torch.cuda.synchronize()
    st, n_sub = out["status"].cpu().numpy(), out["n_sub"].cpu().numpy()
    ok = np.nonzero(st == lipmpc.RRT_FOUND)[0]
    assert len(ok) >= B // 2, st
    S = int(n_sub.max())
    P = lipmpc.LipMpcParams(N=3, n_obs_max=len(rings), v_max=v_max, flags=lipmpc.FLAG_INTERIOR, tol_interior=IPOPT_LIKE_TOL,
                            sampling_time=0.4)
    sv = lipmpc.BatchedLipMpc(P)
    dev = torch.device("cuda")
    idx = torch.as_tensor(ok, device=dev)
    sg = out["sub_goals"][:, :S].index_select(0, idx).contiguous()
    ro = sv.rollout_subgoals(torch.zeros((len(ok), 5), dtype=torch.float64, device=dev), sg, out["n_sub"].index_select(0, idx),
                             torch.ones((len(ok),), dtype=torch.int8, device=dev),
                             torch.as_tensor(xy[ok], device=dev), torch.as_tensor(nv[ok], device=dev), None, k_max=300,
                             mpc_step=1)
    torch.cuda.synchronize()
    nk, Xb = ro["n_kept"].cpu().numpy(), ro["X_pred"].cpu().numpy()
    subs_all = out["sub_goals"].cpu().numpy()
    arrived, stopped = 0, 0
    for i, b in enumerate(ok):
        subs = subs_all[b, : n_sub[b]]
        mpc = lipmpc.HumanoidMPCWithRRT(goal=goals[b], obstacles=rings, sub_goals=subs, N_horizon=3, N_mpc_timesteps=300,
                                        sampling_time=0.4, verbosity=0)
        X, _, _ = mpc.run_simulation(None)
        ran = [s for s in range(n_sub[b]) if nk[i, s] >= 0]
        cat = np.concatenate([Xb[i, s, : nk[i, s] + 1].T for s in ran], axis=1)
        if len(ran) < n_sub[b]:
            # a failed solve ends the robot's batched walk (rollout_subgoals); the class goes on with the next sub-goal
            assert int(ro["last_status"][i]) not in (lipmpc.STATUS_SOLVED, lipmpc.STATUS_UNCERTIFIED), b
            X = X[:, : cat.shape[1]]
            stopped += 1
        assert cat.shape == X.shape, (b, cat.shape, X.shape)
        assert np.max(np.abs(cat - X)) < 1e-5, b
        arrived += np.hypot(X[0, -1] - subs[-1, 0], X[2, -1] - subs[-1, 1]) < 0.2
    print(f"{len(ok)} robots planned, {arrived} arrive, {stopped} stopped by a failed solve")


def _inside(p, ring):
    r = np.asarray(ring, float)
    e = np.roll(r, -1, 0) - r
    return bool(np.all(e[:, 0] * (p[1] - r[:, 1]) - e[:, 1] * (p[0] - r[:, 0]) >= 0))


def test_without_obstacle_slots():
    """No obstacle slots at all (obs_xy = None): NO_OBSTACLE_GRID, d2 = -1 on every cell, no sub-goal; the planner as the
    class's planner raises."""
    pl = lipmpc.RrtStarPlanner(n=50)
    out = pl.plan_batch(np.array([[3.0, 2.0], [1.0, -1.0]]), None, None, with_grids=True, with_tree=True)
    torch.cuda.synchronize()
    W1, H1 = (int(v) for v in out["grid_dims"][0].cpu())
    assert out["status"].cpu().tolist() == [R.NO_OBSTACLE_GRID] * 2 and out["n_sub"].cpu().tolist() == [0, 0]
    assert bool((out["occ_d2"][0, : W1 * H1] == -1).all())
    with pytest.raises(RuntimeError):
        pl(lipmpc.HumanoidMPCWithRRT(goal=(3.0, 2.0), obstacles=[], verbosity=0))
