"""Neighbour LDCBF rows on the device (lipmpc_neighbour_c_eta_batch, lipmpc.NeighbourRows, UnknownEnvFleet(avoid=)) against
the numpy restatement of the contract (tests/neighbour_oracle.py).

c_eta, n_rows, n_near and neighbours are compared BIT FOR BIT: every quantity is a float64 sum / product / quotient / square
root of the inputs evaluated as the contract writes it (NaN rows -- coincident robots -- are compared as NaN = NaN)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402
import lipmpc_oracle as O  # noqa: E402
import neighbour_oracle as NO  # noqa: E402
from helpers import raw_call  # noqa: E402
from neighbour_checks import assert_equals_oracle as _assert_equals_oracle, bits_equal as _bits_equal  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -7.25
E_ARG = -1
CELL = lambda R: R * (1.0 + 2.0 ** -20)          # the grid's cell width (csrc/lipmpc_neighbours.hip)


def _dev(a, dt):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _states(x, y):
    st = np.zeros((len(x), 5))
    st[:, 0], st[:, 2] = x, y
    st[:, 1], st[:, 3], st[:, 4] = 0.3, -0.2, 0.7            # never read
    return st


def _device_rows(st, radius, R, k_rows, n_obs_max, share=0.5, group=None, first_slot=None, prefill=SENTINEL):
    """(device outputs as numpy, oracle outputs) of one call on a c_eta prefilled with ``prefill``."""
    rad = radius if np.isscalar(radius) else _dev(radius, torch.float64)
    nb = lipmpc.NeighbourRows(rad, R, k_rows, share)
    before = np.full((len(st), n_obs_max, 4), prefill)
    ce = _dev(before, torch.float64)
    out = nb.append(_dev(st, torch.float64), ce, _dev(first_slot, torch.int32), _dev(group, torch.int32))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["c_eta"] = ce.cpu().numpy()
    ref = NO.neighbour_rows(st, radius, R, k_rows, n_obs_max, share, group, first_slot, c_eta=before)
    return got, ref


# ---- 1. random robots ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [257, 1, 2])
def test_random_robots_equal_the_oracle(B):
    rng = np.random.default_rng(B)
    st = _states(rng.uniform(0, 6, B), rng.uniform(0, 6, B)) if B > 2 else _states(rng.uniform(0, 0.5, B), rng.uniform(0, 0.5, B))
    first = rng.integers(0, 7, B).astype(np.int32)
    group = rng.integers(-1, 3, B).astype(np.int32) if B > 2 else np.zeros(B, np.int32)
    radius = rng.uniform(0.05, 0.3, B)
    got, ref = _device_rows(st, radius, 1.0, 4, 6, group=group, first_slot=first)
    _assert_equals_oracle(got, ref, f"B={B}")
    for b in range(B):                                       # slots below first_slot keep the sentinel; the rest are rows or zeros
        assert (got["c_eta"][b, : first[b]] == SENTINEL).all()
        assert not got["c_eta"][b, first[b] + got["n_rows"][b]:].any()
    if B == 257:
        assert (group < 0).sum() > 20 and not got["n_near"][group < 0].any()
        assert got["n_near"].max() > 4 and (got["n_rows"] < np.minimum(got["n_near"], 4)).any()      # k_rows and the slots both bind
    if B == 2:
        assert got["n_near"].tolist() == [1, 1]
    # the same robots without groups and first slots (NULL pointers), one radius for all
    got, ref = _device_rows(st, 0.2, 1.0, 4, 6)
    _assert_equals_oracle(got, ref, f"B={B}, NULL group / first_slot")


# ---- 2. edges --------------------------------------------------------------------------------------------------------
def _edge_batch():
    """One batch of edge cases, the cases far apart from each other (sense_range 1): returns (states, radius, named indices)."""
    R, w = 1.0, CELL(1.0)
    inside = np.nextafter(R, 0.0)
    x, y, rad, at = [], [], [], {}

    def add(name, pts, r=0.1):
        at[name] = list(range(len(x), len(x) + len(pts)))
        for p in pts:
            x.append(p[0]); y.append(p[1]); rad.append(r)

    # robots on exact multiples of the cell width and of the range, negative ones included, each with partners across the
    # cell boundary: one ulp below it, and 0.6 / 0.5 away along the axes and the diagonal
    for name, pitch, y0 in (("cell multiples", w, 0.0), ("range multiples", R, 50.0)):
        pts = []
        for i in range(-2, 3):
            for j in range(-2, 3):
                px, py = i * pitch, j * pitch
                pts += [(px, y0 + py), (np.nextafter(px, -np.inf), y0 + py), (px - 0.6, y0 + py), (px, y0 + py - 0.6), (px - 0.5, y0 + py - 0.5)]
        add(name, pts)
    add("exactly at range", [(0.0, 100.0), (R, 100.0), (0.0, 110.0), (0.0, 110.0 + R), (-R, 120.0), (0.0, 120.0)])
    add("one ulp inside", [(0.0, 130.0), (inside, 130.0), (-inside, 140.0), (0.0, 140.0), (500.0, 0.0), (500.0, -inside)])
    add("equidistant", [(0.5, 200.0), (0.0, 200.5), (-0.5, 200.0), (0.0, 199.5), (0.0, 200.0)])
    add("coincident", [(3.0, 300.0), (3.0, 300.0)])
    rng = np.random.default_rng(5)
    add("near 1e6", [(1e6 + a, -1e6 + b) for a, b in rng.uniform(-1.0, 1.0, (24, 2))])
    add("bad robots", [(0.2, 400.0), (np.nan, 400.0), (0.4, 400.0), (0.3, 400.2), (0.3, np.inf)])
    rad[at["bad robots"][2]] = -0.1
    return _states(x, y), np.array(rad), at


@pytest.mark.parametrize("k_rows", [2, 4])
def test_edges_equal_the_oracle(k_rows):
    st, rad, at = _edge_batch()
    got, ref = _device_rows(st, rad, 1.0, k_rows, 5)
    _assert_equals_oracle(got, ref, f"edges, k_rows={k_rows}")
    # what the oracle itself must say about them
    assert not ref["n_near"][at["exactly at range"]].any()                       # dist == sense_range: out
    assert (ref["n_near"][at["one ulp inside"]] == 1).all()                      # nextafter(sense_range, 0): in
    centre = at["equidistant"][4]
    assert ref["n_near"][centre] == 4 and ref["neighbours"][centre, :2].tolist() == at["equidistant"][:2]      # ties: by index
    a, b = at["coincident"]
    assert ref["n_rows"][[a, b]].tolist() == [1, 1] and np.isnan(got["c_eta"][[a, b], 0]).all()                  # NaN eta
    assert ref["n_near"][at["near 1e6"]].min() >= 1
    ok0, nan_x, neg_r, ok1, inf_y = at["bad robots"]
    assert ref["n_near"][[ok0, nan_x, neg_r, ok1, inf_y]].tolist() == [1, 0, 0, 1, 0] and ref["neighbours"][ok0, 0] == ok1
    for name in ("cell multiples", "range multiples"):                           # every lattice robot has its partner one ulp across
        assert (ref["n_near"][at[name]] >= 1).all()


# ---- 3. distinct cells share buckets ---------------------------------------------------------------------------------
def test_robots_alone_in_their_cells_share_buckets():
    """300 robots at the centres of distinct cells of a 400 x 400-cell area (cell centres are a cell width apart: out of range),
    far more cells than the 1024 buckets a batch of 300 gets; eight partners planted 0.6 cells from eight of them."""
    R, w, B = 1.0, CELL(1.0), 300
    rng = np.random.default_rng(11)
    cells = rng.choice(400 * 400, B - 8, replace=False)
    ci, cj = cells // 400 - 200, cells % 400 - 200
    x, y = list((ci + 0.5) * w), list((cj + 0.5) * w)
    for k in range(8):
        x.append(x[k] + (0.6 * w if k % 2 else 0.0) * (-1) ** (k // 2)); y.append(y[k] + (0.0 if k % 2 else 0.6 * w) * (-1) ** (k // 2))
    got, ref = _device_rows(_states(x, y), 0.2, R, 4, 6)
    _assert_equals_oracle(got, ref, "bucket sharing")
    assert (ref["n_near"][:8] >= 1).all() and (ref["n_near"][-8:] >= 1).all()
    lonely = np.ones(B, bool)
    lonely[ref["neighbours"][ref["neighbours"] >= 0]] = False
    assert lonely.sum() > 250 and not got["n_near"][lonely].any() and not got["c_eta"][lonely].any()


# ---- 4. a crowd in one cell ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_obs_max", [20, 4])
def test_a_crowd_in_one_cell(n_obs_max):
    rng = np.random.default_rng(4)
    st = _states(rng.uniform(0.1, 0.9, 64), rng.uniform(0.1, 0.9, 64))
    got, ref = _device_rows(st, 0.01, 1.5, 16, n_obs_max)
    _assert_equals_oracle(got, ref, f"crowd, n_obs_max={n_obs_max}")
    assert (got["n_near"] == 63).all() and (got["n_rows"] == min(16, n_obs_max)).all()


# ---- 5. determinism, graphs, refusals --------------------------------------------------------------------------------
def test_two_calls_give_identical_bits_and_a_graph_replays_on_new_states():
    B, R, k_rows, n_obs_max = 513, 1.0, 4, 6
    rng = np.random.default_rng(8)
    st = [_states(rng.uniform(0, 8, B), rng.uniform(0, 8, B)) for _ in range(2)]
    first = rng.integers(0, 4, B).astype(np.int32)
    nb = lipmpc.NeighbourRows(0.2, R, k_rows)
    d_st, d_first = _dev(st[0], torch.float64), _dev(first, torch.int32)
    ce = torch.full((B, n_obs_max, 4), SENTINEL, dtype=torch.float64, device="cuda")
    out = nb.alloc_outputs(B)
    snap = lambda: {k: v.cpu().numpy().copy() for k, v in dict(out, c_eta=ce).items()}
    nb.append(d_st, ce, d_first, out=out)
    one = snap()
    ce.fill_(SENTINEL)
    nb.append(d_st, ce, d_first, out=out)
    two = snap()
    for k in one:
        assert np.array_equal(one[k].view(np.int32), two[k].view(np.int32)), k
    _assert_equals_oracle(one, NO.neighbour_rows(st[0], 0.2, R, k_rows, n_obs_max, first_slot=first, c_eta=np.full((B, n_obs_max, 4), SENTINEL)))
    # captured, then replayed after the state tensor was overwritten
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nb.append(d_st, ce, d_first, out=out)
    d_st.copy_(_dev(st[1], torch.float64))
    ce.fill_(SENTINEL)
    for v in out.values():
        v.fill_(-5)
    graph.replay()
    torch.cuda.synchronize()
    _assert_equals_oracle(snap(), NO.neighbour_rows(st[1], 0.2, R, k_rows, n_obs_max, first_slot=first, c_eta=np.full((B, n_obs_max, 4), SENTINEL)),
                          "graph replay")


def test_every_refusal_returns_e_arg_and_touches_nothing():
    B, n_obs_max = 16, 6
    lib = lipmpc._lib.load()
    st = _dev(_states(np.linspace(0, 1, B), np.zeros(B)), torch.float64)
    rad = torch.full((B,), 0.1, dtype=torch.float64, device="cuda")
    ws = torch.empty((int(lib.lipmpc_neighbour_workspace_bytes(B)),), dtype=torch.uint8, device="cuda")
    ce = torch.full((B, n_obs_max, 4), SENTINEL, dtype=torch.float64, device="cuda")
    n_rows, n_near = (torch.full((B,), -5, dtype=torch.int32, device="cuda") for _ in range(2))
    good = dict(device=0, B=B, n_obs_max=n_obs_max, k_rows=4, sense_range=1.0, share=0.5)
    ptrs = dict(state=st.data_ptr(), radius=rad.data_ptr(), workspace=ws.data_ptr(), c_eta=ce.data_ptr(), n_rows=n_rows.data_ptr(),
                n_near=n_near.data_ptr())
    for bad in (dict(k_rows=0), dict(k_rows=17), dict(n_obs_max=0), dict(n_obs_max=51), dict(sense_range=0.0), dict(sense_range=-1.0),
                dict(sense_range=float("inf")), dict(sense_range=float("nan")), dict(share=-0.1), dict(share=1.1)):
        assert raw_call("lipmpc_neighbour_c_eta_batch", **{**good, **bad}, **ptrs) == E_ARG, bad
    for missing in ptrs:
        assert raw_call("lipmpc_neighbour_c_eta_batch", **good, **{k: v for k, v in ptrs.items() if k != missing}) == E_ARG, missing
    torch.cuda.synchronize()
    assert (ce == SENTINEL).all() and (n_rows == -5).all() and (n_near == -5).all()
    assert raw_call("lipmpc_neighbour_c_eta_batch", **good, **ptrs) == 0         # and the same call, complete, runs
    torch.cuda.synchronize()
    assert (n_near.cpu().numpy() == NO.neighbour_rows(st.cpu().numpy(), 0.1, 1.0, 4, n_obs_max)["n_near"]).all()


# ---- 6. behind the scanner's rows ------------------------------------------------------------------------------------
def test_rows_behind_a_scan_and_the_step_keeps_to_them():
    """64 robots on the CROWDED map: scan, then the neighbour rows from slot n_inferred on, then the step against both.  (On
    the oracle chain 46 of the 64 solve, the others overlap a neighbour's disc or an obstacle: tests need some, not all.)"""
    d = np.load(os.path.join(HERE, "golden", "lidar_golden.npz"))
    rings = [d["env"][0][j][: d["env_nv"][0][j]] for j in range(d["env"].shape[1]) if d["env_nv"][0][j] > 0]
    rng = np.random.default_rng(6)
    pos = []
    while len(pos) < 64:
        p = rng.uniform(-0.5, 5.5, 2)
        if not any(O.point_in_ring(p, r) for r in rings):
            pos.append(p)
    pos = np.array(pos)
    B, N, n_obs_max, radius, R, k_rows = 64, 3, 12, 0.1, 1.0, 4
    st = np.zeros((B, 5)); st[:, 0], st[:, 2], st[:, 4] = pos[:, 0], pos[:, 1], rng.uniform(-3, 3, B)
    d_st = _dev(st, torch.float64)
    sensor = lipmpc.LidarSensor(rings, lidar_range=1.5, n_obs_max=n_obs_max, v_max=32)
    sen = sensor.sense(d_st, None, c_eta=True, rings=False)
    scan = sen["c_eta"].cpu().numpy().copy()
    n_inf = sen["n_inferred"].cpu().numpy()
    nbr = lipmpc.NeighbourRows(radius, R, k_rows).append(d_st, sen["c_eta"], first_slot=sen["n_inferred"])
    sv = lipmpc.BatchedLipMpc(lipmpc.LipMpcParams(N=N, n_obs_max=n_obs_max, v_max=32))
    goal = torch.tensor([[5.0, 5.0]], dtype=torch.float64, device="cuda").repeat(B, 1).contiguous()
    out = sv.plan_step_batch_c_eta(d_st, goal, torch.ones((B,), dtype=torch.int8, device="cuda"), sen["c_eta"], overflow=sen["overflow"])
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in nbr.items()}
    got["c_eta"] = sen["c_eta"].cpu().numpy()
    ref = NO.neighbour_rows(st, radius, R, k_rows, n_obs_max, first_slot=n_inf, c_eta=scan)
    _assert_equals_oracle(got, ref, "behind a scan")
    for b in range(B):                                       # the scan's rows are where they were, the neighbours' follow
        f = min(int(n_inf[b]), n_obs_max)
        assert _bits_equal(got["c_eta"][b, :f], scan[b, :f])
    status, X = out["status"].cpu().numpy(), out["X"].cpu().numpy()
    ok = np.isin(status, (lipmpc.STATUS_SOLVED, lipmpc.STATUS_UNCERTIFIED))
    assert (ok & (got["n_rows"] > 0)).sum() >= 16, status
    worst = 0.0
    for b in np.nonzero(ok)[0]:
        rows = got["c_eta"][b][(got["c_eta"][b, :, 2:] != 0).any(1)]
        p = X[b][:, [0, 2]]                                  # predicted CoM, stages 0..N
        slack = np.einsum("krd,rd->kr", p[:, None, :] - rows[None, :, :2], rows[:, 2:])          # eta.(p_k - c), every stage and row
        worst = min(worst, float(slack.min())) if rows.size else worst
    print("rows behind a scan:", int(ok.sum()), "of", B, "solved; smallest eta.(p_k - c) =", worst)
    assert worst >= -1e-9


# ---- 7. the swap, closed loop ----------------------------------------------------------------------------------------
FAR_OBSTACLE = [np.array([[100.0, 100.0], [101.0, 100.0], [101.0, 101.0], [100.0, 101.0]])]      # out of every scan's range
K_MAX = 80


def _swap_inputs():
    st, goal = NO.swap_scenario()
    return _dev(st, torch.float64), _dev(goal, torch.float64), torch.ones((4,), dtype=torch.int8, device="cuda"), goal


def _host_loop(fleet, st0, goal, foot):
    """The fleet's sample as a host loop of the four public calls."""
    B = st0.shape[0]
    sn, sv, avoid = fleet.sensor, fleet.solver, fleet.avoid
    table = lipmpc.solver.fleet_state(B, K_MAX)
    fl = {k: torch.zeros(shape, dtype=dt, device="cuda") for k, (dt, shape, _) in table.items()}
    fl["state"].copy_(st0); fl["first_foot"].copy_(foot); fl["walking"].fill_(1); fl["last_obj"].fill_(float("inf"))
    fl["X_pred"][:, 0] = st0
    n_crowded = torch.zeros((B,), dtype=torch.int32, device="cuda")
    for _ in range(K_MAX):
        sen = sn.sense(fl["state"], None, c_eta=True, rings=False)
        nbr = avoid.append(fl["state"], sen["c_eta"], first_slot=sen["n_inferred"])
        out = sv.plan_step_batch_c_eta(fl["state"], goal, fl["first_foot"], sen["c_eta"], overflow=sen["overflow"])
        sv.fleet_update(fl, out, overflow=sen["overflow"])
        n_crowded += nbr["n_near"] > nbr["n_rows"]
    torch.cuda.synchronize()
    return fl, n_crowded


def test_swap_closed_loop_keeps_the_robots_apart():
    st0, goal, foot, goal_np = _swap_inputs()
    runs = {}
    for use_graph in (True, False):
        fleet = lipmpc.UnknownEnvFleet(FAR_OBSTACLE, N_horizon=3, avoid=lipmpc.NeighbourRows(0.25, 1.5, 4))
        r = fleet.run(st0, goal, foot, K_MAX, noise=None, use_graph=use_graph)
        torch.cuda.synchronize()
        assert set(r) == {"X_pred", "U_pred", "n_steps", "last_status", "overflow", "n_crowded"}
        runs[use_graph] = {k: v.cpu().numpy().copy() for k, v in r.items()}
    fl, n_crowded = _host_loop(fleet, st0, goal, foot)
    X = runs[True]["X_pred"]
    assert np.array_equal(X, runs[False]["X_pred"]) and np.array_equal(X, fl["X_pred"].cpu().numpy())
    assert np.array_equal(runs[True]["n_steps"], fl["n_steps"].cpu().numpy())
    r = runs[True]
    d = NO.min_pair_distance(X)
    left = np.linalg.norm(X[:, -1][:, [0, 2]] - goal_np, axis=1)
    print("swap with neighbour rows: min distance", d, "steps", r["n_steps"], "status", r["last_status"], "left to the goal", left)
    # all four stop on the objective: no failed solve, samples to spare, and at the goal (the objective's k = 0 term < 0.05)
    assert (r["last_status"] == lipmpc.STATUS_SOLVED).all() and (r["n_steps"] < K_MAX).all() and (left ** 2 < 0.05).all()
    assert not r["n_crowded"].any() and not n_crowded.cpu().numpy().any() and not r["overflow"].any()
    assert d >= 0.5 - 1e-9                                   # the contract's derivation (the oracle's run gives 0.5316)


def test_swap_closed_loop_without_rows_walks_through():
    st0, goal, foot, goal_np = _swap_inputs()
    fleet = lipmpc.UnknownEnvFleet(FAR_OBSTACLE, N_horizon=3)
    r = fleet.run(st0, goal, foot, K_MAX, noise=None)
    torch.cuda.synchronize()
    assert set(r) == {"X_pred", "U_pred", "n_steps", "last_status", "overflow"}          # avoid=None: nothing changes
    d = NO.min_pair_distance(r["X_pred"].cpu().numpy())
    print("swap without rows: min distance", d)
    assert d < 0.5                                           # (the oracle's run gives 0.145)
