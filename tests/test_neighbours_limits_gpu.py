"""Neighbour LDCBF rows on the device at the limits of their grid, sort and doubles: the cases of tests/neighbour_cases.py
(ranges that are not 1, the +-2^30 cell clamp, the 2^-500 floor, w = inf, subnormal and overflowing d2, ties in a full list,
colliding buckets, first_slot outside its range, batches above 2^12 and 2^16 robots), two streams on one object, a graph
replayed after an eager call, and a fleet in which n_crowded counts.  Every comparison is bit for bit
(neighbour_checks.assert_equals_oracle); tests/test_neighbour_cases_oracle.py shows that each case is what it claims."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402
import neighbour_cases as NC  # noqa: E402
import neighbour_oracle as NO  # noqa: E402
from neighbour_checks import assert_equals_oracle  # noqa: E402

SENTINEL = -7.25


def _dev(a, dt):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


@functools.lru_cache(maxsize=None)
def _solved(name):
    """(case, oracle outputs on a c_eta prefilled with the sentinel): computed once, shared, never written."""
    case = NC.large() if name == "large" else NC.CASES[name]()
    oracle = NO.neighbour_rows_sweep if name == "large" else NO.neighbour_rows
    before = np.full((len(case["state"]), case["n_obs_max"], 4), SENTINEL)
    return case, oracle(**NC.call_args(case), c_eta=before)


def _rows_object(case):
    rad = case["radius"]
    return lipmpc.NeighbourRows(rad if np.isscalar(rad) else _dev(rad, torch.float64), case["sense_range"], case["k_rows"], case["share"])


def _inputs(case):
    B = len(case["state"])
    return dict(state=_dev(case["state"], torch.float64), first_slot=_dev(case["first_slot"], torch.int32),
                group=_dev(case["group"], torch.int32),
                c_eta=torch.full((B, case["n_obs_max"], 4), SENTINEL, dtype=torch.float64, device="cuda"))


def _append(nb, case, inp, out=None):
    out = nb.alloc_outputs(len(case["state"]), with_neighbours=case["with_neighbours"]) if out is None else out
    return nb.append(inp["state"], inp["c_eta"], inp["first_slot"], inp["group"], out=out)


def _download(out, inp):
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["c_eta"] = inp["c_eta"].cpu().numpy()
    return got


def _check(got, case, ref, what):
    assert_equals_oracle(got, ref, what, without=() if case["with_neighbours"] else ("neighbours",))
    if case["first_slot"] is not None:                       # slots below the clamped first_slot still hold the sentinel
        first = np.clip(case["first_slot"].astype(np.int64), 0, case["n_obs_max"])
        below = np.arange(case["n_obs_max"])[None, :] < first[:, None]
        assert (got["c_eta"][below] == SENTINEL).all() and (got["c_eta"][~below] != SENTINEL).all(), what


# ---- 1. every case ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NC.CASES))
def test_a_case_equals_the_oracle(name):
    case, ref = _solved(name)
    nb, inp = _rows_object(case), _inputs(case)
    out = _append(nb, case, inp)
    torch.cuda.synchronize()
    got = _download(out, inp)
    print(name, "B", len(ref["n_near"]), "n_near", ref["n_near"].min(), "..", ref["n_near"].max())
    _check(got, case, ref, name)
    if name == "collisions":
        # the kernel's own buckets, from the workspace (int32 [B] behind the bucket table and the allocator's 256 bytes):
        # the cases aim at colliding buckets with a restated hash, and a hash that changed must fail here, not empty the case
        B, n = len(case["state"]), NC.n_buckets(len(case["state"]))
        (ws, _), = nb._ws_by_stream.values()
        offset = ((n * 8 + 255) & ~255) + 256
        assert nb.lib.lipmpc_neighbour_workspace_bytes(B) > offset + 4 * B
        bucket = ws[offset: offset + 4 * B].view(torch.int32).cpu().numpy()
        assert bucket.tolist() == NC.buckets(case).tolist()


# ---- 2. above 2^16 robots --------------------------------------------------------------------------------------------
def test_the_large_case_equals_the_sweep_oracle_twice():
    case, ref = _solved("large")
    nb, inp = _rows_object(case), _inputs(case)
    out = _append(nb, case, inp)
    torch.cuda.synchronize()
    one = _download(out, inp)
    _check(one, case, ref, "large")
    inp["c_eta"].fill_(SENTINEL)
    for v in out.values():
        v.fill_(-5)
    _append(nb, case, inp, out)
    torch.cuda.synchronize()
    two = _download(out, inp)
    for k in one:
        assert np.array_equal(one[k].view(np.int32), two[k].view(np.int32)), k


# ---- 3. streams and graphs on one object -----------------------------------------------------------------------------
def test_two_streams_share_one_object():
    """Batches of 4099 and of 300 robots on two streams, nothing between them, three times over: the object keeps a workspace
    per stream, so neither batch sorts in the other's table."""
    cases = [_solved("batch 4099"), _solved("batch 300")]
    nb = _rows_object(cases[0][0])
    streams = [torch.cuda.Stream() for _ in cases]
    runs = [[_inputs(case) for _ in range(3)] for case, _ in cases]
    outs = [[nb.alloc_outputs(len(case["state"])) for _ in range(3)] for case, _ in cases]
    torch.cuda.synchronize()
    for rep in range(3):
        for k, (case, _) in enumerate(cases):
            with torch.cuda.stream(streams[k]):
                _append(nb, case, runs[k][rep], outs[k][rep])
    torch.cuda.synchronize()
    assert len(nb._ws_by_stream) == 2
    for rep in range(3):
        for k, (case, ref) in enumerate(cases):
            _check(_download(outs[k][rep], runs[k][rep]), case, ref, f"stream {k}, repetition {rep}")


def test_a_graph_replays_after_a_larger_eager_call():
    """Captured at 300 robots, replayed after an eager call at 4099 on the same object: the captured call keeps a workspace
    of its own, which the eager call's larger one does not replace."""
    (big, big_ref), (small, small_ref) = _solved("batch 4099"), _solved("batch 300")
    nb = _rows_object(small)
    s_in, b_in = _inputs(small), _inputs(big)
    s_out = _append(nb, small, s_in)                         # (the first call of a batch size fills its radius tensor)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _append(nb, small, s_in, s_out)
    b_out = _append(nb, big, b_in)
    s_in["c_eta"].fill_(SENTINEL)
    for v in s_out.values():
        v.fill_(-5)
    graph.replay()
    torch.cuda.synchronize()
    _check(_download(b_out, b_in), big, big_ref, "eager, 4099 robots")
    _check(_download(s_out, s_in), small, small_ref, "replayed, 300 robots")


# ---- 4. a fleet in which n_crowded counts ----------------------------------------------------------------------------
FAR_OBSTACLE = [np.array([[0.0, 1000.0], [1.0, 1000.0], [1.0, 1001.0], [0.0, 1001.0]])]          # out of every scan's range
K_MAX = 80


def test_a_crowded_fleet_counts_and_agrees_with_its_host_loop():
    """Twenty swaps of four robots, 100 m apart (80 robots: more than a wave), one row per robot: at each crossing a robot has
    up to three neighbours in range and a row for one.  Graph, eager and host loop agree bit for bit, every sample's rows are
    the oracle's, and n_crowded counts.  With one row the robots are not kept apart: the distance is printed, not asserted."""
    copies = [NO.swap_scenario(seed=k) for k in range(20)]
    st0 = np.concatenate([st + np.array([100.0 * k, 0, 0, 0, 0]) for k, (st, _) in enumerate(copies)])
    goal = np.concatenate([g + np.array([100.0 * k, 0]) for k, (_, g) in enumerate(copies)])
    B = len(st0)
    d_st0, d_goal, foot = _dev(st0, torch.float64), _dev(goal, torch.float64), torch.ones((B,), dtype=torch.int8, device="cuda")
    runs = {}
    for use_graph in (True, False):
        fleet = lipmpc.UnknownEnvFleet(FAR_OBSTACLE, N_horizon=3, avoid=lipmpc.NeighbourRows(0.25, 1.5, k_rows=1))
        r = fleet.run(d_st0, d_goal, foot, K_MAX, noise=None, use_graph=use_graph)
        torch.cuda.synchronize()
        runs[use_graph] = {k: v.cpu().numpy().copy() for k, v in r.items()}
    # the host loop of the four public calls, every sample's rows against the oracle
    sn, sv, avoid = fleet.sensor, fleet.solver, fleet.avoid
    table = lipmpc.solver.fleet_state(B, K_MAX)
    fl = {k: torch.zeros(shape, dtype=dt, device="cuda") for k, (dt, shape, _) in table.items()}
    fl["state"].copy_(d_st0); fl["first_foot"].copy_(foot); fl["walking"].fill_(1); fl["last_obj"].fill_(float("inf"))
    fl["X_pred"][:, 0] = d_st0
    n_crowded = np.zeros(B, np.int64)
    for k in range(K_MAX):
        sen = sn.sense(fl["state"], None, c_eta=True, rings=False)
        st, scan, n_inf = fl["state"].cpu().numpy(), sen["c_eta"].cpu().numpy(), sen["n_inferred"].cpu().numpy()
        nbr = avoid.append(fl["state"], sen["c_eta"], first_slot=sen["n_inferred"])
        out = sv.plan_step_batch_c_eta(fl["state"], d_goal, fl["first_foot"], sen["c_eta"], overflow=sen["overflow"])
        sv.fleet_update(fl, out, overflow=sen["overflow"])
        got = {name: v.cpu().numpy() for name, v in nbr.items()}
        got["c_eta"] = sen["c_eta"].cpu().numpy()
        ref = NO.neighbour_rows(st, 0.25, 1.5, 1, scan.shape[1], first_slot=n_inf, c_eta=scan)
        assert_equals_oracle(got, ref, f"sample {k}")
        n_crowded += ref["n_near"] > ref["n_rows"]
    torch.cuda.synchronize()
    X = runs[True]["X_pred"]
    assert np.array_equal(X, runs[False]["X_pred"]) and np.array_equal(X, fl["X_pred"].cpu().numpy())
    assert np.array_equal(runs[True]["n_steps"], runs[False]["n_steps"]) and np.array_equal(runs[True]["n_steps"], fl["n_steps"].cpu().numpy())
    assert np.array_equal(runs[True]["n_crowded"], runs[False]["n_crowded"]) and np.array_equal(runs[True]["n_crowded"], n_crowded)
    print("crowded fleet: n_crowded", n_crowded.reshape(20, 4).sum(1), "steps", runs[True]["n_steps"].reshape(20, 4).min(1),
          "smallest pair distance", NO.min_pair_distance(X))
    assert n_crowded.any()
