"""GPU: the tiled field calls (include/lipmpc.h, TILED FIELDS) against the Dijkstra oracles, bit for bit, on the inputs of
tests/field_tiled_cases.py (tests/test_field_tiled_oracle.py shows on the CPU what each case reaches); the round guarantee, the
budget and the resume on the spiral; 2048^2 and 4096^2 maps against closed forms; repeats, leftover state and graph replay.

Every comparison with an oracle is tests/grid_checks.py's: every output, bit for bit, the sentinel in the rows behind n_sub."""
import ctypes as C

import numpy as np
import pytest

import field_oracle as Fo
import field_tiled_cases as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402
from grid_checks import SENTINEL, bits, field_buffers, frontier_buffers, host, same_field, same_frontier  # noqa: E402

TW, TH = T.TW, T.TH
FIELD_CASES = [i for i in T.IDS if i != "no_frontier"]
FRONTIER_CASES = [i for i in T.IDS if i != "bad_goals"]
POISON = -0x01010102                                          # int32 of the bytes FE FE FE FE: not a status, a count or a flag


def _dims(c, kind):
    """(B, F, W, H): F fields -- one per goal, or one per evidence map."""
    F = len(c["goal"]) if kind == "field" else 1 if c["ev"].ndim == 2 else len(c["ev"])
    return (len(c["start"]), F) + c["occ"].shape[-2:]


def _planner(c, kind, **kw):
    if kind == "field":
        return lipmpc.GridFieldPlanner(r_inflate=c["r"], max_seg=c["max_seg"], **kw)
    return lipmpc.FrontierPlanner(r_inflate=c["r"], min_unknown=c["mu"], t_free=T.T_FREE, t_occ=T.T_OCC, max_seg=c["max_seg"], **kw)


def _buffers(c, kind):
    B, F, W, H = _dims(c, kind)
    out = (field_buffers if kind == "field" else frontier_buffers)(B, F, W, H, c["S_max"])
    out["settled"] = torch.full((F,), POISON, dtype=torch.int32, device="cuda")
    return out


def _inputs(c, kind):
    start = torch.as_tensor(c["start"], device="cuda")
    if kind == "field":
        return dict(goal=torch.as_tensor(c["goal"], device="cuda"), grid=lipmpc.GridMap(c["occ"], T.ORIGIN, T.CELL).to("cuda"), start=start)
    return dict(ev=torch.as_tensor(np.ascontiguousarray(c["ev"]), device="cuda"), start=start)


def _plan(pl, kind, inp, out, S_max):
    if kind == "field":
        return pl.plan_grid_batch(inp["goal"], inp["grid"], inp["start"], S_max=S_max, out=out)
    return pl.plan(inp["ev"], inp["start"], origin=T.ORIGIN, cell=T.CELL, S_max=S_max, out=out)


def _run(c, kind, **kw):
    out, pl = _buffers(c, kind), _planner(c, kind, tiled=True, **kw)
    got = _plan(pl, kind, _inputs(c, kind), out, c["S_max"])
    torch.cuda.synchronize()
    assert got is out and pl.last is out
    return host(out)


def _same(kind, got, want, S_max):
    (same_field if kind == "field" else same_frontier)(got, want, S_max)


def _same_bits(a, b):
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("kind,id_", [("field", i) for i in FIELD_CASES] + [("frontier", i) for i in FRONTIER_CASES])
def test_tiled_equals_the_oracle(kind, id_):
    """Both kinds of field and both path calls with rounds=None: settled, and every output the oracle's."""
    c = T.case(id_)
    got = _run(c, kind)
    assert got["settled"].tolist() == [1] * _dims(c, kind)[1]
    _same(kind, got, T.oracle(id_, kind), c["S_max"])


def test_the_one_workgroup_calls_still_refuse_363_x_362():
    c = T.case("363x362")
    for kind in ("field", "frontier"):
        with pytest.raises(RuntimeError) as e:
            _plan(_planner(c, kind), kind, _inputs(c, kind), None, c["S_max"])
        assert e.value.code == -2


# -- scale: closed forms, no Python Dijkstra --------------------------------------------------------------------------------
def test_open_2048_squared_settles_within_the_guaranteed_rounds():
    """An empty 2048 x 2048 grid, the goal in cell (0, 0).  A least-cost path is monotone in i and in j, so it changes tile at most
    (tiles along W - 1) + (tiles along H - 1) times: by the round guarantee every value is final after one round fewer than
    tiles along W + tiles along H, and the last round, in which nothing falls, leaves no tile active."""
    W = H = 2048
    rounds = -(-W // TW) - (-H // TH)
    pl = lipmpc.GridFieldPlanner(tiled=True, rounds=rounds)
    grid = lipmpc.GridMap(torch.zeros((W, H), dtype=torch.uint8, device="cuda"), (0.0, 0.0), (0.05, 0.05))
    got = pl.field(torch.tensor([[0.01, 0.02]], dtype=torch.float64, device="cuda"), grid)
    i, j = torch.arange(W, device="cuda")[:, None], torch.arange(H, device="cuda")[None, :]
    want = (7 * torch.minimum(i, j) + 5 * (i - j).abs()).to(torch.int32)
    assert got["settled"].tolist() == [1] and got["status"].tolist() == [0]
    assert torch.equal(got["field"][0].view(torch.int32), want)


def test_frontier_4096_squared():
    """An all-free 4096 x 4096 evidence grid whose rows i >= 4000 are unknown, min_unknown = 3, r_inflate = 0.  A cell of row 3999
    has the three unknown neighbours (4000, j - 1 .. j + 1) -- but on the two edge columns only two of them are inside the grid,
    and nothing outside counts: (3999, 0) and (3999, 4095) are no frontier cells.  So n_frontier = 4094, the field is
    5 (3999 - i) on columns 1 .. 4094, and on the two edge columns 5 in row 3999 (one axial step to the frontier) and
    5 (3999 - i) + 2 above it (one diagonal step inward, then straight down)."""
    W = H = 4096
    ev = torch.full((W, H), -T.T_FREE, dtype=torch.int32, device="cuda")
    ev[4000:] = 0
    pl = lipmpc.FrontierPlanner(r_inflate=0, min_unknown=3, t_free=T.T_FREE, t_occ=T.T_OCC, tiled=True)
    got = pl.field(ev)
    assert got["settled"].tolist() == [1] and got["n_frontier"].tolist() == [H - 2]
    i = torch.arange(W, device="cuda")[:, None].expand(W, H)
    want = (5 * (3999 - i)).to(torch.int32).clone()
    for col in (0, H - 1):
        want[:3999, col] += 2
        want[3999, col] = 5
    want[4000:] = -1                                           # INF
    assert torch.equal(got["field"][0].view(torch.int32), want)
    fr = torch.zeros((W, H), dtype=torch.uint8, device="cuda")
    fr[3999, 1:H - 1] = 1
    assert torch.equal(got["frontier"][0], fr)


# -- the budget, the guarantee and the resume, through the C calls ---------------------------------------------------------
def _field_call(kind, c, inp, out, work, rounds, resume):
    B, F, W, H = _dims(c, kind)
    tail = dict(work=work, work_bytes=work.numel(), max_rounds=rounds, resume=resume, settled=out["settled"],
                hip_stream=torch.cuda.current_stream().cuda_stream)
    if kind == "field":
        lipmpc._lib.call("lipmpc_grid_field_tiled_batch", device=0, F=F, **inp["grid"]._args(F, torch.device("cuda", 0)), goal=inp["goal"],
                         r_inflate=c["r"], field=out["field"], field_status=out["field_status"], **tail)
    else:
        lipmpc._lib.call("lipmpc_grid_frontier_field_tiled_batch", device=0, F=F, W=W, H=H, evidence=inp["ev"], t_free=T.T_FREE,
                         t_occ=T.T_OCC, r_inflate=c["r"], min_unknown=c["mu"], frontier=out["frontier"], field=out["field"],
                         n_frontier=out["n_frontier"], **tail)
    torch.cuda.synchronize()
    return host({k: out[k] for k in ("field", "settled")})


def _work(c, kind):
    B, F, W, H = _dims(c, kind)
    need = lipmpc._lib.load().lipmpc_grid_tiled_workspace_bytes(F, W, H)
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("kind", ["field", "frontier"])
def test_budget_guarantee_and_resume_on_the_spiral(kind):
    c, want = T.case("spiral"), T.oracle("spiral", kind)
    fld = want["field"][0]
    changes = T.tile_changes(want["cells"][0])                 # of the whole corridor: no cell's path changes tile more often
    # rounds=1 through the planner: unsettled, and the path call says so and writes nothing else
    got = _run(c, kind, rounds=1)
    assert got["settled"].tolist() == [0]
    assert got["status"].tolist() == [lipmpc.RRT_FIELD_UNSETTLED] * 2 and got["n_sub"].tolist() == [0, 0]
    assert np.isnan(got["path_cost"]).all() and (got["sub_goals"] == SENTINEL).all()
    if kind == "frontier":
        assert got["target_cell"].tolist() == [-1, -1] and np.isnan(got["target"]).all()

    def holds(got, rounds):
        finite = got["field"][0] != Fo.INF
        assert (got["field"][0][finite] >= fld[finite]).all() and (fld[finite] != Fo.INF).all()      # costs of real paths
        covered = T.guaranteed(fld, rounds)
        assert np.array_equal(got["field"][0][covered], fld[covered]), (rounds, int((got["field"][0][covered] != fld[covered]).sum()))
        return int(covered.sum())

    n1 = holds(got, 1)
    assert 0 < n1 < (fld != Fo.INF).sum()
    # the same through the C call, then resume round by round: a for loop bounded by the oracle's tile changes + 1
    inp, out, work = _inputs(c, kind), _buffers(c, kind), _work(c, kind)
    got = _field_call(kind, c, inp, out, work, 1, 0)
    assert got["settled"].tolist() == [0] and holds(got, 1) == n1
    settled_at = None
    for r in range(2, changes + 3):                            # total rounds 2 .. changes + 2
        got = _field_call(kind, c, inp, out, work, 1, 1)
        holds(got, r)
        if got["settled"].tolist() == [1]:
            settled_at = r
            break
    print(f"spiral {kind}: {changes} tile changes, settled after {settled_at} rounds")
    assert settled_at is not None and np.array_equal(got["field"], want["field"])
    # one more resume leaves every bit as it was
    again = _field_call(kind, c, inp, out, work, 3, 1)
    assert again["settled"].tolist() == [1] and np.array_equal(again["field"], want["field"])


@pytest.mark.parametrize("kind", ["field", "frontier"])
def test_three_maps_in_one_call_each_at_its_own_pace(kind):
    """F = 3 maps that need different numbers of rounds, one call with the budget that the guarantee gives the OPEN map (monotone
    paths: at most tiles along W - 1 + tiles along H - 1 tile changes, + 2): that map is settled; every settled field and its
    path are the oracle's, a robot on a field that is not settled is UNSETTLED."""
    c, want = T.case("three_maps"), T.oracle("three_maps", kind)
    B, F, W, H = _dims(c, kind)
    rounds = -(-W // TW) - (-H // TH)
    got = _run(c, kind, rounds=rounds)
    assert got["settled"][0] == 1
    for f in range(3):
        if got["settled"][f]:
            assert np.array_equal(got["field"][f], want["field"][f]) and got["status"][f] == want["status"][f]
        else:
            assert got["status"][f] == lipmpc.RRT_FIELD_UNSETTLED and got["n_sub"][f] == 0
    print("three_maps", kind, "tile changes", [T.tile_changes(p) for p in want["cells"]], f"settled after {rounds} rounds",
          got["settled"].tolist())


# -- repeats, leftover state, graphs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["field", "frontier"])
def test_two_cold_calls_and_leftover_state_give_the_same_bits(kind):
    c, want = T.case("baffles"), T.oracle("baffles", kind)
    first = _run(c, kind)
    _same_bits(first, _run(c, kind))
    _same(kind, first, want, c["S_max"])
    # work, field and settled full of 0xFF before a cold call
    inp, out, work = _inputs(c, kind), _buffers(c, kind), _work(c, kind)
    work.fill_(0xFF)
    out["field"].view(torch.int32).fill_(-1)
    out["settled"].fill_(-1)
    got = _field_call(kind, c, inp, out, work, T.rounds_to_settle(want["field"][0]), 0)
    assert got["settled"].tolist() == [1] and np.array_equal(got["field"], want["field"])


@pytest.mark.parametrize("kind", ["field", "frontier"])
def test_graph_replay_with_fixed_rounds(kind):
    """Field + path with a fixed budget captured in one graph and replayed twice into poisoned buffers: the oracle's bits."""
    c, want = T.case("baffles"), T.oracle("baffles", kind)
    B, F, W, H = _dims(c, kind)
    rounds = T.rounds_to_settle(want["field"][0])              # from the round guarantee, not measured
    pl, inp, out = _planner(c, kind, tiled=True, rounds=rounds), _inputs(c, kind), _buffers(c, kind)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _plan(pl, kind, inp, out, c["S_max"])                 # warm-up outside the capture: the workspace grows here
    torch.cuda.current_stream().wait_stream(side)
    works = len(pl._works)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _plan(pl, kind, inp, out, c["S_max"])
    assert len(pl._works) == works                             # nothing reallocated while capturing
    for _ in range(2):
        for k, v in out.items():
            if k == "sub_goals":
                v.fill_(SENTINEL)
            elif k == "field":
                v.view(torch.int32).fill_(12345)
            elif v.dtype == torch.float64:
                v.fill_(SENTINEL)
            else:
                v.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        got = host(out)
        assert got["settled"].tolist() == [1]
        _same(kind, got, want, c["S_max"])


def test_rounds_none_raises_under_capture_and_subclasses_refuse_tiled():
    c = T.case("one_tile")
    for kind in ("field", "frontier"):
        pl, inp, out = _planner(c, kind, tiled=True), _inputs(c, kind), _buffers(c, kind)
        _plan(pl, kind, inp, out, c["S_max"])                 # (eager: fine)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="rounds"):
            with torch.cuda.graph(graph):
                out["settled"].fill_(POISON)                   # (something to capture: the planner raises before it enqueues)
                _plan(pl, kind, inp, out, c["S_max"])
    with pytest.raises(ValueError, match="tiled"):
        lipmpc.CoordinatedFrontierPlanner(r_claim=4, tiled=True)
    with pytest.raises(ValueError, match="tiled"):
        lipmpc.InformedFrontierPlanner(r_view=8, w_gain=16, g_cap=64, tiled=True)
    with pytest.raises(ValueError, match="rounds"):
        lipmpc.GridFieldPlanner(rounds=4)                      # rounds without tiled
    with pytest.raises(ValueError, match="rounds"):
        lipmpc.FrontierPlanner(tiled=True, rounds=0)
