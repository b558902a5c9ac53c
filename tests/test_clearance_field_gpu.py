"""GPU: the weighted tiled fields and their path calls (include/lipmpc.h, SOFT CLEARANCE) against the weighted Dijkstra oracle of
tests/clearance_oracle.py, bit for bit -- field, statuses, settled, sub-goal doubles, n_sub, path_cost, target_cell -- on the inputs
of tests/clearance_cases.py (tests/test_clearance_oracle.py shows on the CPU what each case reaches); the zero layer against the
existing tiled calls; budget, resume and graph replay.

Every comparison with an oracle is tests/grid_checks.py's: every output, the sentinel in the rows behind n_sub."""
import numpy as np
import pytest

import clearance_cases as K
import clearance_oracle as CO
import field_tiled_cases as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402
from grid_checks import SENTINEL, bits, field_buffers, frontier_buffers, host, same_field, same_frontier  # noqa: E402

KINDS = ("field", "frontier")
POISON = -0x01010102


def _dims(c, kind):
    F = len(c["goal"]) if kind == "field" else 1 if c["ev"].ndim == 2 else len(c["ev"])
    return (len(c["start"]), F) + c["occ"].shape[-2:]


def _maps(c, kind):
    """How many maps (and so layers) the call sees."""
    return 1 if (c["occ"] if kind == "field" else c["ev"]).ndim == 2 else len(c["occ"])


def _planner(c, kind, **kw):
    if "clear" in c:
        kw.update(r_clear=c["clear"][0], w_clear=c["clear"][1])
    if kind == "field":
        return lipmpc.GridFieldPlanner(r_inflate=c["r"], max_seg=c["max_seg"], tiled=True, **kw)
    return lipmpc.FrontierPlanner(r_inflate=c["r"], min_unknown=c["mu"], t_free=K.T_FREE, t_occ=K.T_OCC, max_seg=c["max_seg"], tiled=True, **kw)


def _buffers(c, kind):
    B, F, W, H = _dims(c, kind)
    out = (field_buffers if kind == "field" else frontier_buffers)(B, F, W, H, c["S_max"])
    out["settled"] = torch.full((F,), POISON, dtype=torch.int32, device="cuda")
    return out


def _inputs(c, kind, cost=None):
    inp = dict(start=torch.as_tensor(c["start"], device="cuda"))
    if kind == "field":
        inp.update(goal=torch.as_tensor(c["goal"], device="cuda"), grid=lipmpc.GridMap(c["occ"], K.ORIGIN, K.CELL).to("cuda"))
    else:
        inp.update(ev=torch.as_tensor(np.ascontiguousarray(c["ev"]), device="cuda"))
    cost = c.get("cost") if cost is None else cost
    if cost is not None:
        inp["cost"] = torch.as_tensor(np.ascontiguousarray(cost), device="cuda")
    return inp


def _plan(pl, kind, inp, out, S_max):
    more = dict(cost=inp["cost"]) if "cost" in inp else {}
    if kind == "field":
        return pl.plan_grid_batch(inp["goal"], inp["grid"], inp["start"], S_max=S_max, out=out, **more)
    return pl.plan(inp["ev"], inp["start"], origin=K.ORIGIN, cell=K.CELL, S_max=S_max, out=out, **more)


def _run(c, kind, cost=None, **kw):
    out, pl = _buffers(c, kind), _planner(c, kind, **kw)
    got = _plan(pl, kind, _inputs(c, kind, cost), out, c["S_max"])
    torch.cuda.synchronize()
    assert got is out and pl.last is out
    return host(out)


def _same(kind, got, want, S_max):
    (same_field if kind == "field" else same_frontier)(got, want, S_max)


def _same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("id_", K.IDS)
def test_weighted_equals_the_oracle(id_, kind):
    """Both weighted fields and both weighted path calls with rounds=None: settled, every output the oracle's, and the layer the
    dict returns is the one the oracle was given (the clearance layer where the planner made it)."""
    c = K.case(id_)
    got = _run(c, kind)
    assert got["settled"].tolist() == [1] * _dims(c, kind)[1]
    want = K.oracle(id_, kind)
    print(id_, kind, "status", np.bincount(want["status"], minlength=9).tolist(), "most sub-goals", int(want["n_sub"].max()))
    _same(kind, got, want, c["S_max"])
    layer = K.layer(c)
    assert got["cost"].shape == (_maps(c, kind),) + c["occ"].shape[-2:] and np.array_equal(got["cost"].reshape(layer.shape), layer)


@pytest.mark.parametrize("id_,kind", [(i, k) for i in K.ZERO_IDS for k in KINDS if (i, k) != ("no_frontier", "field")])
def test_zero_layer_equals_the_tiled_calls(id_, kind):
    """An all-zero layer: every output bit of the weighted calls is the existing tiled calls' (and so the unweighted oracle's)."""
    c = T.case(id_)
    plain = _run(c, kind)
    assert "cost" not in plain
    zero = _run(c, kind, cost=np.zeros((_maps(c, kind),) + c["occ"].shape[-2:], np.uint8))
    assert not zero.pop("cost").any()
    _same_bits(zero, plain)
    _same(kind, zero, T.oracle(id_, kind), c["S_max"])


@pytest.mark.parametrize("kind", KINDS)
def test_w_clear_zero_equals_the_tiled_calls(kind):
    """r_clear with w_clear = 0: the clearance layer is all zero, the plan is the plain tiled one."""
    c = dict(K.case("clear_strip_r2"))
    del c["clear"]
    plain = _run(c, kind)
    zero = _run(c, kind, r_clear=4, w_clear=0)
    assert not zero.pop("cost").any()
    _same_bits(zero, plain)


def test_cost_keyword_needs_tiled_and_a_fitting_layer():
    c = K.case("two_door")
    inp = _inputs(c, "field")
    W, H = c["occ"].shape
    good = torch.zeros((W, H), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="tiled"):
        lipmpc.GridFieldPlanner().plan_grid_batch(inp["goal"], inp["grid"], inp["start"], cost=good)
    with pytest.raises(ValueError, match="tiled"):
        lipmpc.FrontierPlanner(t_free=1, t_occ=3).field(torch.as_tensor(c["ev"], device="cuda"), cost=good)
    pl = lipmpc.GridFieldPlanner(tiled=True)
    for bad in (good[:, :-1].contiguous(), good.to(torch.int32), good.cpu(), good.t()):
        with pytest.raises(ValueError, match="cost"):
            pl.plan_grid_batch(inp["goal"], inp["grid"], inp["start"], cost=bad)
    with pytest.raises(TypeError):
        lipmpc.TiledInformedFrontierPlanner(r_view=8, w_gain=16, g_cap=64, t_free=1, t_occ=3).plan(
            torch.as_tensor(c["ev"], device="cuda"), inp["start"], origin=K.ORIGIN, cell=K.CELL, cost=good)
    # cost= in place of the planner's own layer, [W,H] for one map; field() returns it too
    own = lipmpc.GridFieldPlanner(tiled=True, r_clear=4, w_clear=40)
    got = own.field(inp["goal"], inp["grid"], cost=good)
    assert got["cost"].shape == (1, W, H) and got["cost"].data_ptr() == good.data_ptr()
    torch.cuda.synchronize()
    assert np.array_equal(got["field"].view(torch.int32).cpu().numpy().view(np.uint32), K.plan(c, "field", np.zeros((W, H), np.uint8))["field"])


# -- the budget and the resume, through the C calls ---------------------------------------------------------------------------
def _field_call(kind, c, inp, cost, out, work, rounds, resume):
    B, F, W, H = _dims(c, kind)
    tail = dict(work=work, work_bytes=work.numel(), max_rounds=rounds, resume=resume, settled=out["settled"],
                hip_stream=torch.cuda.current_stream().cuda_stream)
    if kind == "field":
        lipmpc._lib.call("lipmpc_grid_field_weighted_batch", device=0, F=F, **inp["grid"]._args(F, torch.device("cuda", 0)), cost=cost,
                         goal=inp["goal"], r_inflate=c["r"], field=out["field"], field_status=out["field_status"], **tail)
    else:
        lipmpc._lib.call("lipmpc_grid_frontier_field_weighted_batch", device=0, F=F, W=W, H=H, evidence=inp["ev"], cost=cost, t_free=K.T_FREE,
                         t_occ=K.T_OCC, r_inflate=c["r"], min_unknown=c["mu"], frontier=out["frontier"], field=out["field"],
                         n_frontier=out["n_frontier"], **tail)
    torch.cuda.synchronize()
    return host({k: out[k] for k in ("field", "settled")})


def _work(c, kind):
    B, F, W, H = _dims(c, kind)
    need = lipmpc._lib.load().lipmpc_grid_tiled_workspace_bytes(F, W, H)
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("id_", ["two_tiles", "serpentine"])
def test_one_round_is_unsettled_and_resumes_settle(id_, kind):
    """rounds=1 on a two-tile map: settled 0, RRT_FIELD_UNSETTLED and nothing else written; every finite word is then the cost of a
    real path (>= the final value), final where the round guarantee says so; resumes, one round each and no more of them than the
    guarantee allows, end settled with the oracle's field."""
    c, want = K.case(id_), K.oracle(id_, kind)
    fld, layer = want["field"][0], K.layer(c)
    B = len(c["start"])
    got = _run(c, kind, rounds=1)
    assert got["settled"].tolist() == [0]
    assert got["status"].tolist() == [lipmpc.RRT_FIELD_UNSETTLED] * B and got["n_sub"].tolist() == [0] * B
    assert np.isnan(got["path_cost"]).all() and (got["sub_goals"] == SENTINEL).all()
    if kind == "frontier":
        assert got["target_cell"].tolist() == [-1] * B and np.isnan(got["target"]).all()
    changes = K.descent_changes(fld, CO.k_of(layer))

    def holds(got, rounds):
        finite = got["field"][0] != CO.INF
        assert (got["field"][0][finite] >= fld[finite]).all() and (fld[finite] != CO.INF).all()
        covered = (changes >= 0) & (changes <= rounds - 1)
        assert np.array_equal(got["field"][0][covered], fld[covered]), rounds

    holds(got, 1)
    inp, out, work = _inputs(c, kind), _buffers(c, kind), _work(c, kind)
    cost = torch.as_tensor(np.ascontiguousarray(layer), device="cuda")
    got = _field_call(kind, c, inp, cost, out, work, 1, 0)
    assert got["settled"].tolist() == [0]
    holds(got, 1)
    budget, settled_at = K.rounds_to_settle(fld, layer), None
    for r in range(2, budget + 1):
        got = _field_call(kind, c, inp, cost, out, work, 1, 1)
        holds(got, r)
        if got["settled"].tolist() == [1]:
            settled_at = r
            break
    print(f"{id_} {kind}: most tile changes {int(changes.max())}, settled after {settled_at} rounds (budget {budget})")
    assert settled_at is not None and np.array_equal(got["field"], want["field"])
    again = _field_call(kind, c, inp, cost, out, work, 3, 1)
    assert again["settled"].tolist() == [1] and np.array_equal(again["field"], want["field"])


@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_and_leftover_state_give_the_same_bits(kind):
    c, want = K.case("random"), K.oracle("random", kind)
    first = _run(c, kind)
    _same_bits(first, _run(c, kind))
    inp, out, work = _inputs(c, kind), _buffers(c, kind), _work(c, kind)
    work.fill_(0xFF)
    out["field"].view(torch.int32).fill_(-1)
    out["settled"].fill_(-1)
    got = _field_call(kind, c, inp, inp["cost"], out, work, K.rounds_to_settle(want["field"][0], c["cost"]), 0)
    assert got["settled"].tolist() == [1] and np.array_equal(got["field"], want["field"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("id_", ["clear_strip_r2", "random"])
def test_graph_replay_with_fixed_rounds(id_, kind):
    """Cost layer + weighted field + weighted path with a fixed budget captured in one graph and replayed twice into poisoned buffers
    (the planner's own layer included): the oracle's bits, nothing allocated while capturing."""
    c, want = K.case(id_), K.oracle(id_, kind)
    rounds = K.rounds_to_settle(want["field"][0], K.layer(c))            # from the round guarantee, not measured
    pl, inp, out = _planner(c, kind, rounds=rounds), _inputs(c, kind), _buffers(c, kind)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _plan(pl, kind, inp, out, c["S_max"])                 # warm-up outside the capture: workspace and layer grow here
    torch.cuda.current_stream().wait_stream(side)
    works, costs = len(pl._works), len(pl._costs)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _plan(pl, kind, inp, out, c["S_max"])
    assert len(pl._works) == works and len(pl._costs) == costs
    for _ in range(2):
        for k, v in out.items():
            if k == "sub_goals":
                v.fill_(SENTINEL)
            elif k == "field":
                v.view(torch.int32).fill_(12345)
            elif k == "cost":
                if "clear" in c:
                    v.fill_(0xA5)                              # (the planner's layer: the graph makes it again)
            elif v.dtype == torch.float64:
                v.fill_(SENTINEL)
            else:
                v.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        got = host(out)
        assert got["settled"].tolist() == [1]
        _same(kind, got, want, c["S_max"])
        assert np.array_equal(got["cost"].reshape(K.layer(c).shape), K.layer(c))


def test_the_layer_buffer_must_not_grow_under_capture():
    c = K.case("two_door")
    pl, inp, out = _planner(c, "field", rounds=4), _inputs(c, "field"), _buffers(c, "field")
    pl._works.append(torch.empty(1 << 20, dtype=torch.uint8, device="cuda"))      # (the workspace is there; the layer is not)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="clearance"):
        with torch.cuda.graph(graph):
            out["settled"].fill_(POISON)
            _plan(pl, "field", inp, out, c["S_max"])
