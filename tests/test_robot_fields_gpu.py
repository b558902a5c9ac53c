"""GPU: the claims from per-robot fields (lipmpc_grid_frontier_assign_robot_fields_batch, through RobotFieldsFrontierPlanner) against
tests/robot_fields_oracle.py: claim_round, n_claims, kept, n_kept, the int32 n_sub / status / target_cell and the doubles of
path_cost, target and the WHOLE sub-goal buffer, bit for bit, on the cases of tests/robot_fields_checks.py -- the smallest shapes at
which the kernels can go wrong.  Every buffer starts poisoned; tests/test_robot_fields_oracle.py holds each case to its name."""
import numpy as np
import pytest

import assign_checks as AC
import frontier_oracle as FR
import robot_fields_checks as RC
from assign_checks import CELL, ORIGIN, SENTINEL, bits, centres, open_field

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_every_output_equals_the_oracle(name):
    c = RC.case(name)
    RC.same(RC.run(c), RC.expected(name), c)


def test_s_max_at_n_sub_and_one_below():
    """S_max == n_sub: the rows fit exactly; one below: PATH_OVERFLOW, nothing written, the robot still claims."""
    c, full = RC.case("every-cell-marked"), RC.expected("every-cell-marked")
    b = full["winners"][0]
    n = int(full["n_sub"][b])
    for S_max in (n, n - 1):
        cs = dict(c, S_max=S_max)
        want = RC.expected_of(cs)
        got = RC.run(cs)
        RC.same(got, want, cs)
        assert got["claim_round"][b] == 0 and got["status"][b] == (FR.FOUND if S_max == n else FR.PATH_OVERFLOW)
        if S_max < n:
            assert got["n_sub"][b] == 0 and (got["sub_goals"][b] == SENTINEL).all()


def test_no_previous_targets_equals_the_null_call_and_two_calls_give_identical_bits():
    null, none = RC.run(RC.case("open6-r5")), RC.run(RC.case("keep-none"))
    assert RC.case("keep-none")["r_claim"] == RC.case("open6-r5")["r_claim"] and not none["kept"].any() and none["n_kept"].tolist() == [0]
    for k in null:
        assert np.array_equal(bits(none[k]), bits(null[k])), k
    for name in ("open6-r5", "keep-tile-corner", "B65"):
        a, b = RC.run(RC.case(name)), RC.run(RC.case(name))
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), (name, k)


def _claim_calls(c, budgets):
    """The nearest-frontier plan of a case (settled), then one claim call per (budget, resume) on the same buffers: the host copy of
    the outputs after each."""
    pl = RC.planner(c)
    out = RC.buffers(len(c["start"]), *c["ev"].shape, c["S_max"], c["keep"] is not None)
    ev, start, may, prev = RC.device(c)
    lipmpc.FrontierPlanner.plan(pl, ev, start, ORIGIN, CELL, c["S_max"], out)
    org, cs, org_c, cell_c = pl._placement(ORIGIN, CELL)
    W, H = c["ev"].shape
    for budget, resume in budgets:
        pl._claim_call(len(c["start"]), W, H, start, may, prev, org_c, cell_c, c["S_max"], out, budget, resume)
        pl._target(out, org, cs, H)
        torch.cuda.synchronize()
        yield AC.host(out)


def test_one_round_claims_nothing_and_resumed_calls_reach_the_cold_calls_bits():
    """rounds = 1 on the 2 x 2-tile map: a robot's field cannot cross a tile border in one round, so claims_settled is 0 and every
    row is exactly the path call's; one more round per resumed call until it settles; then every output equals one cold call's with
    a large budget, which equals the oracle's."""
    name = "keep-tile-corner"
    c, want = RC.case(name), RC.expected(name)
    cold, = _claim_calls(c, [(64, 0)])
    RC.same(cold, want, c)
    seen = []
    for got in _claim_calls(c, [(1, 0)] + [(1, 1)] * 7):
        seen.append(int(got["claims_settled"][0]))
        if seen[-1]:
            for k in cold:
                assert np.array_equal(bits(got[k]), bits(cold[k])), k
        else:
            RC.unclaimed(got, want["nearest"], c["S_max"])
    print("claims_settled after each one-round call:", seen)
    assert seen[0] == 0 and seen[-1] == 1 and seen == sorted(seen)
    # one call of the fixed budget 1 through the planner: no synchronisation, nobody claims (its frontier field is unsettled too)
    got = RC.run(c, rounds=1)
    assert got["claims_settled"].tolist() == [0] and got["n_claims"].tolist() == [0] and (got["claim_round"] == -1).all()


def test_serpentine_needs_more_rounds_than_an_open_map_through_rounds_none():
    ev = RC.serpentine()
    W, H = ev.shape
    c = RC._case(ev, centres([(1, 5), (33, 60), (65, 100)]), 3, r=0)
    want = RC.expected_of(c)
    assert want["n_claims"] >= 2 and max(want["costs"]) > 5 * 8 * H // 2
    open_map = -(-W // RC.TW) - (-H // RC.TH) + 1
    short = RC.run(c, rounds=open_map)
    assert short["claims_settled"].tolist() == [0] and short["n_claims"].tolist() == [0]
    RC.same(RC.run(c), want, c)


def test_graph_replay_with_fixed_rounds_after_the_evidence_changed():
    c = RC.case("keep-all")
    pl = RC.planner(c, rounds=6)                              # 2 x 1 tiles of an open rectangle: a path changes tile at most once
    out = RC.buffers(len(c["start"]), *c["ev"].shape, c["S_max"], True)
    ev, start, may, prev = RC.device(c)
    plan = lambda: pl.replan(ev, start, origin=ORIGIN, cell=CELL, S_max=c["S_max"], out=out, prev_target=prev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan()                                                 # warm-up outside the capture: the workspaces grow here
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan()
    works = len(pl._claim_works)
    changed = dict(c, ev=np.ascontiguousarray(open_field(40, 44, margin=4)))
    for cs, want in ((c, RC.expected("keep-all")), (changed, RC.expected_of(changed))):
        ev.copy_(torch.as_tensor(cs["ev"], device="cuda"))
        RC.poison(out)
        graph.replay()
        torch.cuda.synchronize()
        RC.same(AC.host(out), want, cs)
    assert len(pl._claim_works) == works and want["n_kept"] < 6      # (the ring receded by two cells: r_keep 0 finds no anchor)


def test_the_launch_count_is_max_rounds_plus_8_and_the_fleet_cap_is_refused_in_python():
    import ctypes as C
    c = RC.case("open6-r5")
    hip = C.CDLL("libamdhip64.so")
    for rounds, resume, extra in ((1, 0, 8), (5, 0, 8), (3, 1, 5)):
        pl = RC.planner(c)
        out = RC.buffers(len(c["start"]), *c["ev"].shape, c["S_max"], False)
        ev, start, may, prev = RC.device(c)
        lipmpc.FrontierPlanner.plan(pl, ev, start, ORIGIN, CELL, c["S_max"], out)
        org, cs, org_c, cell_c = pl._placement(ORIGIN, CELL)
        call = lambda r: pl._claim_call(len(c["start"]), 40, 44, start, may, prev, org_c, cell_c, c["S_max"], out, rounds, r)
        call(0)                                                # outside the capture: the workspace grows here
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        handle, graph, n = C.c_void_p(stream.cuda_stream), C.c_void_p(), C.c_size_t()
        assert hip.hipStreamBeginCapture(handle, 2) == 0       # hipStreamCaptureModeRelaxed
        try:
            with torch.cuda.stream(stream):
                call(resume)
        finally:
            assert hip.hipStreamEndCapture(handle, C.byref(graph)) == 0
        assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and hip.hipGraphDestroy(graph) == 0
        assert n.value == rounds + extra, (rounds, resume, n.value)
    big = RC.planner(c)
    with pytest.raises(ValueError, match="2\\^31"):
        big.plan(torch.zeros((2048, 4096), dtype=torch.int32, device="cuda"), torch.zeros((300, 2), dtype=torch.float64, device="cuda"),
                 origin=ORIGIN, cell=CELL)
