"""GPU: claim hysteresis for the gain-seeded claims by tiles (lipmpc_grid_frontier_assign_keep_utility_tiled_batch, through
TiledGainKeepFrontierPlanner.replan) against tests/assign_keep_utility_oracle.py and against the one-workgroup call, EVERY output bit
for bit, on a map of 2 x 2 tiles and on the first shape the one-workgroup calls refuse.  Every buffer starts poisoned."""
import ctypes as C_
import functools

import numpy as np
import pytest

import assign_keep_utility_checks as C
import assign_utility_checks as U
from assign_keep_utility_checks import GENEROUS, index
from gain_checks import CELL, ORIGIN, SENTINEL, T_FREE, T_OCC, bits, centres

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

TW, TH, _ = lipmpc.planner.tiled_info()
R_CLAIM, GAIN = 9, (4, 16, 60, 0)                             # (r_view, w_gain, g_cap, min_gain)
SHAPES = ((TW + 1, TH + 8), (363, 362))                       # 2 x 2 tiles, one row and eight columns over the tile edges; > 2^17 cells
TABLE = lipmpc.planner.tiled_assign_keep_utility_outputs
CALL = "lipmpc_grid_frontier_assign_keep_utility_tiled_batch"


def tile_of(c):
    return c[0] // TW, c[1] // TH


@functools.lru_cache(maxsize=None)
def scene(W, H, keep=GENEROUS):
    """tests/test_assign_utility_tiled_gpu.py's scene -- a free room with a wall stub in the far corner of an unknown map, a
    hand-written gain, four robots side by side -- with previous targets: robot 0 had the room's far corner cell (in another tile than
    the robots), robot 2 a cell of the near rim, robots 1 and 3 none.  (ev, gain, start, prev, the oracle's plan)."""
    assert (TW, TH) == (32, 64)
    ev = np.zeros((W, H), np.int32)
    i0, j0 = max(2, W - 100), max(2, H - 150)
    ev[i0:W - 2, j0:H - 2] = -T_FREE
    ev[(i0 + W) // 2, j0 + 6:H - 12] = T_OCC
    gain = np.fromfunction(lambda i, j: 5 + (3 * i + 7 * j) % 61, (W, H)).astype(np.int32)
    start = centres([((i0 + W) // 2 - 5, (j0 + H) // 2 + k) for k in range(4)])
    prev = np.array([index((W - 3, H - 3), H), -1, index((i0, (j0 + H) // 2), H), -1], np.int32)
    want = C.expected(ev, start, R_CLAIM, GAIN, prev, keep, gain=gain)
    assert tile_of((i0, j0)) != tile_of((W - 3, H - 3))         # the room lies in several tiles
    return ev, gain, start, prev, want


def _buffers(B, W, H, S_max=64):
    table = dict(TABLE(B, W, H, S_max), settled=(torch.int32, (1,), True), usettled=(torch.int32, (1,), True))
    return C.buffers(B, W, H, S_max, table)


def _planner(gain, keep=GENEROUS, max_claims=64, rounds=None):
    return C.planner(R_CLAIM, GAIN, keep, max_claims, gain=gain, cls=lipmpc.TiledGainKeepFrontierPlanner, rounds=rounds)


def _run(ev, gain, start, prev, keep=GENEROUS, max_claims=64, rounds=None, pl=None, out=None):
    W, H = ev.shape
    out = _buffers(len(start), W, H) if out is None else out
    pl = pl or _planner(gain, keep, max_claims, rounds)
    got = pl.replan(torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda"), origin=ORIGIN, cell=CELL, S_max=64, out=out,
                    prev_target=None if prev is None else torch.as_tensor(prev, device="cuda"))
    torch.cuda.synchronize()
    assert got is out and pl.last is out and "work" not in out
    return C.host(out)


@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("keep", [GENEROUS, (6, 24, 8)])
def test_settled_equals_the_oracle_and_the_one_workgroup_call(W, H, keep):
    ev, gain, start, prev, want = scene(W, H, keep)
    assert want["n_claims"] == 4 and len(want["attempts"]) == 2 and (want["n_kept"] == 2 if keep == GENEROUS else True)
    got = _run(ev, gain, start, prev, keep)
    assert got["settled"].tolist() == got["usettled"].tolist() == got["claims_settled"].tolist() == [1]
    C.same(got, want, 64)
    C.hence(want, R_CLAIM, 64)
    assert set(got) == set(TABLE(4, W, H, 64)) | {"settled", "usettled"}
    one = C.planner(R_CLAIM, GAIN, keep, gain=gain)
    d_ev, d_start, d_prev = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda"), torch.as_tensor(prev, device="cuda")
    if W * H > 1 << 17:                                        # the one-workgroup planner refuses the shape: LIPMPC_E_UNSUPPORTED
        with pytest.raises(RuntimeError) as e:
            one.replan(d_ev, d_start, origin=ORIGIN, cell=CELL, prev_target=d_prev)
        assert e.value.code == -2
        return
    plain = C.host(one.replan(d_ev, d_start, origin=ORIGIN, cell=CELL, out=C.buffers(len(start), W, H, 64), prev_target=d_prev))
    for k in plain:
        assert np.array_equal(bits(plain[k]), bits(got[k])), k


def test_no_previous_target_is_the_tiled_gain_seeded_claim():
    W, H = SHAPES[0]
    ev, gain, start, _, _ = scene(W, H)
    got = _run(ev, gain, start, None, (5, 16, 0))
    pl = U.planner(R_CLAIM, *GAIN, gain=gain, cls=lipmpc.TiledCoordinatedFrontierPlanner)
    table = dict(lipmpc.planner.tiled_assign_utility_outputs(4, W, H, 64), settled=(torch.int32, (1,), True), usettled=(torch.int32, (1,), True))
    seeded = pl.plan(torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda"), origin=ORIGIN, cell=CELL,
                     out=U.buffers(4, W, H, 64, table))          # (poisoned as the new call's: the rows past n_sub hold the sentinel in both)
    torch.cuda.synchronize()
    seeded = U.host(seeded)
    assert int(seeded["n_claims"][0]) == 4 and not got["kept"].any() and got["n_kept"].tolist() == [0]
    for k in seeded:
        assert np.array_equal(bits(got[k]), bits(seeded[k])), k


def _settled_plan(W, H):
    """The plan that precedes the claims, settled, into fresh poisoned buffers with no claim allowed: (planner, out, what a claim
    call takes)."""
    ev, gain, start, prev, want = scene(W, H)
    pl = _planner(gain, max_claims=0)
    out = _buffers(4, W, H)
    got = _run(ev, gain, start, prev, pl=pl, out=out)
    assert got["settled"].tolist() == got["usettled"].tolist() == [1] and got["n_claims"].tolist() == got["n_kept"].tolist() == [0]
    org, cs, org_c, cell_c = pl._placement(ORIGIN, CELL)
    pl.max_claims = 64

    def claims(budget):
        pl.rounds = budget
        pl._gain_keep_claims(4, W, H, torch.as_tensor(start, device="cuda"), None, torch.as_tensor(prev, device="cuda"), org_c, cell_c, 64, out)
        pl._target(out, org, cs, H)
        torch.cuda.synchronize()
        return C.host(out)
    return pl, out, claims


@pytest.mark.parametrize("W,H", SHAPES)
def test_a_budget_too_short_gives_the_rules_first_winners_and_a_larger_one_completes_them(W, H):
    """Robot 0 keeps the far corner of the room: the field of that one cell crosses the tile borders.  Every budget runs on the
    same buffers; with claims_settled == 0 the winners so far are exactly the rule's first n_claims (GENEROUS: every attempt
    succeeds, so n_claims slots were spent), and the first budget that settles every slot gives the oracle's answer, as does any
    larger one.  One round short of that budget is not enough."""
    ev, gain, start, prev, want = scene(W, H)
    pl, out, claims = _settled_plan(W, H)
    seen, budget = [], 1
    first = functools.lru_cache(maxsize=None)(                 # the rule's first n winners (the oracle once per n)
        lambda n: C.expected(ev, start, R_CLAIM, GAIN, prev, GENEROUS, max_claims=n, gain=gain, informed=want["informed"]))
    while True:
        got = claims(budget)
        n, ok = int(got["n_claims"][0]), int(got["claims_settled"][0])
        seen.append((budget, n, ok))
        C.same(got, want if ok else first(n), 64)
        assert ok or n < want["n_claims"]
        if ok or budget >= 64:
            break
        budget += 1
    print("budget, n_claims, claims_settled:", seen)
    assert len(seen) > 1 and seen[-1][1:] == (want["n_claims"], 1) and seen[-2][2] == 0, seen         # one round short: claims_settled 0
    assert [n for _, n, _ in seen] == sorted(n for _, n, _ in seen)
    got = claims(budget + 3)                                   # a repeat with a larger budget: the same answer
    assert got["claims_settled"].tolist() == [1]
    C.same(got, want, 64)
    # rounds=None doubles the budget by itself
    C.same(_run(ev, gain, start, prev), want, 64)


def test_an_unsettled_utility_field_or_frontier_field_stops_the_call_from_the_start():
    W, H = SHAPES[0]
    pl, out, claims = _settled_plan(W, H)
    before = C.host(out)
    for key in ("usettled", "settled"):
        out[key].zero_()
        for k in ("claim_round", "n_claims", "n_kept", "claims_settled"):
            out[k].fill_(C.POISON_I32)
        out["kept"].fill_(C.POISON_I8)
        got = claims(16)
        assert got["n_claims"].tolist() == got["n_kept"].tolist() == got["claims_settled"].tolist() == [0], key
        assert (got["claim_round"] == -1).all() and not got["kept"].any()
        for k in ("sub_goals", "n_sub", "status", "path_cost", "target_cell", "target_gain"):
            assert np.array_equal(bits(got[k]), bits(before[k])), (key, k)
        out[key].fill_(1)
    assert claims(16)["claims_settled"].tolist() == [1]         # both settled again: the call runs


def _kernel_nodes(enqueue):
    """The nodes of the graph a stream capture of ``enqueue(stream)`` gives: every launch of the call is one kernel node."""
    hip = C_.CDLL("libamdhip64.so")
    stream = torch.cuda.Stream()
    handle, graph, n = C_.c_void_p(stream.cuda_stream), C_.c_void_p(), C_.c_size_t()
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(handle, 2) == 0           # hipStreamCaptureModeRelaxed
    try:
        enqueue(stream.cuda_stream)
    finally:
        assert hip.hipStreamEndCapture(handle, C_.byref(graph)) == 0
    assert hip.hipGraphGetNodes(graph, None, C_.byref(n)) == 0
    assert hip.hipGraphDestroy(graph) == 0
    return n.value


def test_kernel_nodes_of_a_captured_call_equal_the_header_formula_and_a_replay_gives_the_oracles_bits():
    """max_claims * (max_rounds + 5) + 3 launches, whatever the fleet needs -- the tiled keep call's count."""
    W, H = SHAPES[0]
    ev, gain, start, prev, want = scene(W, H)
    rounds, max_claims = 6, 5
    pl = _planner(gain, GENEROUS, max_claims, rounds)
    out = _buffers(4, W, H)
    _run(ev, gain, start, prev, pl=pl, out=out)                # outside the capture: the workspaces grow here
    org, cs, org_c, cell_c = pl._placement(ORIGIN, CELL)
    d_ev, d_start, d_prev = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda"), torch.as_tensor(prev, device="cuda")
    work = pl._claim_works[-1]
    common = dict(device=pl.device_index, B=4, W=W, H=H, origin=C_.addressof(org_c), cell=C_.addressof(cell_c), frontier=out["frontier"],
                  field=out["field"], settled=out["settled"], start=d_start, may_claim=None, prev_target=d_prev, r_inflate=2, r_claim=R_CLAIM,
                  r_keep=0, keep_ratio16=1024, keep_slack=4096, max_seg=pl.max_seg, S_max=64, work=work, work_bytes=work.numel(),
                  claims_settled=out["claims_settled"], gain=out["gain"], ufield=out["ufield"], usettled=out["usettled"], w_gain=GAIN[1],
                  g_cap=GAIN[2], min_gain=GAIN[3], target_gain=out["target_gain"],
                  **{k: out[k] for k in ("sub_goals", "n_sub", "status", "path_cost", "target_cell", "claim_round", "n_claims", "kept", "n_kept")})
    for claims, budget in ((1, 1), (3, 4), (max_claims, rounds)):
        call = lambda s: lipmpc._lib.call(CALL, **common, max_claims=claims, max_rounds=budget, hip_stream=s)
        assert _kernel_nodes(call) == claims * (budget + 5) + 3
    whole = torch.cuda.CUDAGraph()
    with torch.cuda.graph(whole):
        pl.replan(d_ev, d_start, origin=ORIGIN, cell=CELL, S_max=64, out=out, prev_target=d_prev)
    for _ in range(2):
        C.poison(out)
        whole.replay()
        torch.cuda.synchronize()
        got = C.host(out)
        assert got["settled"].tolist() == got["usettled"].tolist() == got["claims_settled"].tolist() == [1]
        C.same(got, C.expected(ev, start, R_CLAIM, GAIN, prev, GENEROUS, max_claims=max_claims, gain=gain, informed=want["informed"]), 64)
