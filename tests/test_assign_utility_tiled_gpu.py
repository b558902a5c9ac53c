"""GPU: the tiled gain-seeded claims (lipmpc_grid_frontier_assign_utility_tiled_batch, through TiledCoordinatedFrontierPlanner
with the gain keywords) against tests/assign_utility_oracle.py and against the one-workgroup call, EVERY output bit for bit, on maps
of several tiles and on the first shape the one-workgroup calls refuse.  Every buffer starts poisoned."""
import functools

import numpy as np
import pytest

import assign_utility_checks as U
from gain_checks import CELL, ORIGIN, SENTINEL, T_FREE, T_OCC, bits, centres

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

TW, TH, _ = lipmpc.planner.tiled_info()
POISON = -0x01010102                                          # int32 of the bytes FE FE FE FE: not a status, a count or a flag
R_CLAIM, GAIN = 9, (4, 16, 60, 0)                             # (r_view, w_gain, g_cap, min_gain)
SHAPES = ((33, 72), (65, 130), (363, 362))


@functools.lru_cache(maxsize=None)
def scene(W, H):
    """A free room with a wall stub in the far corner of an unknown map -- on 363 x 362 over a dozen tiles, at the largest cell
    indices -- a hand-written gain that favours the far side, and four robots side by side: (ev, gain, start, the oracle's plan)."""
    assert (TW, TH) == (32, 64)
    ev = np.zeros((W, H), np.int32)
    i0, j0 = max(2, W - 100), max(2, H - 150)
    ev[i0:W - 2, j0:H - 2] = -T_FREE
    ev[(i0 + W) // 2, j0 + 6:H - 12] = T_OCC
    gain = np.fromfunction(lambda i, j: 5 + (3 * i + 7 * j) % 61, (W, H)).astype(np.int32)
    start = centres([((i0 + W) // 2 - 5, (j0 + H) // 2 + k) for k in range(4)])
    want = U.expected(ev, start, R_CLAIM, *GAIN, gain=gain)
    assert want["n_claims"] == 4 and tile_of((i0, j0)) != tile_of((W - 3, H - 3))           # the room lies in several tiles
    return ev, gain, start, want


def tile_of(c):
    return c[0] // TW, c[1] // TH


def _buffers(B, W, H, S_max=64):
    table = lipmpc.planner.tiled_assign_utility_outputs(B, W, H, S_max)
    out = {k: torch.empty(shape, dtype=dt, device="cuda") for k, (dt, shape, _) in table.items()}
    for k in ("settled", "usettled"):
        out[k] = torch.empty((1,), dtype=torch.int32, device="cuda")
    _poison(out)
    return out


def _poison(out):
    U.poison(out)
    for k in ("settled", "usettled", "claims_settled"):
        out[k].fill_(POISON)


def _planner(gain, max_claims=64, rounds=None):
    return U.planner(R_CLAIM, *GAIN, max_claims=max_claims, gain=gain, cls=lipmpc.TiledCoordinatedFrontierPlanner, rounds=rounds)


def _run(ev, gain, start, max_claims=64, rounds=None, pl=None, out=None):
    W, H = ev.shape
    out = _buffers(len(start), W, H) if out is None else out
    pl = pl or _planner(gain, max_claims, rounds)
    got = pl.plan(torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda"), origin=ORIGIN, cell=CELL, S_max=64, out=out)
    torch.cuda.synchronize()
    assert got is out and pl.last is out and "work" not in out
    return U.host(out)


@pytest.mark.parametrize("W,H", SHAPES)
def test_rounds_none_equals_the_oracle_and_the_one_workgroup_call(W, H):
    ev, gain, start, want = scene(W, H)
    got = _run(ev, gain, start)
    assert got["settled"].tolist() == got["usettled"].tolist() == got["claims_settled"].tolist() == [1]
    U.same(got, want, 64)
    U.hence(want, R_CLAIM, 64)
    one = U.planner(R_CLAIM, *GAIN, gain=gain)
    d_ev, d_start = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda")
    if W * H > 1 << 17:                                        # the one-workgroup planner refuses the shape: LIPMPC_E_UNSUPPORTED
        with pytest.raises(RuntimeError) as e:
            one.plan(d_ev, d_start, origin=ORIGIN, cell=CELL)
        assert e.value.code == -2
        return
    plain = U.host(one.plan(d_ev, d_start, origin=ORIGIN, cell=CELL, out=U.buffers(len(start), W, H, 64)))
    for k in plain:
        assert np.array_equal(bits(plain[k]), bits(got[k])), k


@pytest.mark.parametrize("W,H", SHAPES)
def test_rounds_1_gives_the_rules_first_rounds(W, H):
    """One tiled round per field settles nothing that crosses a tile border.  Through the class every robot is parked
    (RRT_FIELD_UNSETTLED) and nobody claims; with settled fields and a budget of one round per claim, claims_settled is 0 and the
    claims made are exactly the rule's first n_claims rounds."""
    ev, gain, start, want = scene(W, H)
    got = _run(ev, gain, start, rounds=1)
    assert got["claims_settled"].tolist() == [0] and got["n_claims"].tolist() == [0] and (got["claim_round"] == -1).all()
    assert got["status"].tolist() == [lipmpc.RRT_FIELD_UNSETTLED] * 4 and (got["sub_goals"] == SENTINEL).all()
    # the settled plan first (rounds=None, no claim allowed), then the claim call alone with one round per claim
    pl = _planner(gain, max_claims=0)
    out = _buffers(4, W, H)
    got = _run(ev, gain, start, pl=pl, out=out)
    assert got["usettled"].tolist() == [1] and got["n_claims"].tolist() == [0]
    org, cs, org_c, cell_c = pl._placement(ORIGIN, CELL)
    pl.max_claims, pl.rounds = 64, 1
    pl._gain_claims(4, W, H, torch.as_tensor(start, device="cuda"), None, org_c, cell_c, 64, out)
    pl._target(out, org, cs, H)
    torch.cuda.synchronize()
    got = U.host(out)
    n = int(got["n_claims"][0])
    print("n_claims with one round per claim:", n, "of", want["n_claims"])
    assert got["claims_settled"].tolist() == [0] and n < want["n_claims"]
    U.same(got, U.expected(ev, start, R_CLAIM, *GAIN, max_claims=n, gain=gain, informed=want["informed"]), 64)
    # growing budgets on the SAME buffers: a prefix of the rule's rounds while claims_settled is 0, the oracle's answer once it is 1
    seen = [(1, n, 0)]
    for budget in range(2, 8):
        pl.rounds = budget
        pl._gain_claims(4, W, H, torch.as_tensor(start, device="cuda"), None, org_c, cell_c, 64, out)
        pl._target(out, org, cs, H)
        torch.cuda.synchronize()
        got = U.host(out)
        n, ok = int(got["n_claims"][0]), int(got["claims_settled"][0])
        seen.append((budget, n, ok))
        U.same(got, want if ok else U.expected(ev, start, R_CLAIM, *GAIN, max_claims=n, gain=gain, informed=want["informed"]), 64)
        assert ok or n < want["n_claims"]
    print("budget, n_claims, claims_settled:", seen)
    assert [n for _, n, _ in seen] == sorted(n for _, n, _ in seen) and seen[-1][1:] == (want["n_claims"], 1), seen


def _kernel_nodes(enqueue):
    """The nodes of the graph a stream capture of ``enqueue(stream)`` gives: every launch of the call is one kernel node."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    stream = torch.cuda.Stream()
    handle, graph, n = C.c_void_p(stream.cuda_stream), C.c_void_p(), C.c_size_t()
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(handle, 2) == 0           # hipStreamCaptureModeRelaxed
    try:
        enqueue(stream.cuda_stream)
    finally:
        assert hip.hipStreamEndCapture(handle, C.byref(graph)) == 0
    assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0
    assert hip.hipGraphDestroy(graph) == 0
    return n.value


def test_kernel_nodes_of_a_captured_call_equal_the_formula():
    """max_claims * (max_rounds + 4) + 3 launches, whatever the fleet needs -- the tiled claim call's count; and a captured plan's
    replay gives the oracle's bits."""
    import ctypes as C
    W, H = SHAPES[1]
    ev, gain, start, want = scene(W, H)
    rounds, max_claims = -(-W // TW) - (-H // TH) + 2, 5
    pl = _planner(gain, max_claims, rounds)
    out = _buffers(4, W, H)
    _run(ev, gain, start, pl=pl, out=out)                      # outside the capture: the workspaces grow here
    org, cs, org_c, cell_c = pl._placement(ORIGIN, CELL)
    d_ev, d_start = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda")
    work = pl._claim_works[-1]
    common = dict(device=pl.device_index, B=4, W=W, H=H, origin=C.addressof(org_c), cell=C.addressof(cell_c), frontier=out["frontier"],
                  field=out["field"], settled=out["settled"], start=d_start, may_claim=None, r_inflate=2, r_claim=R_CLAIM, max_seg=pl.max_seg,
                  S_max=64, work=work, work_bytes=work.numel(), claims_settled=out["claims_settled"],
                  **{k: out[k] for k in ("sub_goals", "n_sub", "status", "path_cost", "target_cell", "claim_round", "n_claims")})
    for claims, budget in ((1, 1), (max_claims, rounds)):
        seeded = lambda s: lipmpc._lib.call("lipmpc_grid_frontier_assign_utility_tiled_batch", **common, max_claims=claims, max_rounds=budget,
                                            gain=out["gain"], w_gain=GAIN[1], g_cap=GAIN[2], min_gain=GAIN[3], target_gain=out["target_gain"],
                                            hip_stream=s)
        plain = lambda s: lipmpc._lib.call("lipmpc_grid_frontier_assign_tiled_batch", **common, max_claims=claims, max_rounds=budget, hip_stream=s)
        assert _kernel_nodes(seeded) == _kernel_nodes(plain) == claims * (budget + 4) + 3
    whole = torch.cuda.CUDAGraph()
    with torch.cuda.graph(whole):
        pl.plan(d_ev, d_start, origin=ORIGIN, cell=CELL, S_max=64, out=out)
    _poison(out)
    whole.replay()
    torch.cuda.synchronize()
    got = U.host(out)
    assert got["claims_settled"].tolist() == [1]
    U.same(got, want, 64)
