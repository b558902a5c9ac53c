"""GPU: claim hysteresis by tiles (lipmpc_grid_frontier_assign_keep_tiled_batch, through TiledCoordinatedFrontierPlanner.replan)
against tests/assign_keep_oracle.py and against the one-workgroup keep call, bit for bit, on maps of 2 x 2 tiles with one side one
cell over a tile edge.  Every buffer starts poisoned; each case first asserts on the oracle's record that it is what its name says."""
import numpy as np
import pytest

import assign_checks as AC
import assign_keep_checks as KC
import field_tiled_cases as T
import frontier_oracle as FR
import test_assign_tiled_gpu as AT
from assign_checks import CELL, ORIGIN, SENTINEL, T_FREE, T_OCC, bits, centres, open_field
from assign_keep_checks import GENEROUS, index

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

TW, TH = T.TW, T.TH
W, H = TW + 1, TH + 8                                         # 2 x 2 tiles: one row over the tile edge along i, eight columns along j
FAR = (W - 3, H - 3)                                          # the ring's far corner


def _planner(r_claim, max_claims, keep, r=2, mu=2, max_seg=None, rounds=None):
    return lipmpc.TiledCoordinatedFrontierPlanner(r_claim, max_claims, r_keep=keep[0], keep_ratio16=keep[1], keep_slack=keep[2], r_inflate=r,
                                                  min_unknown=mu, t_free=T_FREE, t_occ=T_OCC, max_seg=max_seg, rounds=rounds)


def _buffers(B, W, H, S_max):
    out = AT._buffers(B, W, H, S_max)
    out["kept"] = torch.full((B,), KC.POISON_I8, dtype=torch.int8, device="cuda")
    out["n_kept"] = torch.full((1,), AC.POISON_I32, dtype=torch.int32, device="cuda")
    return out


def _run(ev, start, r_claim, max_claims, prev, keep, r=2, mu=2, max_seg=None, S_max=64, may_claim=None, rounds=None):
    ev, start = np.ascontiguousarray(ev, np.int32), np.ascontiguousarray(np.asarray(start, np.float64).reshape(-1, 2))
    out = _buffers(len(start), *ev.shape, S_max)
    pl = _planner(r_claim, max_claims, keep, r, mu, max_seg, rounds)
    may = None if may_claim is None else torch.as_tensor(np.asarray(may_claim), device="cuda")
    prev = None if prev is None else torch.as_tensor(np.asarray(prev, np.int32), device="cuda")
    got = pl.replan(torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda"), origin=ORIGIN, cell=CELL, S_max=S_max, out=out,
                    may_claim=may, prev_target=prev)
    torch.cuda.synchronize()
    assert got is out and pl.last is out and "work" not in out
    return AC.host(out)


def _check(ev, start, r_claim, max_claims, prev, keep, **kw):
    """The tiled call settled, equal to the oracle and to the one-workgroup keep call."""
    want = KC.expected(ev, start, r_claim, max_claims, prev, keep, **kw)
    got = _run(ev, start, r_claim, max_claims, prev, keep, **kw)
    assert got["settled"].tolist() == [1] and got["claims_settled"].tolist() == [1]
    KC.same(got, want, kw.get("S_max", 64))
    one = KC.run(ev, start, r_claim, max_claims, prev, keep, **kw)
    for k in one:
        assert np.array_equal(bits(one[k]), bits(got[k])), k
    return got, want


def _side_by_side(n, i=TW - 8, j0=TH - 2):
    """n robots in a row across the tile border along j, six cells before the ring."""
    return centres([(i, j0 + k) for k in range(n)])


def test_no_previous_target_is_the_tiled_claim():
    ev, start = open_field(W, H), _side_by_side(4)
    got, want = _check(ev, start, 7, 64, None, (5, 16, 0))
    plain = AT._run(ev, start, 7, 64)
    for k in plain:
        assert np.array_equal(bits(got[k]), bits(plain[k])), k
    assert want["n_kept"] == 0 and want["n_claims"] == 4


def test_a_target_across_the_tiles_is_kept():
    got, want = _check(open_field(W, H), _side_by_side(2), 5, 64, [index(FAR, H), -1], GENEROUS)
    assert want["kept"].tolist() == [1, 0] and want["targets"][0] == FAR and want["claim_round"].tolist() == [0, 1]


@pytest.mark.parametrize("r_keep,anchored", [(3, True), (2, False)])
def test_receding_frontier(r_keep, anchored):
    got, want = _check(open_field(W, H), _side_by_side(2), 5, 64, [index((W - 6, TH + 1), H), -1], (r_keep, 1024, 4096))
    assert [r["anchor"] for r in want["attempts"]] == ([(W - 3, TH + 1)] if anchored else []) and want["n_kept"] == int(anchored)
    assert want["slots"] == 2 and want["n_claims"] == 2


def test_two_anchors_at_equal_distance_and_two_robots_with_one_target():
    ev, start = open_field(W, H), _side_by_side(2)
    got, want = _check(ev, start, 5, 64, [index((5, 5), H)] * 2, (3, 1024, 4096))
    assert [(r["robot"], r["anchor"]) for r in want["attempts"]] == [(0, (2, 5))] and want["kept"].tolist() == [1, 0]
    assert want["claim_round"].tolist() == [0, 1] and KC.spaced(want, 5)


def test_a_failed_test_a_mask_and_the_allowance_used_up_by_keeps():
    ev, start = open_field(W, H), _side_by_side(4)
    prev = [index(c, H) for c in (FAR, (2, 5), (2, H - 6), (W - 3, 8))]
    got, want = _check(ev, start, 3, 64, prev, (0, 16, 0), may_claim=np.array([1, 0, 1, 1], np.int8))      # strict: nobody keeps
    assert [r["robot"] for r in want["attempts"]] == [0, 2, 3] and want["n_kept"] == 0 and want["n_claims"] == 3 and want["slots"] == 6
    got, want = _check(ev, start, 3, 2, prev, GENEROUS)
    assert want["kept"].tolist() == [1, 1, 0, 0] and want["claim_round"].tolist() == [0, 1, -1, -1] and want["slots"] == 2
    got, want = _check(ev, start, 3, 5, prev, (0, 16, 0))      # five slots: four failed attempts, one round
    assert want["n_kept"] == 0 and want["n_claims"] == 1 and want["slots"] == 5


def test_anchor_in_a_sealed_off_room_and_an_overflow_keeper():
    ev = AC.two_rooms(W, H)
    got, want = _check(ev, centres([(5, 6), (6, 6)]), 3, 64, [index((16, 6), H), -1], GENEROUS, r=0)
    assert want["attempts"][0]["entry"] is None and want["slots"] == 3 and want["claim_round"].tolist() == [0, 1] and want["n_kept"] == 0
    ev = AC.block_in_field(W, H, (TW - 10, TH))
    start = centres([(TW - 8, TH), (TW - 8, TH + 1)])
    got, want = _check(ev, start, 6, 64, [index(FAR, H)] * 2, (3, 1024, 4096), max_seg=10, S_max=1)
    assert want["kept"].tolist() == [1, 0] and (want["status"] == FR.PATH_OVERFLOW).all() and (got["sub_goals"] == SENTINEL).all()
    assert [r["robot"] for r in want["attempts"]] == [0]


def test_candidates_past_the_mode_kernels_first_chunk():
    """1100 robots: the keep cursor crosses the mode kernel's chunk of 1024; robot 1 has a previous target that fails the test."""
    B = 1100
    ev = open_field(W, H)
    rng = np.random.default_rng(B)
    start = centres([(4, 9)])[0] + rng.uniform(-0.14, 0.14, (B, 2)) * np.array(CELL)
    prev = np.full(B, -1, np.int64)
    prev[[3, 1030, B - 1]] = [index(c, H) for c in ((W - 3, 10), (2, 30), (12, 2))]
    prev[1] = index(FAR, H)
    got, want = _check(ev, start, 6, 6, prev, (0, 64, 32))
    assert [(r["robot"], r["kept"]) for r in want["attempts"]] == [(1, False), (3, True), (1030, True), (B - 1, True)]
    assert want["n_claims"] == 5 and want["slots"] == 6


def test_a_budget_one_round_short_in_a_keep_slot_stops_the_call_and_a_larger_one_converges():
    """Robot 0 keeps the far corner of the ring: the field of that one cell crosses both tile borders and needs more rounds than
    the field of the whole ring.  Every budget runs on the same buffers; with claims_settled == 0 the winners so far are the rule's
    first n_claims (GENEROUS: every attempt succeeds, so n_claims slots were spent), and the first budget that settles gives the
    oracle's answer, as does any larger one."""
    ev, start = open_field(W, H), centres([(5, 5), (5, 6), (6, 5)])
    prev = [index(FAR, H), -1, index((2, 5), H)]
    full = KC.expected(ev, start, 5, 64, prev, GENEROUS)
    assert full["kept"].tolist() == [1, 0, 1] and full["n_claims"] == 3
    pl = _planner(5, 64, GENEROUS)
    out = _buffers(3, W, H, 64)
    d_ev, d_start, d_prev = (torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in (ev, start, np.asarray(prev, np.int32)))
    pl.rounds = None
    lipmpc.FrontierPlanner.plan(pl, d_ev, d_start, ORIGIN, CELL, 64, out)
    org, cs, org_c, cell_c = pl._placement(ORIGIN, CELL)
    seen = []
    for budget in range(1, 7):
        pl.rounds = budget
        pl._keep_claims(3, W, H, d_start, None, d_prev, org_c, cell_c, 64, out)
        pl._target(out, org, cs, H)
        torch.cuda.synchronize()
        got = AC.host(out)
        n, ok = int(got["n_claims"][0]), int(got["claims_settled"][0])
        seen.append((budget, n, ok))
        KC.same(got, full if ok else KC.expected(ev, start, 5, n, prev, GENEROUS), 64)
        assert ok or n < full["n_claims"]
    print("budget, n_claims, claims_settled:", seen)
    first = next(k for k, (_, _, ok) in enumerate(seen) if ok)
    assert first > 0 and seen[first - 1][1] == 0              # one round short: the keep slot of robot 0 did not settle, nobody won
    assert all(ok == 1 and n == 3 for _, n, ok in seen[first:])
    # rounds=None doubles the budget by itself
    KC.same(_run(ev, start, 5, 64, prev, GENEROUS), full, 64)


def test_graph_replay_with_fixed_rounds():
    ev, start = open_field(W, H), _side_by_side(4)
    prev = [index(FAR, H), -1, index((2, 5), H), -1]
    want = KC.expected(ev, start, 7, 6, prev, GENEROUS)
    pl = _planner(7, 6, GENEROUS, rounds=4)                   # 2 x 2 tiles of an open rectangle: a path changes tile at most twice
    out = _buffers(4, W, H, 64)
    d_ev, d_start, d_prev = (torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in (ev, start, np.asarray(prev, np.int32)))
    plan = lambda: pl.replan(d_ev, d_start, origin=ORIGIN, cell=CELL, S_max=64, out=out, prev_target=d_prev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan()                                                 # warm-up outside the capture: the workspaces grow here
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan()
    for _ in range(2):
        AT._poison(out)
        out["kept"].fill_(KC.POISON_I8)
        out["n_kept"].fill_(AC.POISON_I32)
        graph.replay()
        torch.cuda.synchronize()
        got = AC.host(out)
        assert got["settled"].tolist() == [1] and got["claims_settled"].tolist() == [1]
        KC.same(got, want, 64)


# -- the one-workgroup test's remaining cases, on the 2 x 2-tile map: the tiled kernels carry their own callers of the anchor search,
# -- the "is a cell" test, the keep test and the snap -------------------------------------------------------------------------------
@pytest.mark.parametrize("none", [-1, "cells", KC.K.INT32_MAX, -(1 << 31)])
def test_previous_targets_that_are_no_cell_mean_none(none):
    ev, start = open_field(W, H), _side_by_side(4)
    prev = np.full(4, W * H if none == "cells" else none, np.int64).astype(np.int32)
    got, want = _check(ev, start, 7, 64, prev, (5, 16, 0))
    plain = AT._run(ev, start, 7, 64)
    for k in plain:
        assert np.array_equal(bits(got[k]), bits(plain[k])), k
    assert want["attempts"] == [] and not got["kept"].any() and got["n_kept"].tolist() == [0]


@pytest.mark.parametrize("keep,target,kept", [((0, 16, 25), (6, H - 3), 1), ((0, 16, 25), (W - 3, 53), 0), ((0, 16, 24), (6, H - 3), 0),
                                              ((0, 116, 0), (6, H - 3), 1), ((0, 116, 0), (W - 3, 53), 0), ((0, 115, 0), (6, H - 3), 0)])
def test_keep_test_at_equality_and_one_unit_above(keep, target, kept):
    """From (6, 40) the nearest frontier costs 20, the ring cell (6, 69) across the tile border 145 (29 axial moves) and (30, 53) 146
    (13 diagonal and 11 axial moves): 16 * 145 = 16 * 20 + 80 * 25 = 116 * 20 holds with equality, 16 * 146 is one cost unit above
    it, and one step less of either parameter fails 145 too."""
    got, want = _check(open_field(W, H), centres([(6, 40)]), 5, 64, [index(target, H)], keep)
    rec, = want["attempts"]
    assert rec["near"] == 20 and rec["cost"] == (145 if target == (6, H - 3) else 146) and rec["kept"] == bool(kept)
    over = 16 * rec["cost"] - (keep[1] * 20 + 80 * keep[2])
    assert over == 0 if kept else over == 16 if rec["cost"] == 146 else 0 < over <= 80
    assert got["kept"].tolist() == [kept] and want["n_claims"] == 1 and want["slots"] == 2 - kept


@pytest.mark.parametrize("r_keep", [6, 64])
def test_anchor_window_clipped_at_each_grid_edge(r_keep):
    """A known field with single unknown cells one step from every corner and edge (min_unknown 1: the outermost rows and columns
    are frontier): previous targets in the four corners and beside the four edges, whose windows reach over every end of the grid."""
    ev = np.full((W, H), -T_FREE, np.int32)
    for c in ((1, 1), (1, H - 2), (W - 2, 1), (W - 2, H - 2), (1, TH), (W - 2, TH - 1), (16, 1), (16, H - 2)):
        ev[c] = 0
    start = centres([(14 + k // 3, TH - 1 + k % 3) for k in range(8)])
    prev = [index(c, H) for c in ((0, 0), (0, H - 1), (W - 1, 0), (W - 1, H - 1), (0, TH - 3), (W - 1, TH + 2), (13, 0), (19, H - 1))]
    got, want = _check(ev, start, 3, 64, prev, (r_keep, 1024, 4096), r=0, mu=1)
    assert len(want["attempts"]) >= (8 if r_keep == 6 else 4) and want["n_kept"] == len(want["attempts"]) and KC.spaced(want, 3)
    if r_keep == 6:
        assert want["attempts"][0]["anchor"] == (0, 0) and want["attempts"][3]["anchor"] == (W - 1, H - 1)


@pytest.mark.parametrize("r_keep", [0, 64])
def test_smallest_and_largest_keep_radius(r_keep):
    ev, start = open_field(W, H), _side_by_side(2)
    got, want = _check(ev, start, 5, 64, [index((16, TH + 2), H), index((2, 8), H)], (r_keep, 1024, 4096))
    if r_keep == 0:
        assert [r["robot"] for r in want["attempts"]] == [1] and want["kept"].tolist() == [0, 1]
    else:
        assert want["attempts"][0]["anchor"] == (16, H - 3) and want["kept"].tolist() == [1, 1]      # three cells away, in another tile


def test_start_in_the_inflation_band_snaps_in_the_keep_field():
    """The solid cell where the four tiles meet; the robot beside it is blocked, (TW - 1, TH + 2) and (TW + 1, TH + 2) are equally
    near, and the field of the far anchor alone is lower at the second, where the nearest-frontier field sent it to another."""
    ev = AC.block_in_field(W + 20, H, (TW, TH))
    start = centres([(TW, TH + 1)])
    got, want = _check(ev, start, 12, 64, [index((W + 20 - 3, TH + 2), H)], GENEROUS)
    rec, = want["attempts"]
    assert want["nearest"]["field"][0][TW, TH + 1] == FR.INF and rec["kept"] and rec["entry"] == (TW + 1, TH + 2)
    assert rec["entry"] != AC.FO.snap(want["nearest"]["field"][0], (TW, TH + 1), 2)


def test_more_robots_than_a_wave():
    B = 65
    ev = open_field(W, H)
    rng = np.random.default_rng(B)
    start = centres([(4, 9)])[0] + rng.uniform(-0.14, 0.14, (B, 2)) * np.array(CELL)
    prev = np.full(B, -1, np.int64)
    prev[[3, 40, B - 1]] = [index(c, H) for c in ((W - 3, 10), (2, 30), (12, 2))]
    prev[1] = index(FAR, H)
    got, want = _check(ev, start, 6, 8, prev, (0, 64, 32))
    assert [(r["robot"], r["kept"]) for r in want["attempts"]] == [(1, False), (3, True), (40, True), (B - 1, True)]
    assert want["n_claims"] == 7 and want["slots"] == 8


# -- the launch count -----------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("max_claims,rounds", [(1, 1), (3, 4), (6, 2)])
def test_the_launch_count_is_the_documented_formula(max_claims, rounds):
    """max_claims * (max_rounds + 5) + 3 for the keep call, max_claims * (max_rounds + 4) + 3 for the existing tiled claim call,
    counted as the kernel nodes of a captured call."""
    import ctypes as C
    ev, start = open_field(W, H), _side_by_side(4)
    pl = _planner(7, max_claims, GENEROUS)
    out = _buffers(4, W, H, 64)
    d_ev, d_start = torch.as_tensor(ev, device="cuda"), torch.as_tensor(np.ascontiguousarray(start), device="cuda")
    d_prev = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    lipmpc.FrontierPlanner.plan(pl, d_ev, d_start, ORIGIN, CELL, 64, out)
    org, cs, org_c, cell_c = pl._placement(ORIGIN, CELL)
    pl.rounds = rounds
    pl._keep_claims(4, W, H, d_start, None, d_prev, org_c, cell_c, 64, out)                 # outside the capture: the workspace grows here
    pl._claims(4, W, H, d_start, None, org_c, cell_c, 64, out)
    torch.cuda.synchronize()
    work = pl._claim_works[-1]
    common = dict(device=pl.device_index, B=4, W=W, H=H, origin=C.addressof(org_c), cell=C.addressof(cell_c), frontier=out["frontier"],
                  field=out["field"], settled=out["settled"], start=d_start, may_claim=None, r_inflate=2, r_claim=7, max_claims=max_claims,
                  max_seg=pl.max_seg, S_max=64, work=work, work_bytes=work.numel(), max_rounds=rounds, claims_settled=out["claims_settled"],
                  **{k: out[k] for k in ("sub_goals", "n_sub", "status", "path_cost", "target_cell", "claim_round", "n_claims")})
    keep = lambda s: lipmpc._lib.call("lipmpc_grid_frontier_assign_keep_tiled_batch", **common, prev_target=d_prev, r_keep=0, keep_ratio16=1024,
                                      keep_slack=4096, kept=out["kept"], n_kept=out["n_kept"], hip_stream=s)
    plain = lambda s: lipmpc._lib.call("lipmpc_grid_frontier_assign_tiled_batch", **common, hip_stream=s)
    assert _kernel_nodes(keep) == max_claims * (rounds + 5) + 3
    assert _kernel_nodes(plain) == max_claims * (rounds + 4) + 3
