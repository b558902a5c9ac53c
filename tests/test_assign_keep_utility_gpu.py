"""GPU: claim hysteresis for the gain-seeded claims (lipmpc_grid_frontier_assign_keep_utility_batch, through
GainKeepFrontierPlanner.replan) against tests/assign_keep_utility_oracle.py: EVERY output -- claim_round, n_claims, kept, n_kept,
n_sub / status / target_cell / target_gain, the doubles of path_cost, target and the WHOLE sub-goal buffer, and the fields of the plan
that precedes the claims -- bit for bit, on the smallest shapes at which the kernels can go wrong.  Every buffer starts poisoned.  Each
case first asserts on the oracle's record that it is the case its name says."""
import numpy as np
import pytest

import assign_keep_checks as KC
import assign_keep_utility_checks as C
import assign_keep_utility_oracle as KU
import assign_utility_checks as U
import frontier_oracle as FR
import gain_checks as K
from assign_checks import open_field
from assign_keep_utility_checks import GENEROUS, index
from gain_checks import CELL, ORIGIN, SENTINEL, T_FREE, T_OCC, bits, centres

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402


def _hand_gain(shape, seed=5, lo=-60, hi=160):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.int32)


def _side_by_side(n, i=6, j0=8):
    return centres([(i, j0 + k) for k in range(n)])


def test_gpu_two_pockets_the_keep_rule_keeps_what_the_memoryless_rule_gives_away():
    ev, gain = C.two_pockets()
    prev = [index(C.POCKET_FAR, 44), -1]
    got, want = C.check(ev, C.POCKET_STARTS, C.POCKET_R_CLAIM, C.POCKET_GAIN, prev, (6, 24, 8), gain=gain)
    memoryless = U.expected(ev, C.POCKET_STARTS, C.POCKET_R_CLAIM, *C.POCKET_GAIN, gain=gain)
    assert memoryless["target_cell"].tolist() == [index(C.POCKET_NEAR, 44), index(C.POCKET_FAR, 44)]
    assert got["target_cell"].tolist() == [index(C.POCKET_FAR, 44), index(C.POCKET_NEAR, 44)] and got["kept"].tolist() == [1, 0]
    assert got["target_gain"].tolist() == [110, 60] and got["claim_round"].tolist() == [0, 1]


@pytest.mark.parametrize("slack,kept", [(5, 1), (4, 0)])
def test_gpu_corridor_keep_test_at_equality_and_one_slack_less(slack, kept):
    ev, gain = C.kept_corridor()
    got, want = C.check(ev, C.KEPT_START, 2, C.KEPT_GAIN, [index(C.KEPT_A, 16)], (0, 32, slack), gain=gain, **C.KEPT_KW)
    rec, = want["attempts"]
    assert (rec["cost"], rec["near"]) == (115, 45) and 16 * 115 - (32 * 45 + 80 * slack) == (0 if kept else 80)
    assert got["kept"].tolist() == [kept] and got["target_cell"].tolist() == [index(C.KEPT_A if kept else (1, 4), 16)]
    assert got["path_cost"].tolist() == [11.0 if kept else 3.0] and want["slots"] == 2 - kept


@pytest.mark.parametrize("gain_a", [0, -7])
def test_gpu_previous_target_whose_gain_fell_below_min_gain(gain_a):
    """The previous target A is no source any more (gain below min_gain 1, or negative): within r_keep 3 nothing is left, so no
    slot is spent; within r_keep 8 the anchor is B, elsewhere."""
    ev, gain = C.kept_corridor(gain_a)
    got, want = C.check(ev, C.KEPT_START, 2, C.KEPT_GAIN, [index(C.KEPT_A, 16)], (3, 1024, 4096), gain=gain, **C.KEPT_KW)
    assert want["attempts"] == [] and want["slots"] == want["n_claims"] == 1 and got["kept"].tolist() == [0]
    got, want = C.check(ev, C.KEPT_START, 2, C.KEPT_GAIN, [index(C.KEPT_A, 16)], (8, 1024, 4096), gain=gain, **C.KEPT_KW)
    assert want["attempts"][0]["anchor"] == (1, 4) and got["kept"].tolist() == [1] and got["target_gain"].tolist() == [70]


def test_gpu_a_keepers_disc_removes_the_next_robots_anchor():
    ev, gain = C.two_pockets()
    prev = [index(C.POCKET_FAR, 44)] * 2
    got, want = C.check(ev, C.POCKET_STARTS, C.POCKET_R_CLAIM, C.POCKET_GAIN, prev, (3, 1024, 4096), gain=gain)
    assert [r["robot"] for r in want["attempts"]] == [0] and want["kept"].tolist() == [1, 0] and want["slots"] == 2
    assert got["claim_round"].tolist() == [0, 1] and got["target_cell"][1] == index(C.POCKET_NEAR, 44)


@pytest.mark.parametrize("max_claims", [0, 1, 2, 3])
def test_gpu_failed_attempts_use_up_max_claims(max_claims):
    """Robots 0 and 1 have previous targets that fail the tightest test; they spend a slot each, and the rounds get what is left."""
    ev, start = open_field(20, 24), _side_by_side(3)
    prev = [index((17, 12), 24), index((2, 20), 24), -1]
    got, want = C.check(ev, start, 3, (4, 16, 60, 0), prev, (0, 16, 0), max_claims=max_claims)
    assert len(want["attempts"]) == min(max_claims, 2) and want["n_kept"] == 0 and want["n_claims"] == max(max_claims - 2, 0)
    assert want["slots"] == max_claims and int(got["n_claims"][0]) == max(max_claims - 2, 0)


@pytest.mark.parametrize("r_keep", [0, 64])
def test_gpu_smallest_and_largest_keep_radius_window_clipped_at_a_grid_edge(r_keep):
    """Robot 0's previous target is an inner cell, robot 1's a ring cell beside the edge, robot 2's the corner cell (0, 0): r_keep
    0 takes the very cell or nothing; r_keep 64 searches a window larger than the map, clipped at every edge."""
    ev, start = open_field(20, 24), _side_by_side(3)
    prev = [index((10, 12), 24), index((2, 8), 24), 0]
    got, want = C.check(ev, start, 5, (4, 16, 60, 0), prev, (r_keep, 1024, 4096))
    if r_keep == 0:
        assert [r["robot"] for r in want["attempts"]] == [1] and want["kept"].tolist() == [0, 1, 0]
    else:
        assert [r["robot"] for r in want["attempts"]] == [0, 1, 2] and want["kept"].tolist() == [1, 1, 1]
        assert want["attempts"][2]["anchor"] == (2, 2)


def test_gpu_nothing_known():
    got, want = C.check(np.zeros((2, 2), np.int32), centres(((0, 0), (1, 1))), 1, (1, 16, 10, 0), [0, 3], GENEROUS, r=0, mu=1)
    assert want["n_claims"] == 0 and want["slots"] == 0 and (got["sub_goals"] == SENTINEL).all() and got["n_kept"].tolist() == [0]


def test_gpu_fleet_case():
    """48 x 36, 130 starts with the special ones; previous targets that include wall cells, -1, W * H, INT32 min and INT32 max."""
    ev, start = K.fleet_case()
    prev = C.fleet_prev()
    got, want = C.check(ev, start, 6, (5, 16, 60, 0), prev, (6, 24, 8))
    assert want["n_claims"] >= 4 and want["n_kept"] >= 1 and len(want["attempts"]) > want["n_kept"]
    assert (want["claim_round"] == -1).sum() == 130 - want["n_claims"]
    got, want = C.check(ev, start, 6, (5, 65535, 16384, 0), prev, (10, 64, 32), gain=_hand_gain(ev.shape))     # the largest seed;
    assert want["n_claims"] >= 3 and want["n_kept"] >= 1                                    # stored gains below 0 and above g_cap
    assert max(r["cost"] for r in want["attempts"] if r["cost"] is not None) > 1 << 25
    got, want = C.check(ev, start, 6, (5, 16, 60, 16384), prev, GENEROUS)                   # a min_gain that leaves no source
    assert want["n_claims"] == 0 and want["attempts"] == [] and int(got["n_kept"][0]) == 0


def _switch_map(W, H):
    ev = open_field(W, H, margin=3)
    ev[W // 2, 10:H - 10] = T_OCC
    gain = np.zeros((W, H), np.int32)
    gain[:W // 2] = 7                                          # the near side reveals little, the far side of the wall much
    gain[W // 2:] = 90
    return ev, gain, centres([(W // 2 - 6, H // 2), (W // 2 - 6, H // 2 + 1), (W // 2 - 7, H // 2)])


def test_gpu_each_side_of_the_lds_switch():
    """The largest map whose slot field the kernel keeps in LDS and the first it relaxes in ``work``, by the oracle module's
    restatement of the kernel's own rule (48 words: another W than the sibling kernels' only where their rules differ); 3 slots."""
    sizes = KU.sizes_at_the_lds_switch()
    assert sizes[0][1] == sizes[1][1] == 193
    for W, H in sizes:
        ev, gain, start = _switch_map(W, H)
        got, want = C.check(ev, start, 30, (4, 16, 100, 0), [-1, index((3, 20), H), -1], GENEROUS, max_claims=3, S_max=16, gain=gain)
        assert want["kept"].tolist() == [0, 1, 0] and want["n_claims"] == 3 and want["slots"] == 3


def test_gpu_map_at_the_cap():
    """512 x 256 = 2^17 cells: a free room in the far corner, where the cell indices are the largest the call takes."""
    W, H = 512, 256
    ev = np.zeros((W, H), np.int32)
    ev[W - 70:W - 2, H - 60:H - 2] = -T_FREE
    gain = _hand_gain((W, H), 11, 0, 200)
    start = centres([(W - 40, H - 30), (W - 40, H - 31), (W - 41, H - 30)])
    prev = [index((W - 3, H - 3), H), -1, index((W - 71, H - 30), H)]
    got, want = C.check(ev, start, 25, (4, 16, 150, 0), prev, (6, 1024, 4096), max_claims=3, gain=gain)
    assert want["n_claims"] == 3 and want["n_kept"] == 2 and min(want["target_cell"]) > (W - 72) * H


@pytest.mark.parametrize("B", [1, 1025])
def test_gpu_one_robot_and_keep_candidates_across_the_chunk_cursor(B):
    """B = 1025: keep candidates at indices 1023 (the last of the first chunk of robots) and 1024 (the first of the second)."""
    ev = open_field(24, 20)
    rng = np.random.default_rng(B)
    start = centres([(4, 9)])[0] + rng.uniform(-0.14, 0.14, (B, 2)) * np.array(CELL)
    prev = np.full(B, -1, np.int64)
    if B == 1:
        prev[0] = index((21, 10), 20)
    else:
        prev[[1023, 1024]] = [index((21, 10), 20), index((12, 17), 20)]
    got, want = C.check(ev, start, 6, (4, 16, 30, 0), prev, GENEROUS, max_claims=8)
    assert [(r["robot"], r["kept"]) for r in want["attempts"]] == ([(0, True)] if B == 1 else [(1023, True), (1024, True)])
    assert want["n_claims"] == min(B, 8) and (want["claim_round"] == -1).sum() == B - min(B, 8)


def test_gpu_overflow_keeper_still_takes_its_disc():
    ev, gain = C.two_pockets()
    prev = [index(C.POCKET_FAR, 44)] * 2
    got, want = C.check(ev, C.POCKET_STARTS, C.POCKET_R_CLAIM, C.POCKET_GAIN, prev, (3, 1024, 4096), max_seg=10, S_max=1, gain=gain)
    assert want["kept"].tolist() == [1, 0] and (want["status"] == FR.PATH_OVERFLOW).all() and (want["n_sub"] == 0).all()
    assert [r["robot"] for r in want["attempts"]] == [0] and (got["sub_goals"] == SENTINEL).all()


def test_gpu_a_robot_that_may_not_claim_is_never_kept():
    ev, start = open_field(20, 24), _side_by_side(3)
    prev = [index((17, 12), 24)] * 3
    got, want = C.check(ev, start, 3, (4, 16, 60, 0), prev, GENEROUS, may_claim=np.array([0, 1, 1], np.int8))
    assert want["kept"].tolist() == [0, 1, 0] and want["claim_round"][0] == -1 and [r["robot"] for r in want["attempts"]] == [1]
    assert got["target_cell"][0] == want["informed"]["target_cell"][0]


@pytest.mark.parametrize("none", [None, -1, "cells", (1 << 31) - 1, -(1 << 31)])
def test_gpu_no_previous_target_is_the_gain_seeded_claim_on_the_device(none):
    """Against lipmpc_grid_frontier_assign_utility_batch run on the device here: every output the two calls share, bit for bit."""
    ev, _ = K.scanned_maps()
    prev = None if none is None else np.full(6, ev.size if none == "cells" else none, np.int64).astype(np.int32)
    seeded = U.run(ev, U.UWALL_STARTS, U.UWALL_R_CLAIM, 15, 16, 120, 8, origin=K.MAP_ORIGIN, cell=K.MAP_CELL)
    got = C.run(ev, U.UWALL_STARTS, U.UWALL_R_CLAIM, (15, 16, 120, 8), prev, (6, 24, 8), origin=K.MAP_ORIGIN, cell=K.MAP_CELL)
    assert int(seeded["n_claims"][0]) == 6
    for k in seeded:
        assert np.array_equal(bits(got[k]), bits(seeded[k])), k
    assert not got["kept"].any() and got["n_kept"].tolist() == [0]


@pytest.mark.parametrize("case", ["fleet", "field"])
def test_gpu_w_gain_0_is_the_plain_keep_call_on_the_device(case):
    """w_gain 0 / min_gain 0 against lipmpc_grid_frontier_assign_keep_batch run on the device here: every output, kept and n_kept
    included (the gain call's output is >= 0, so ufield == field)."""
    if case == "fleet":
        (ev, start), r_claim, prev, keep = K.fleet_case(), 6, C.fleet_prev(), (6, 24, 8)
    else:
        ev, start, r_claim, keep = open_field(40, 44), _side_by_side(6, 8, 18), 7, (3, 24, 4)
        prev = KC.AC.expected(ev, start, 7, 64)["target_cell"]
    plain = KC.run(ev, start, r_claim, 64, prev, keep)
    got = C.run(ev, start, r_claim, (10, 0, 100, 0), prev, keep)
    assert int(plain["n_kept"][0]) >= 1 and int(plain["n_claims"][0]) > int(plain["n_kept"][0])
    for k in plain:
        assert np.array_equal(bits(got[k]), bits(plain[k])), k
    assert np.array_equal(got["ufield"], got["field"])


def _captured(pl, ev, start, prev, out):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pl.replan(ev, start, origin=ORIGIN, cell=CELL, out=out, prev_target=prev)         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pl.replan(ev, start, origin=ORIGIN, cell=CELL, out=out, prev_target=prev)
    return graph


def test_gpu_graph_replay_and_repeat_give_the_same_bits():
    ev, start = open_field(40, 44), _side_by_side(6, 8, 18)
    gainp, keep = (6, 16, 60, 0), (3, 24, 4)
    prev = U.expected(ev, start, 7, *gainp)["target_cell"]
    eager = [C.run(ev, start, 7, gainp, prev, keep) for _ in range(2)]
    for k in eager[0]:
        assert np.array_equal(bits(eager[0][k]), bits(eager[1][k])), k
    assert 0 < eager[0]["n_kept"][0] <= 6 and int(eager[0]["n_claims"][0]) >= 3
    pl = C.planner(7, gainp, keep)
    out = C.buffers(6, 40, 44, 64)
    d_ev, d_start = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda")      # (alive as long as the graph reads them)
    d_prev = torch.as_tensor(prev, device="cuda")
    graph = _captured(pl, d_ev, d_start, d_prev, out)
    for zero_work in (False, True):
        C.poison(out)                                          # poisoned again, in the memory the graph writes
        if zero_work:
            out["work"].view(torch.int32).zero_()              # (another poison for the scratch: zeros look like sources)
        graph.replay()
        torch.cuda.synchronize()
        got = C.host(out)
        for k in eager[0]:
            assert np.array_equal(bits(got[k]), bits(eager[0][k])), k


def test_gpu_planner_arguments():
    ev, start = open_field(20, 24), _side_by_side(3)
    d_ev = torch.as_tensor(ev, device="cuda")
    pl = C.planner(5, (4, 16, 30, 0), GENEROUS)
    prev = [index((17, 12), 24), -1, -1]
    fresh = pl.replan(d_ev, start, origin=ORIGIN, cell=CELL, prev_target=prev)          # fresh buffers, a list of Python ints
    torch.cuda.synchronize()
    assert set(fresh) == set(lipmpc.planner.assign_utility_outputs(3, 20, 24, 64)) | {"kept", "n_kept"}
    assert fresh["kept"].tolist() == [1, 0, 0] and fresh["n_kept"].tolist() == [1] and fresh["n_claims"].tolist() == [3]
    assert all((fresh["sub_goals"][b, int(fresh["n_sub"][b]):] == 0).all() for b in range(3))
    plain = pl.plan(d_ev, start, origin=ORIGIN, cell=CELL)      # plan = replan without previous targets: the gain-seeded parent's
    torch.cuda.synchronize()
    old = U.planner(5, 4, 16, 30).plan(d_ev, start, origin=ORIGIN, cell=CELL)
    torch.cuda.synchronize()
    assert plain["kept"].tolist() == [0, 0, 0] and all(torch.equal(plain[k], old[k]) for k in old if k != "work")
    assert tuple(pl.replan(d_ev, np.zeros((0, 2)), origin=ORIGIN, cell=CELL)["kept"].shape) == (0,)
    wave = C.planner(5, (4, 16, 30, 0), GENEROUS, paths="wave").replan(d_ev, start, origin=ORIGIN, cell=CELL, prev_target=prev)
    torch.cuda.synchronize()
    wave, fresh = C.host(wave), C.host(fresh)
    for k in fresh:
        assert np.array_equal(bits(wave[k]), bits(fresh[k])), k
    with pytest.raises(ValueError):
        pl.replan(torch.zeros((3, 20, 24), dtype=torch.int32, device="cuda"), start, origin=ORIGIN, cell=CELL)      # one map per robot
    for bad in ([1, 2], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            pl.replan(d_ev, start, origin=ORIGIN, cell=CELL, prev_target=bad)
    with pytest.raises(ValueError):
        lipmpc.GainKeepFrontierPlanner(5, r_view=4, w_gain=16, g_cap=30, r_keep=0, keep_ratio16=16, keep_slack=0, r_clear=3, w_clear=40,
                                       t_free=T_FREE, t_occ=T_OCC)
