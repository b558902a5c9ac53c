"""GPU: the gain-seeded claims (lipmpc_grid_frontier_assign_utility_batch, through CoordinatedFrontierPlanner with the gain
keywords) against tests/assign_utility_oracle.py: EVERY output -- claim_round, n_claims, n_sub / status / target_cell / target_gain,
the doubles of path_cost, target and the WHOLE sub-goal buffer, and the fields of the plan that precedes the claims -- bit for bit,
on the smallest shapes at which the kernels can go wrong.  Every buffer starts poisoned."""
import numpy as np
import pytest

import assign_checks as AC
import assign_utility_checks as U
import assign_utility_oracle as AU
import frontier_oracle as FR
import gain_checks as K
from assign_checks import open_field
from gain_checks import CELL, HAND_MADE, ORIGIN, SENTINEL, T_FREE, T_OCC, bits, centres

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402


def _hand_gain(shape, seed=5, lo=-60, hi=160):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.int32)


def _side_by_side(n, i=6, j0=8):
    return centres([(i, j0 + k) for k in range(n)])


def test_gpu_hand_made_map():
    start = centres(((3, 4), (0, 3), (3, 6), (1, 3)))
    got, want = U.check(HAND_MADE, start, 2, 2, 16, 10, 0, r=0, mu=1)
    assert want["n_claims"] >= 2
    got, want = U.check(HAND_MADE, start, 2, 2, 16, 10, 0, r=0, mu=1, gain=_hand_gain(HAND_MADE.shape, 7, -5, 20))
    assert want["n_claims"] >= 2
    got, want = U.check(np.zeros((2, 2), np.int32), centres(((0, 0), (1, 1))), 1, 1, 16, 10, 0, r=0, mu=1)       # nothing known
    assert want["n_claims"] == 0 and (got["sub_goals"] == SENTINEL).all()


@pytest.mark.parametrize("gain_a", [74, 75, 76])
def test_gpu_corridor_terminal_test_inside_a_round(gain_a):
    ev, gain, want = U.corridor(gain_a)
    kw = K.CORRIDOR_KW
    U.check(ev, U.CORRIDOR_STARTS, U.CORRIDOR_R_CLAIM, kw["r_view"], kw["w_gain"], kw["g_cap"], kw["min_gain"], r=kw["r"], mu=kw["mu"],
            gain=gain, want=want)
    assert want["winners"] == [1, 0] and want["targets"][0] == (K.CORRIDOR_B if gain_a == 74 else K.CORRIDOR_A)


def test_gpu_fleet_case():
    """48 x 36, 130 starts with the special ones: robots that never claim keep the utility path call's rows."""
    ev, start = K.fleet_case()
    got, want = U.check(ev, start, 6, 5, 16, 60, 0)
    assert want["n_claims"] >= 4 and (want["claim_round"] == -1).sum() == 130 - want["n_claims"]
    got, want = U.check(ev, start, 6, 5, 40, 120, 0, gain=_hand_gain(ev.shape))            # stored gains below 0 and above g_cap
    assert want["n_claims"] >= 3
    got, want = U.check(ev, start, 6, 5, 16, 60, 16384)                                      # a min_gain that leaves no source
    assert want["n_claims"] == 0 and want["n_sources"][0] == 0 and int(got["n_claims"][0]) == 0


@pytest.mark.parametrize("params", U.UWALL_SETS)
def test_gpu_uwall(params):
    ev, _ = K.scanned_maps()
    want = U.uwall(*params)
    U.check(ev, U.UWALL_STARTS, U.UWALL_R_CLAIM, *params, origin=K.MAP_ORIGIN, cell=K.MAP_CELL, want=want)
    assert want["n_claims"] == 6


@pytest.mark.parametrize("max_claims,S_max,may", [(0, 64, None), (1, 64, None), (3, 64, None), (64, 1, None), (64, 64, (0, 1, 1, 0, 1, 1))])
def test_gpu_uwall_allowance_overflow_and_mask(max_claims, S_max, may):
    ev, _ = K.scanned_maps()
    may = None if may is None else np.array(may, np.int8)
    got, want = U.check(ev, U.UWALL_STARTS, U.UWALL_R_CLAIM, 30, 64, 600, 0, max_claims, S_max=S_max, may_claim=may, origin=K.MAP_ORIGIN,
                        cell=K.MAP_CELL)
    assert want["n_claims"] == (4 if may is not None else min(max_claims, 6))
    if S_max == 1:
        assert ((want["claim_round"] >= 0) & (want["status"] == FR.PATH_OVERFLOW)).any()


def _switch_map(W, H):
    ev = open_field(W, H, margin=3)
    ev[W // 2, 10:H - 10] = T_OCC
    gain = np.zeros((W, H), np.int32)
    gain[:W // 2] = 7                                          # the near side reveals little, the far side of the wall much
    gain[W // 2:] = 90
    return ev, gain, centres([(W // 2 - 6, H // 2), (W // 2 - 6, H // 2 + 1), (W // 2 - 7, H // 2)])


def test_gpu_each_side_of_the_lds_switch():
    """The largest map whose round field the kernel keeps in LDS and the first it relaxes in ``work``, by the oracle module's
    restatement of the kernel's own rule (another W than the assign kernels': 34 words, not 22); max_claims 2."""
    sizes = AU.sizes_at_the_lds_switch()
    assert sizes[0][1] == sizes[1][1] == 193
    for W, H in sizes:
        ev, gain, start = _switch_map(W, H)
        got, want = U.check(ev, start, 30, 4, 16, 100, 0, max_claims=2, S_max=16, gain=gain)
        assert want["n_claims"] == 2 and want["costs"][1] > want["costs"][0] > 100


def test_gpu_map_at_the_cap():
    """512 x 256 = 2^17 cells: a free room in the far corner, where the cell indices are the largest the call takes."""
    W, H = 512, 256
    ev = np.zeros((W, H), np.int32)
    ev[W - 70:W - 2, H - 60:H - 2] = -T_FREE
    gain = _hand_gain((W, H), 11, 0, 200)
    start = centres([(W - 40, H - 30), (W - 40, H - 31), (W - 41, H - 30)])
    got, want = U.check(ev, start, 25, 4, 16, 150, 0, max_claims=3, gain=gain)
    assert want["n_claims"] == 3 and min(want["target_cell"]) > (W - 71) * H


@pytest.mark.parametrize("B", [1, 1025])
def test_gpu_one_robot_and_more_than_the_workgroup(B):
    """Robot B - 1 is the only one near the far side: it must win its round from the stride's last pass."""
    ev = open_field(24, 20)
    rng = np.random.default_rng(B)
    start = centres([(4, 9)])[0] + rng.uniform(-0.14, 0.14, (B, 2)) * np.array(CELL)
    start[B - 1] = centres([(20, 10)])[0]
    got, want = U.check(ev, start, 6, 4, 16, 30, 0, max_claims=8)
    assert want["n_claims"] == min(B, 8) and want["claim_round"][B - 1] >= 0 and (want["claim_round"] == -1).sum() == B - min(B, 8)


def _captured(pl, ev, start, out, S_max):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pl.plan(ev, start, origin=ORIGIN, cell=CELL, S_max=S_max, out=out)         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pl.plan(ev, start, origin=ORIGIN, cell=CELL, S_max=S_max, out=out)
    return graph


def test_gpu_graph_replay_and_repeat_give_the_same_bits():
    ev, start = open_field(40, 44), _side_by_side(6, i=8, j0=18)
    eager = [U.run(ev, start, 7, 6, 16, 60) for _ in range(2)]
    for k in eager[0]:
        assert np.array_equal(bits(eager[0][k]), bits(eager[1][k])), k
    assert int(eager[0]["n_claims"][0]) >= 3
    pl = U.planner(7, 6, 16, 60)
    out = U.buffers(6, 40, 44, 64)
    d_ev, d_start = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda")      # (alive as long as the graph reads them)
    graph = _captured(pl, d_ev, d_start, out, 64)
    U.poison(out)                                              # poisoned again, in the memory the graph writes
    out["work"].view(torch.int32).zero_()                      # (another poison for the scratch: zeros look like sources)
    graph.replay()
    torch.cuda.synchronize()
    got = U.host(out)
    for k in eager[0]:
        assert np.array_equal(bits(got[k]), bits(eager[0][k])), k


@pytest.mark.parametrize("case", ["fleet", "uwall"])
def test_gpu_w_gain_0_is_the_plain_claim_on_the_device(case):
    """w_gain 0 / min_gain 0 against lipmpc_grid_frontier_assign_batch run on the device here: every output the two share."""
    if case == "fleet":
        (ev, start), origin, cell, r_claim = K.fleet_case(), ORIGIN, CELL, 6
    else:
        ev, start, origin, cell, r_claim = K.scanned_maps()[0], U.UWALL_STARTS, K.MAP_ORIGIN, K.MAP_CELL, U.UWALL_R_CLAIM
    plain = AC.run(ev, start, r_claim, 64, origin=origin, cell=cell)
    got = U.run(ev, start, r_claim, 10, 0, 100, 0, origin=origin, cell=cell)
    assert int(plain["n_claims"][0]) >= 4
    for k in plain:
        assert np.array_equal(bits(got[k]), bits(plain[k])), k
    assert np.array_equal(got["ufield"], got["field"]) and np.array_equal(got["n_sources"], got["n_frontier"])


def test_gpu_planner_arguments():
    ev, start = open_field(20, 24), _side_by_side(3)
    d_ev = torch.as_tensor(ev, device="cuda")
    pl = U.planner(5, 4, 16, 30)
    fresh = pl.plan(d_ev, start, origin=ORIGIN, cell=CELL)      # fresh buffers: rows past n_sub are 0
    torch.cuda.synchronize()
    assert set(fresh) == set(lipmpc.planner.assign_utility_outputs(3, 20, 24, 64)) and fresh["n_claims"].tolist() == [3]
    assert all((fresh["sub_goals"][b, int(fresh["n_sub"][b]):] == 0).all() for b in range(3))
    assert tuple(pl.plan(d_ev, np.zeros((0, 2)), origin=ORIGIN, cell=CELL)["target_gain"].shape) == (0,)
    with pytest.raises(ValueError):
        pl.plan(torch.zeros((3, 20, 24), dtype=torch.int32, device="cuda"), start, origin=ORIGIN, cell=CELL)      # one map per robot
    with pytest.raises(ValueError):
        pl.replan(d_ev, start, origin=ORIGIN, cell=CELL, prev_target=[1, 2, 3])
    wave = U.planner(5, 4, 16, 30, paths="wave").plan(d_ev, start, origin=ORIGIN, cell=CELL)       # the utility path call alone
    torch.cuda.synchronize()
    wave, fresh = U.host(wave), U.host(fresh)
    for k in fresh:
        assert np.array_equal(bits(wave[k]), bits(fresh[k])), k
