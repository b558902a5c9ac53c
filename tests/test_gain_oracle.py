"""CPU: tests/gain_oracle.py, the numpy restatement of the informed explorer's three contracts, against what the contracts imply."""
import os

import numpy as np
import pytest

import field_oracle as FO
import frontier_oracle as FR
import gain_checks as K
import gain_oracle as G
from gain_checks import CELL, HAND_MADE, ORIGIN, T_FREE, T_OCC, bits as _bits

SIX_STARTS = np.concatenate([np.array(K.SCAN_AT), np.array(K.SCAN_AT) + (0.3, -0.25)])


@pytest.mark.parametrize("r,disc_minus_one", sorted(G.OPEN_MAP_GAINS.items()))
def test_open_map_gain_is_the_disc(r, disc_minus_one):
    """On an all-unknown map the fan to the ring reaches every cell of the disc."""
    ev = K.one_free_cell(r)
    fr = np.zeros(ev.shape, np.uint8)
    fr[r + 1, r + 1] = 1
    g = G.gain(ev, T_FREE, T_OCC, fr, r)
    disc = sum(a * a + b * b <= r * r for a in range(-r, r + 1) for b in range(-r, r + 1))
    assert g[r + 1, r + 1] == disc_minus_one == disc - 1 and g.sum() == disc_minus_one


def test_gain_stops_at_solid_and_reads_the_given_frontier():
    ev = np.zeros((9, 9), np.int32)
    ev[4, 4] = -T_FREE
    ev[4, 6] = T_OCC                                           # a solid cell two to the right: it and what lies behind it are not seen
    fr = np.zeros((9, 9), np.uint8)
    fr[4, 4] = 1
    open_ = G.gain(np.where(ev == T_OCC, 0, ev), T_FREE, T_OCC, fr, 4)[4, 4]
    g = G.gain(ev, T_FREE, T_OCC, fr, 4)
    assert g[4, 4] < open_ - 1 and (g == 0).sum() == 80
    fr[0, 0] = 1                                               # not a frontier cell of this map: the call takes the given bytes
    assert G.gain(ev, T_FREE, T_OCC, fr, 4)[0, 0] > 0
    ev[:] = -T_FREE                                            # nothing unknown: nothing to gain
    assert not G.gain(ev, T_FREE, T_OCC, fr, 4).any()


def test_scanned_map_gains_spread_widely():
    """The figures of the issue: 153 frontier cells whose gain is 18 ... 174 at a view radius of 10 and 90 ... 1195 at 30."""
    shared, _ = K.scanned_maps()
    _, fr, n = FR.field(shared, T_FREE, T_OCC, 2, 2)
    assert n == 153
    for r, lo, hi in ((10, 18, 174), (30, 90, 1195)):
        g = G.gain(shared, T_FREE, T_OCC, fr, r)
        assert (g[fr == 0] == 0).all() and g[fr != 0].min() == lo and g[fr != 0].max() == hi


def _identity(ev, start, origin, cell, r, mu, max_seg=None, S_max=64):
    near = FR.plan_batch(ev, T_FREE, T_OCC, origin, cell, start, r, mu, max_seg, S_max)
    got = G.plan_batch(ev, T_FREE, T_OCC, origin, cell, start, 3, 0, 50, 0, r, mu, max_seg, S_max, nearest=near)
    assert np.array_equal(got["ufield"], near["field"]) and np.array_equal(got["n_sources"], near["n_frontier"])
    for k in ("status", "n_sub", "target_cell"):
        assert np.array_equal(got[k], near[k]), k
    assert np.array_equal(_bits(got["path_cost"]), _bits(near["path_cost"]))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got["sub_goals"], near["sub_goals"]))
    assert got["cells"] == near["cells"]
    return got


def test_w_gain_0_is_the_nearest_frontier_plan():
    shared, per = K.scanned_maps()
    rng = np.random.default_rng(3)
    starts = np.concatenate([np.array(K.SCAN_AT), K.points(rng, K.MAP_W, K.MAP_H, 9, K.MAP_ORIGIN, K.MAP_CELL, margin=1.0)])
    got = _identity(shared, starts, K.MAP_ORIGIN, K.MAP_CELL, 2, 2, S_max=96)
    assert (got["status"][:3] == G.FOUND).all()
    _identity(shared, starts, K.MAP_ORIGIN, K.MAP_CELL, 0, 1, max_seg=5, S_max=96)
    _identity(per, np.array(K.SCAN_AT), K.MAP_ORIGIN, K.MAP_CELL, 2, 2)
    every = list(K.centres([(i, j) for i in range(5) for j in range(7)])) + [(ORIGIN[0] - 0.01, 0.3), (0.0, np.inf)]
    for r, mu in ((0, 1), (0, 2), (2, 1)):
        _identity(HAND_MADE, every, ORIGIN, CELL, r, mu)


def _cost_from(src, field):
    """Brute force: the plain 5 / 7 cost from every passable cell to the one cell ``src``."""
    one = np.zeros(field.shape, np.uint8)
    one[src] = 1
    return G.ufield(one, field, np.zeros(field.shape, np.int32), 0, 1, 0)[0]


@pytest.mark.parametrize("seed,w_gain,g_cap,min_gain", [(1, 16, 12, 0), (2, 200, 9, 0), (3, 65535, 16384, 0), (4, 40, 12, 3), (5, 7, 6, 1)])
def test_speckled_maps_hold_the_field_equation(seed, w_gain, g_cap, min_gain):
    rng = np.random.default_rng(seed)
    W, H = 12, 14
    ev = K.speckled(rng, W, H, p_free=0.8, p_solid=0.05)
    start = K.points(rng, W, H, 24, margin=0.3)
    want = G.plan_batch(ev, T_FREE, T_OCC, ORIGIN, CELL, start, 3, w_gain, g_cap, min_gain, 0, 1)
    fr, fld, gain, uf = want["frontier"][0], want["field"][0], want["gain"][0], want["ufield"][0]
    src = G.sources(fr, fld, gain, min_gain)
    assert want["n_sources"][0] == src.sum() >= 3 and (want["status"] == G.FOUND).sum() >= 8
    seeds = {(int(i), int(j)): G.seed(gain[i, j], w_gain, g_cap) for i, j in zip(*np.nonzero(src))}
    costs = {c: _cost_from(c, fld) for c in seeds}
    # the field is the least seeded cost, cell by cell
    least = np.full((W, H), int(FO.INF), np.int64)
    for c, sd in seeds.items():
        least = np.minimum(least, np.where(costs[c] == FO.INF, int(FO.INF), costs[c].astype(np.int64) + sd))
    assert np.array_equal(uf.astype(np.int64), least)
    for b in np.nonzero(want["status"] == G.FOUND)[0]:
        s, path = want["cells"][b][0], want["cells"][b]
        t = path[-1]
        assert t in seeds and int(uf[t]) == seeds[t]                                  # a source that nothing dominates
        assert int(uf[s]) - seeds[t] == round(5 * want["path_cost"][b]) and 5 * want["path_cost"][b] == int(uf[s]) - seeds[t]
        assert all(int(uf[s]) <= sd + int(costs[c][s]) for c, sd in seeds.items() if costs[c][s] != FO.INF)
        assert want["target_gain"][b] == gain[t] >= min_gain and want["target_cell"][b] == t[0] * H + t[1]
        assert not any(G.terminal(c, fr, gain, uf, w_gain, g_cap, min_gain) for c in path[:-1])      # the FIRST terminal cell
        walked = sum(7 if a[0] != c[0] and a[1] != c[1] else 5 for a, c in zip(path, path[1:]))
        assert walked == int(uf[s]) - int(uf[t])


def _corridor(gain_a, start_cells):
    ev, gain = K.corridor(gain_a)
    kw = dict(K.CORRIDOR_KW)
    return K.expected(ev, K.centres(start_cells), kw["r_view"], kw["w_gain"], kw["g_cap"], kw["min_gain"], kw["r"], kw["mu"], gain=gain)


def test_a_source_whose_seed_ties_the_route_through_it_is_where_the_descent_stops():
    A, B = K.CORRIDOR_A, K.CORRIDOR_B
    want = _corridor(75, [(1, 0), A, (1, 4), (1, 5), (1, 11)])
    uf = want["ufield"][0]
    assert want["n_sources"][0] == 2 and want["n_frontier"][0] == 6
    assert uf[B] == 0 and uf[A] == 25 == uf[1, 4] + 5 == G.seed(75, 16, 100)          # the tie
    assert want["target_cell"].tolist() == [A[0] * 12 + A[1]] * 2 + [B[0] * 12 + B[1]] * 3
    assert want["target_gain"].tolist() == [75, 75, 100, 100, 100] and want["n_sub"].tolist() == [1] * 5
    assert want["path_cost"].tolist() == [3.0, 0.0, 4.0, 3.0, 3.0]                      # the walk's length, not the field's value
    better = _corridor(76, [(1, 0), (1, 4)])                  # strictly better: A holds its own seed, 24
    assert better["ufield"][0][A] == 24 and better["target_cell"].tolist() == [A[0] * 12 + A[1], B[0] * 12 + B[1]]


def test_a_dominated_source_is_nobodys_target():
    A, B = K.CORRIDOR_A, K.CORRIDOR_B
    want = _corridor(74, [(1, j) for j in range(12)])
    uf = want["ufield"][0]
    assert want["n_sources"][0] == 2 and uf[A] == 25 < G.seed(74, 16, 100)
    assert (want["status"] == G.FOUND).all() and (want["target_cell"] == B[0] * 12 + B[1]).all() and (want["target_gain"] == 100).all()
    assert want["n_sub"][A[1]] == 1 and want["path_cost"][A[1]] == 5.0                  # a robot ON the dominated source walks on


def test_min_gain_above_every_gain_leaves_no_source():
    shared, _ = K.scanned_maps()
    want = G.plan_batch(shared, T_FREE, T_OCC, K.MAP_ORIGIN, K.MAP_CELL, SIX_STARTS, 10, 16, 174, 175)
    assert want["n_sources"].tolist() == [0] and want["n_frontier"][0] == 153 and (want["ufield"] == FO.INF).all()
    assert (want["status"] == G.NO_PATH).all() and (want["target_gain"] == -1).all() and (want["target_cell"] == -1).all()
    assert (want["nearest"]["status"] == G.FOUND).all()
    some = G.plan_batch(shared, T_FREE, T_OCC, K.MAP_ORIGIN, K.MAP_CELL, SIX_STARTS, 10, 16, 174, 100)
    assert 0 < some["n_sources"][0] < 153 and (some["target_gain"] >= 100).all()


def test_informed_targets_differ_from_the_nearest_ones_on_the_scanned_map():
    """r_view 10, g_cap the largest gain, w_gain 16 (one cost unit per cell not revealed): every one of the six starts gets another
    target than its nearest frontier cell, one that reveals more."""
    shared, _ = K.scanned_maps()
    g_cap = int(G.gain(shared, T_FREE, T_OCC, FR.field(shared, T_FREE, T_OCC, 2, 2)[1], 10).max())
    want = G.plan_batch(shared, T_FREE, T_OCC, K.MAP_ORIGIN, K.MAP_CELL, SIX_STARTS, 10, 16, g_cap)
    near = want["nearest"]
    assert (want["status"] == G.FOUND).all() and (near["status"] == G.FOUND).all()
    assert (want["target_cell"] != near["target_cell"]).all()
    assert (want["target_gain"] > want["gain"][0].reshape(-1)[near["target_cell"]]).all()


def test_the_lds_switch_is_this_kernels_own():
    (W, H), (W1, _) = G.sizes_at_the_lds_switch()
    assert G.field_fits_lds(W * H) and not G.field_fits_lds(W1 * H)
    assert 4 * (FO.bitmap_words(W * H) + 2 + W * H) + 256 <= 160 * 1024 < 4 * (FO.bitmap_words(W1 * H) + 2 + W1 * H) + 256
    assert (W, H) != FR.sizes_at_the_lds_switch()[0]           # (one bitmap, not three)


def test_the_recorded_chains_hold_the_bar_the_device_is_held_to():
    """tests/test_gain_fleet_gpu.py allows one seed below min - (max - min) of the CPU chain's coverage: the chains themselves must
    satisfy that cap; and the finishing sample is asserted nowhere unless every seed beats the nearest rule by more than the spread."""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exploration_informed.npz"))
    assert len(d["field/seeds"]) == 6 and len(d["rooms/seeds"]) == 6 and len(d["field/starts"]) == 4 and int(d["min_gain"]) > 0
    assert len(d["single/starts"]) == 1 and len(d["own_maps/starts"]) == 4
    for scene in ("field", "rooms"):
        for rule in ("informed", "pruned"):
            cpu = d[f"{scene}/{rule}/coverage"]
            assert (cpu < cpu.min() - (cpu.max() - cpu.min())).sum() <= 1
            assert not bool(d[f"{scene}/{rule}/sooner_every_seed"])
    assert not d["field/nearest/finished"].all()               # the sliver that keeps the nearest-frontier fleet walking until k_max
