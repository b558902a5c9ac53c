"""CPU: the inputs of the large-map tests (tests/large_map_cases.py) reach what they claim, shown on the oracles alone
(tests/grid_lidar_oracle.py, tests/map_oracle.py, tests/frontier_oracle.py, tests/gain_oracle.py, tests/assign_oracle.py) -- so that
a GPU test that passes has run the scan, the update and the tiled planners above 2^17 cells, over the grid's edges and across the
tile borders it is about.  Every number asserted here comes from an oracle, none from the device."""
import numpy as np
import pytest

import field_tiled_cases as T
import frontier_oracle as FR
import grid_lidar_oracle as G
import large_map_cases as LC
import lidar_oracle as L
import map_oracle as M

TW, TH = LC.TW, LC.TH


def test_shapes_are_derived_from_the_tile_and_lie_between_the_caps():
    want = {"first_refused": (363, 362), "long_j": (TW + 1, LC.SIDE_CAP), "long_i": (LC.SIDE_CAP, TW + 1)}
    for id_, (W, H) in want.items():
        s = LC.shape(id_)
        assert (s["W"], s["H"]) == (W, H) == s["occ"].shape
        assert W * H > LC.OLD_CAP and max(W, H) <= LC.SIDE_CAP and W * H <= LC.MAX_CELLS
    assert (TW + 1) * LC.SIDE_CAP > LC.OLD_CAP >= TW * LC.SIDE_CAP         # one row fewer and the old calls would take the long maps
    assert LC.tiles(LC.shape("long_j")) == (2, LC.SIDE_CAP // TH) and LC.tiles(LC.shape("long_i")) == (LC.SIDE_CAP // TW, 1)
    assert LC.shape("first_refused")["origin"] == LC.ORIGIN and LC.shape("long_j")["cell"] == LC.CELL
    assert LC.shape("long_i")["cell"] == LC.CELL[::-1] and LC.shape("long_i")["origin"] == LC.ORIGIN[::-1]


@pytest.mark.parametrize("id_", LC.LONG_IDS)
def test_every_window_is_wider_than_a_long_map(id_):
    """35 cells along the short axis against TW + 1: no in-grid station has a window row that lies inside the grid from end to
    end, for the scan and for the update alike."""
    s = LC.shape(id_)
    short = 0 if s["W"] < s["H"] else 1
    for half in (LC.scan_half(s), LC.map_half(s)):
        assert 2 * half[short] + 1 > (s["W"], s["H"])[short] and 2 * half[1 - short] + 1 < (s["W"], s["H"])[1 - short]
    for n in LC.IN_GRID:
        c = G.robot_cell(s["stations"][n], s["origin"], s["cell"])
        assert 0 <= c[0] < s["W"] and 0 <= c[1] < s["H"], n
        lo, hi = c[short] - LC.scan_half(s)[short], c[short] + LC.scan_half(s)[short]
        assert lo < 0 or hi >= (s["W"], s["H"])[short], n


@pytest.mark.parametrize("id_", LC.IDS)
def test_the_true_map_has_its_blocks(id_):
    s = LC.shape(id_)
    occ, (ci, cj), W, H = s["occ"], s["anchor"], s["W"], s["H"]
    assert occ[W - 1, H - 1] and occ[W - 1, :].any() and occ[:, H - 1].any()
    block = np.argwhere(occ[ci - 1:ci + 1, cj - 1:cj + 1] != 0) + (ci - 1, cj - 1)
    assert len(block) == 4 and len({T.tile_of(tuple(c)) for c in block}) == min(4, 2 * LC.tiles(s)[1])       # straddles the corner / the border
    assert ci % TW == 0 and (cj % TH == 0 or LC.tiles(s)[1] == 1)
    origin_block = np.argwhere(occ[:12, :12] != 0)
    assert len(origin_block) and np.abs((origin_block + 0.5) * s["cell"]).max() < LC.RANGE


@pytest.mark.parametrize("id_", LC.IDS)
def test_stations_reach_the_edges_the_corner_and_the_large_indices(id_):
    s = LC.shape(id_)
    W, H, occ = s["W"], s["H"], s["occ"]
    pos, table = LC.positions(s), L.ray_table(LC.RESOLUTION)
    scan = LC.scan_oracle(id_)
    n_hits = {n: int(scan[b][1].sum()) for b, n in enumerate(LC.STATIONS)}
    nx, ny = LC.scan_half(s)
    mx, my = LC.map_half(s)
    cells = {n: G.robot_cell(s["stations"][n], s["origin"], s["cell"]) for n in LC.STATIONS}
    # the two corner windows each lose cells over two edges, for the scan and for the update
    for hx, hy in ((nx, ny), (mx, my)):
        assert cells["origin"][0] - hx < 0 and cells["origin"][1] - hy < 0
        assert cells["far_corner"][0] + hx >= W and cells["far_corner"][1] + hy >= H
    # the far corner: readings, and an update that writes beyond flat index 2^17
    hits = LC.oracle_hits(id_)
    delta = M.robot_delta(pos[LC.index("far_corner")], hits[LC.index("far_corner")], W, H, s["origin"], s["cell"], LC.RANGE, table,
                          M.default_depth(s["cell"]), LC.W_HIT, LC.W_MISS)[0]
    flat = np.nonzero(delta.ravel())[0]
    assert n_hits["far_corner"] > 0 and flat.max() > LC.OLD_CAP and (delta > 0).any() and (delta < 0).any()
    assert delta[W - 1].any() and delta[:, H - 1].any()                   # the last row and the last column themselves
    # the solid-cell station, the outside station, the far one
    assert G.in_solid_cell(s["stations"]["solid"], occ, s["origin"], s["cell"]) and n_hits["solid"] == 0
    assert sum(G.in_solid_cell(p, occ, s["origin"], s["cell"]) for p in pos) == 1
    c = cells["outside"]
    assert not (0 <= c[0] < W and 0 <= c[1] < H) and n_hits["outside"] > 0
    ev = np.zeros((W, H), np.int64)
    LC.update(s, ev, pos[LC.index("far"):LC.index("far") + 1], hits[LC.index("far"):LC.index("far") + 1])
    assert n_hits["far"] == 0 and not ev.any()
    # the corner and border stations see the anchor block; the border station stands ON the tile border (a first crossing at t = 0)
    assert n_hits["corner"] > 0 and n_hits["border"] > 0 and n_hits["origin"] > 0
    bi = cells["border"][0]
    assert bi % TW == 0 and 0 < bi < W and s["stations"]["border"][0] == s["origin"][0] + bi * s["cell"][0]
    counts = G.grid_hits(s["stations"]["border"], occ, s["origin"], s["cell"], LC.RANGE, table, counts=True)[2]
    assert counts["t0"] > 0
    # per-robot maps: every in-grid station's own map differs from the shared one within its window, and its scan with it
    per, shared = LC.scan_oracle(id_, True), LC.scan_oracle(id_)
    stack = LC.per_robot_occ(s)
    differ = [n for b, n in enumerate(LC.STATIONS) if not np.array_equal(per[b][1], shared[b][1]) or not np.array_equal(per[b][0], shared[b][0])]
    assert len(differ) >= 3 and all((stack[b] != occ).sum() <= 4 for b in range(len(pos))), differ
    print(f"{id_}: {W} x {H} = {W * H} cells, tiles {LC.tiles(s)}, scan window {2 * nx + 1} x {2 * ny + 1}, readings {n_hits}, "
          f"largest flat index updated {int(flat.max())}, per-robot scans that differ {differ}")


@pytest.mark.parametrize("id_", LC.IDS)
def test_the_hand_made_readings_have_nan_rows_and_the_mask_skips_two(id_):
    s = LC.shape(id_)
    hits = LC.hand_made_hits(s)
    nan_rows = np.isnan(hits).all(2).sum(1)
    assert (nan_rows > 200).all() and np.isnan(hits).any(2).sum() > nan_rows.sum() and np.isinf(hits).any()
    assert LC.mask().tolist().count(0) == 2 and LC.mask().sum() == len(LC.STATIONS) - 2
    ev = LC.update(s, np.zeros((s["W"], s["H"]), np.int64), LC.positions(s), hits)
    assert (ev > 0).sum() > 100 and (ev < 0).sum() > 500 and np.nonzero(ev.ravel())[0].max() > LC.OLD_CAP


@pytest.mark.parametrize("id_", LC.IDS)
def test_the_sample_plans_cross_tiles(id_):
    """After the preset and one noise-free scan of every station: frontier cells in four tiles or more, a FOUND plan into another
    tile, on the long maps a descent along the whole long side; two claims or more; informed targets of different gains."""
    s = LC.shape(id_)
    ev, pos = LC.sample_evidence(id_), LC.positions(s)
    near = LC.plan_oracle(id_, "frontier")
    i0, i1, j0, j1 = s["box"]
    assert ((ev != 0).sum() > (i1 - i0) * (j1 - j0) > 10000) and (LC.preset(s) == 0).sum() > s["W"] * s["H"] // 2
    frontier_tiles = {LC.tile_of_flat(s, int(f)) for f in np.nonzero(near["frontier"][0].ravel())[0]}
    assert len(frontier_tiles) >= 4, frontier_tiles
    found = [b for b in range(len(pos)) if near["status"][b] == FR.FOUND]
    crossing = [b for b in found if T.tile_of(near["cells"][b][0]) != LC.tile_of_flat(s, int(near["target_cell"][b]))]
    assert crossing, near["status"]
    assert near["status"][LC.index("outside")] == FR.OUTSIDE_GRID and near["status"][LC.index("far")] == FR.OUTSIDE_GRID
    assert near["status"][LC.index("solid")] == FR.START_OCCUPIED
    changes = {LC.STATIONS[b]: T.tile_changes(near["cells"][b]) for b in found}
    if id_ in LC.LONG_IDS:
        along = max(LC.tiles(s))
        assert changes["corner"] >= along - 2 and changes["border"] >= along - 2, changes
        fld_changes = T.descent_changes(near["field"][0])
        assert fld_changes[near["cells"][LC.index("corner")][0]] >= along - 2
        assert LC.budgets(id_, "frontier") >= along - 2
    claims = LC.plan_oracle(id_, "claims")
    assert claims["n_claims"] >= 2 and len(set(claims["targets"])) == claims["n_claims"]
    informed = LC.plan_oracle(id_, "informed")
    gains = {int(g) for g in informed["target_gain"] if g >= 0}
    assert informed["n_sources"][0] > 0 and len(gains) >= 2, gains
    print(f"{id_}: {int((ev != 0).sum())} known cells, {int(near['n_frontier'][0])} frontier cells in {len(frontier_tiles)} tiles, "
          f"FOUND {[LC.STATIONS[b] for b in found]}, into another tile {[LC.STATIONS[b] for b in crossing]}, tile changes {changes}, "
          f"{claims['n_claims']} claims by {[LC.STATIONS[b] for b in claims['winners']]}, {int(informed['n_sources'][0])} sources, "
          f"target gains {sorted(gains)}, budgets of rounds {[LC.budgets(id_, k) for k in ('frontier', 'informed', 'claims')]}")


def test_the_per_robot_sample_on_363_x_362_differs_from_map_to_map():
    s = LC.shape("first_refused")
    ev = LC.per_robot_sample_evidence("first_refused")
    assert ev.shape == (len(LC.STATIONS), s["W"], s["H"]) and len({e.tobytes() for e in ev}) >= 5
    near = LC.per_robot_plan_oracle("frontier")
    assert (near["status"] == FR.FOUND).sum() >= 4 and len(set(near["n_frontier"].tolist())) >= 3


def test_the_runners_are_four_free_stations_round_the_corner_and_in_the_corners():
    s = LC.shape("first_refused")
    pos = LC.positions(s, LC.RUNNERS)
    assert len(pos) == 4 and not any(G.in_solid_cell(p, s["occ"], s["origin"], s["cell"]) for p in pos)
    ci, cj = s["anchor"]
    for n in LC.RUNNERS[:2]:
        c = G.robot_cell(s["stations"][n], s["origin"], s["cell"])
        assert max(abs(c[0] - ci), abs(c[1] - cj)) <= 5
    i0, i1, j0, j1 = s["box"]
    assert (i1 - i0) >= 3 * TW and (j1 - j0) >= 3 * TH and i0 < ci < i1 and j0 < cj < j1
    assert LC.noise(s, 12, LC.RUNNERS).shape == (12, 4, LC.RESOLUTION, 2)


def test_only_the_corner_cell_s_fall_wakes_the_diagonal_tile():
    """tests/large_map_cases.py's corner_wake: D's value comes through the diagonal from C, C's own arrives a round after A's and
    B's, and neither A nor B can fall when it does."""
    c, want = LC.corner_wake(), LC.corner_wake_oracle()
    fld = want["field"][0]
    A, B, C, D = (c["cells"][k] for k in "ABCD")
    assert {T.tile_of(x) for x in (A, B, C, D)} == {(0, 1), (1, 0), (1, 1), (0, 0)}
    v = int(fld[C])
    assert int(fld[D]) == v + 7 < min(int(fld[A]), int(fld[B])) + 5 and T.descent_step(fld, D) == C
    assert v + 3 <= int(fld[A]) <= v + 5 and v + 3 <= int(fld[B]) <= v + 5          # C's fall improves D, and neither A nor B
    changes = T.descent_changes(fld)
    assert changes[A] == 0 and changes[B] == 0 and changes[C] == 1 and changes[D] == 2
    free = np.argwhere(fld != FR.INF)
    assert [tuple(x) for x in free if T.tile_of(tuple(x)) == (0, 0)] == [D]     # nothing else in D's tile can wake it
    assert want["status"].tolist() == [FR.FOUND] * 4 and want["n_frontier"].tolist() == [3]
    print("corner_wake: A, B, C, D =", [int(fld[x]) for x in (A, B, C, D)], "tile changes", [int(changes[x]) for x in (A, B, C, D)])


@pytest.mark.parametrize("id_", LC.IDS)
def test_a_reading_beside_a_block_turns_a_free_cell_unknown_again(id_):
    """The update rule, on the oracle: a reading on a block's face near its corner is pushed past the corner into a free cell, which
    gains w_hit and leaves the free class.  So the count of known-free cells of ONE robot's map may fall from scan to scan (the
    run test holds only the shared map and the fleet's total to "does not fall"), and the planners are given min_unknown = 3, at
    which such a lone cell makes no frontier."""
    s = LC.shape(id_)
    before, after = LC.preset(s), LC.sample_evidence(id_)
    i0, i1, j0, j1 = s["box"]
    lost = (before[i0:i1, j0:j1] <= -LC.T_FREE) & (after[i0:i1, j0:j1] > -LC.T_FREE)
    assert 1 <= lost.sum() <= 4 and LC.MIN_UNKNOWN == 3
    assert (s["occ"][i0:i1, j0:j1][lost] == 0).all()
