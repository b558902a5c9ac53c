"""CPU: the inputs of tests/test_field_shapes_gpu.py (tests/field_shape_cases.py) reach what they are meant to reach, shown on the
oracles alone: the boundary shapes sit on either side of the two LDS rules, every map leaves most of its cells reachable, most
starts find a path, one path is as long as the map, the inflation cases block more than the solid cells and make a start snap,
the serpentine corridor is as long as stated and the foreign fields end the way the contract says.  A device test on a map that
is blocked entirely, or on starts that all end early, would pass whatever the kernels did."""
import numpy as np
import pytest

import field_oracle as Fo
import field_shape_cases as S
import frontier_oracle as FR

CASES = S.all_cases()
NAMES = {Fo.FOUND: "FOUND", Fo.NO_PATH: "NO_PATH", Fo.START_OCCUPIED: "START_OCCUPIED", Fo.GOAL_OCCUPIED: "GOAL_OCCUPIED",
         Fo.PATH_OVERFLOW: "PATH_OVERFLOW", Fo.OUTSIDE_GRID: "OUTSIDE_GRID"}


def test_lds_boundary_shapes_follow_from_the_two_rules():
    """39 654 cells (18 x 2203) are the most whose field the field kernel keeps in LDS and 39 655 (35 x 1133 among others) the
    first count over with a shape inside the caps; 37 378 (22 x 1699) and 37 380 for the frontier kernel, 37 379 having no shape.
    At the boundary the dynamic LDS is 163 584 bytes: with the 256 bytes of slack exactly the 160 KiB of a workgroup."""
    (n, fits), (over, shapes) = Fo.lds_boundary(Fo.field_fits_lds)
    assert (n, over) == (39654, 39655) and set(fits) == {S.FIELD_FITS, S.FIELD_FITS[::-1]} and S.FIELD_OVER in shapes
    assert Fo.field_lds_bytes(n) == 163584 == Fo.LDS_LIMIT - Fo.LDS_SLACK
    (n, fits), (over, shapes) = Fo.lds_boundary(FR.field_fits_lds)
    assert (n, over) == (37378, 37380) and {S.FRONTIER_FITS, S.FRONTIER_FITS[::-1]} <= set(fits) and S.FRONTIER_OVER in shapes
    assert not Fo.shapes_of(37379) and FR.field_lds_bytes(n) == 163584
    for W, H, planner, fits in S.boundary_shapes():
        rule = Fo.field_fits_lds if planner == "field" else FR.field_fits_lds
        assert rule(W * H) == fits and W <= Fo.MAX_SIDE and H <= Fo.MAX_SIDE, (W, H, planner)
    assert FR.sizes_at_the_lds_switch() == ((193, 193), (194, 193))            # (the existing frontier test's pair, unchanged)
    for W, H in ((199, 199), (200, 199)):                                      # the existing field test's pair and the serpentine's
        assert Fo.field_fits_lds(W * H) == (W == 199)


def _figures(c, planner):
    """(finite share, statuses, longest path in cells, snapped count, blocked count, blocked count at r = 0) of a case."""
    W, H = c["shape"]
    o = S.oracle(c["id"], planner)
    cells = [Fo.cell_of(s, S.ORIGIN, S.CELL, W, H) for s in c["start"]]
    if planner == "field":
        blocked, blocked0 = Fo.blocked_cells(c["occ"], c["r"]), Fo.blocked_cells(c["occ"], 0)
        snapped = sum(1 for cell, s in zip(cells, o["snapped"]) if s is not None and s != cell)
    else:
        blocked, blocked0 = (FR.masks(c["ev"], S.T_FREE, S.T_OCC, r, S.MU)[0] for r in (c["r"], 0))
        snapped = sum(1 for cell, p in zip(cells, o["cells"]) if p and p[0] != cell)
        assert o["n_frontier"][0] > 0
    finite = float((o["field"][0] != Fo.INF).mean())
    cost = o["path_cost"][o["status"] == Fo.FOUND]
    return finite, o["status"], float(cost.max()) if len(cost) else 0.0, snapped, int(blocked.sum()), int(blocked0.sum())


@pytest.mark.parametrize("planner", ["field", "frontier"])
@pytest.mark.parametrize("case", CASES, ids=S.case_ids(CASES))
def test_case_is_not_vacuous(case, planner):
    """The field is finite on at least 60 % of the cells, at least half of the 16 starts end FOUND and one path is no shorter
    than the map's long side; an inflation case also makes a start snap and blocks more cells than r = 0 does."""
    finite, status, longest, snapped, blocked, blocked0 = _figures(case, planner)
    print(f"{case['id']} {planner}: r {case['r']}, finite {finite:.3f}, statuses {[NAMES[s] for s in status]}, "
          f"longest path {longest:.1f} cells, snapped {snapped}, blocked {blocked} (r = 0: {blocked0})")
    assert len(case["start"]) == 16 and finite >= 0.6
    assert (status == Fo.FOUND).sum() >= 8 and longest >= max(case["shape"])
    assert {Fo.START_OCCUPIED, Fo.OUTSIDE_GRID} <= set(status.tolist())
    if case["inflation"]:
        assert snapped >= 1 and blocked != blocked0


def test_window_cases_block_the_cell_33_bits_away():
    for c in S.window_cases():
        blocked = Fo.blocked_cells(c["occ"], 16)
        assert c["shape"][1] == 64 and blocked[c["blocked"]] and not blocked[c["free"]], c["id"]
        assert FR.masks(c["ev"], S.T_FREE, S.T_OCC, 16, S.MU)[0][c["blocked"]] and not FR.masks(c["ev"], S.T_FREE, S.T_OCC, 16, S.MU)[0][c["free"]]
    (i, j), = [tuple(x) for x in S.window_cases()[0]["solid"]]
    lo = j - 32
    assert (i, j) == (10, 63) and (i * 64 + lo) % 32 == 31                      # the row's window around (10, 47) starts at bit 31


def test_per_robot_maps_and_fleets_reach_every_status():
    occ, ev, goal, start = S.per_robot_maps()
    assert occ.shape == (600, 13, 11)
    o = Fo.plan_batch(occ, S.ORIGIN, S.CELL, goal, start, 1, None, 64)
    print("600 fields", np.bincount(o["status"], minlength=8).tolist(), "field status", np.bincount(o["field_status"], minlength=3).tolist())
    assert (o["status"] == Fo.FOUND).sum() >= 200 and all((o["field_status"] == k).sum() >= 20 for k in (0, 1, 2))
    o = FR.plan_batch(ev, S.T_FREE, S.T_OCC, S.ORIGIN, S.CELL, start, 1, S.MU, None, 64)
    print("600 frontier maps", np.bincount(o["status"], minlength=8).tolist(), "without a frontier", int((o["n_frontier"] == 0).sum()))
    assert (o["status"] == Fo.FOUND).sum() >= 200 and (o["n_frontier"] > 0).sum() >= 500
    occ, goal, start = S.field_fleet_case(988)
    assert len(start) == 1000
    o = Fo.plan_batch(occ, S.ORIGIN, S.CELL, goal, start, 2)
    st = np.bincount(o["status"], minlength=8)
    print("1000 starts", st.tolist())
    assert st[Fo.FOUND] >= 500 and st[Fo.OUTSIDE_GRID] >= 50 and st[Fo.START_OCCUPIED] >= 30 and st[Fo.NO_PATH] >= 20
    ev, start = S.frontier_fleet_case(988)
    o = FR.plan_batch(ev, S.T_FREE, S.T_OCC, S.ORIGIN, S.CELL, start, 2, S.MU)
    st = np.bincount(o["status"], minlength=8)
    print("1000 starts to the frontier", st.tolist())
    assert st[Fo.FOUND] >= 400 and st[Fo.OUTSIDE_GRID] >= 50 and st[Fo.START_OCCUPIED] >= 30 and st[Fo.NO_PATH] >= 20


@pytest.mark.parametrize("W,H", [(199, 199), (200, 199)])
def test_serpentine_is_one_corridor_of_19601_cells(W, H):
    occ, cells = S.serpentine(W, H)
    assert int((occ == 0).sum()) == len(cells) == len(set(cells)) == 19601
    fld, st = Fo.field(occ, S.ORIGIN, S.CELL, S.centre(cells[0]))
    assert st == Fo.FIELD_OK and fld[cells[-1]] == 98000 and all(int(fld[c]) == 5 * k for k, c in enumerate(cells))
    assert Fo.field_fits_lds(W * H) == (W == 199)


def test_foreign_fields_end_as_the_contract_says():
    """A constant field, a field whose only minimum is 10 and a field with one value of a path raised by 1 are no cost-to-go
    fields: the descent finds no neighbour, which the oracle reports as NO_PATH with ``strict=False`` and as an AssertionError
    without.  A stale field -- map A's, beside map B's cells -- is a cost-to-go field still: it is walked as it stands."""
    occ, goal, start = S.field_fleet_case()
    fld, fs = Fo.field(occ, S.ORIGIN, S.CELL, goal[0], 2)
    plan = lambda f, b, o=occ, **kw: Fo.plan(o, S.ORIGIN, S.CELL, goal[0], start[b], 2, fld=f, field_status=fs, **kw)
    good = plan(fld, 3)
    assert good["status"] == Fo.FOUND and len(good["cells"]) > 20
    for name, f in S.foreign_fields(fld, good["cells"]).items():
        with pytest.raises(AssertionError):
            plan(f, 3)
        p = plan(f, 3, strict=False)
        assert p["status"] == Fo.NO_PATH and p["n_sub"] == 0 and np.isnan(p["path_cost"]), name
    assert plan(fld, 3, strict=False)["status"] == Fo.FOUND                    # a valid field: the keyword changes nothing
    stale = [plan(fld, b, S.moved_wall(occ), strict=False) for b in range(len(start))]
    fresh = Fo.plan_batch(S.moved_wall(occ), S.ORIGIN, S.CELL, goal, start, 2)
    status = [p["status"] for p in stale]
    other = sum(1 for p, cells in zip(stale, fresh["cells"]) if p["status"] == Fo.FOUND and p["cells"] != cells)
    print("stale field", np.bincount(status, minlength=8).tolist(), "fresh field", np.bincount(fresh["status"], minlength=8).tolist(),
          "paths that differ", other)
    assert other >= 20 and status.count(Fo.FOUND) >= 60 and status.count(Fo.START_OCCUPIED) >= 4
