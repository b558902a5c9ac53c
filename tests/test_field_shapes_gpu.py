"""GPU: the grid field planner and the frontier explorer away from the shapes they were written at (tests/field_shape_cases.py;
tests/test_field_shapes_oracle.py shows on the CPU what each case reaches): the largest maps whose field stays in LDS and the
first ones over, rows longer than, equal to and just under the 1024 threads of the workgroup, strips 2 cells wide and 4096 long,
2^17 cells, r_inflate up to 16 with a disc row that needs both words of its window, 600 workgroups and 1000 robots in one call,
the longest one-cell corridor a map can hold, and fields that the kernel did not make.

Every comparison is tests/grid_checks.py's: field, field_status / n_frontier, frontier, status, n_sub, target_cell, the bits of
path_cost, target and sub_goals[:n_sub], the sentinel in the rows behind n_sub -- against tests/field_oracle.py and
tests/frontier_oracle.py, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import field_oracle as Fo
import field_shape_cases as S
import frontier_oracle as FR
from helpers import raw_call

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402
from grid_checks import SENTINEL, check_field, check_frontier, field_buffers, frontier_buffers, host, same_paths  # noqa: E402

ORIGIN, CELL = S.ORIGIN, S.CELL
SMALL = S.shape_cases() + S.inflation_cases() + S.window_cases()


def _check(c, planner):
    want = S.oracle(c["id"], planner)
    if planner == "field":
        return check_field(c["occ"], ORIGIN, CELL, c["goal"], c["start"], c["r"], c["max_seg"], c["S_max"], want=want)
    return check_frontier(c["ev"], c["start"], c["r"], S.MU, c["max_seg"], c["S_max"], want=want)


@pytest.mark.parametrize("planner", ["field", "frontier"])
@pytest.mark.parametrize("case", SMALL, ids=S.case_ids(SMALL))
def test_shapes_and_inflation(case, planner):
    """Both planners on every boundary shape of either LDS rule, on H = 1023, 1024, 1025 and their transposes, on 2 x 4096 and
    4096 x 2, at r_inflate 3, 7, 11 and 16 on 64 x 96 and 40 x 67, and on the two maps of one solid cell whose disc row is a
    33-bit window."""
    W, H = case["shape"]
    rule, nbytes = (Fo.field_fits_lds, Fo.field_lds_bytes) if planner == "field" else (FR.field_fits_lds, FR.field_lds_bytes)
    print(f"{case['id']} {planner}: {W * H} cells, field in {'LDS, ' + str(nbytes(W * H)) + ' dynamic bytes' if rule(W * H) else 'global memory'}")
    got, want = _check(case, planner)
    assert (want["status"] == Fo.FOUND).sum() >= 8
    if "blocked" in case:
        assert got["field"][0][case["blocked"]] == Fo.INF and got["field"][0][case["free"]] != Fo.INF


@pytest.mark.parametrize("planner", ["field", "frontier"])
@pytest.mark.parametrize("case", S.cap_cases(), ids=S.case_ids(S.cap_cases()))
def test_caps(case, planner):
    """32 x 4096 and 4096 x 32: 2^17 cells and a side of 4096, the most the calls accept; relaxed in global memory."""
    assert case["shape"][0] * case["shape"][1] == Fo.MAX_CELLS and max(case["shape"]) == Fo.MAX_SIDE
    _check(case, planner)


def test_600_fields_in_one_call():
    """F = B = 600 maps of 13 x 11, one workgroup each: more workgroups than the device holds at once."""
    occ, _, goal, start = S.per_robot_maps()
    got, want = check_field(occ, ORIGIN, CELL, goal, start, r=1)
    assert (want["status"] == Fo.FOUND).sum() >= 200


def test_600_frontier_maps_in_one_call():
    _, ev, _, start = S.per_robot_maps()
    got, want = check_frontier(ev, start, r=1, mu=S.MU)
    assert (want["status"] == Fo.FOUND).sum() >= 200


def test_1000_robots_down_one_field():
    """The 48 x 36 fleet maps with 1000 starts, NaN, outside and solid ones among them: 16 blocks of lanes, the last one partial."""
    occ, goal, start = S.field_fleet_case(988)
    got, want = check_field(occ, ORIGIN, CELL, goal, start, r=2)
    assert len(start) == 1000 and (want["status"] == Fo.FOUND).sum() >= 500
    ev, start = S.frontier_fleet_case(988)
    got, want = check_frontier(ev, start, r=2, mu=S.MU)
    assert len(start) == 1000 and (want["status"] == Fo.FOUND).sum() >= 400


@pytest.mark.parametrize("W,H", [(199, 199), (200, 199)])
def test_serpentine_corridor(W, H):
    """THE WORST CASE OF CHAOTIC RELAXATION: one corridor of 19 601 cells through the whole map, a value per cell to carry from one
    end to the other.  199 x 199 is relaxed in LDS, 200 x 199 in global memory.  The field call alone is timed with device events
    after a warm-up and the time printed; nothing is asserted about it."""
    occ, cells = S.serpentine(W, H)
    goal, start = np.array([S.centre(cells[0])]), np.array([S.centre(cells[-1]), S.centre(cells[len(cells) // 2])])
    got, want = check_field(occ, ORIGIN, CELL, goal, start, max_seg=250, S_max=1024)
    assert got["field"][0][cells[-1]] == 98000 and got["status"].tolist() == [Fo.FOUND, Fo.FOUND] and got["path_cost"][0] == 19600.0
    pl, grid = lipmpc.GridFieldPlanner(), lipmpc.GridMap(occ, ORIGIN, CELL).to("cuda")
    d_goal, out = torch.as_tensor(goal, device="cuda"), field_buffers(0, 1, W, H, 1)
    pl.field(d_goal, grid, out=out)                               # the warm-up
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    pl.field(d_goal, grid, out=out)
    t1.record()
    torch.cuda.synchronize()
    print(f"serpentine {W} x {H}, field in {'LDS' if Fo.field_fits_lds(W * H) else 'global memory'}: field call {t0.elapsed_time(t1):.2f} ms")
    assert np.array_equal(host(out)["field"], want["field"])


# -- fields the kernel did not make -------------------------------------------------------------------------------------------
def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _placement():
    org, cell = (C.c_double * 2)(*ORIGIN), (C.c_double * 2)(*CELL)
    return dict(origin=C.cast(org, C.c_void_p), cell=C.cast(cell, C.c_void_p)), (org, cell)


def _dev(a, dt):
    a = np.ascontiguousarray(a)
    return torch.as_tensor(a.view(np.int32) if a.dtype == np.uint32 else a, dtype=dt, device="cuda")     # (a field's words as int32)


def _prefilled(out):
    for k in ("n_sub", "status", "target_cell"):
        if k in out:
            out[k].fill_(-9)
    out["path_cost"].fill_(SENTINEL)
    return out


def _batch(plans, extra=()):
    keys = ("n_sub", "status") + tuple(extra)
    want = {k: np.array([p[k] for p in plans], np.int32) for k in keys}
    want.update(path_cost=np.array([p["path_cost"] for p in plans]), sub_goals=[p["sub_goals"] for p in plans])
    return want


def _field_fleet():
    occ, goal, start = S.field_fleet_case()
    fld, fs = Fo.field(occ, ORIGIN, CELL, goal[0], 2)
    path = Fo.plan(occ, ORIGIN, CELL, goal[0], start[3], 2, fld=fld, field_status=fs)["cells"]
    fields = dict(S.foreign_fields(fld, path), stale=fld)
    return occ, goal, start, fs, fields


@pytest.mark.parametrize("name", ["stale", "constant", "local_minimum", "raised"])
def test_path_call_on_a_field_it_was_not_given_by_the_field_call(name):
    """lipmpc_grid_path_batch on a `field` of the caller's own: map A's field beside map B's cells (a wall has moved: the field is
    walked as it stands, the start cell judged on B), a constant field, a field whose only minimum is 10, a valid field with one
    value of a path raised by 1.  The contract: where no neighbour satisfies the descent, NO_PATH, n_sub 0, path_cost NaN and no
    sub-goal row touched."""
    occ, goal, start, fs, fields = _field_fleet()
    occ_b = S.moved_wall(occ) if name == "stale" else occ
    fld, B, (W, H), S_max = fields[name], len(start), occ.shape, 64
    plans = [Fo.plan(occ_b, ORIGIN, CELL, goal[0], s, 2, None, S_max, fld=fld, field_status=fs, strict=False) for s in start]
    want = _batch(plans)
    if name != "stale":
        assert (want["status"] == Fo.NO_PATH).sum() >= (1 if name == "raised" else 90)
    if name == "raised":
        assert (want["status"] == Fo.FOUND).sum() >= 30                # the paths that miss the raised cell are found as before
    out = _prefilled(field_buffers(B, 1, W, H, S_max))
    place, keep = _placement()
    d = dict(occ=_dev(occ_b, torch.uint8), field=_dev(fld, torch.int32), field_status=_dev(np.array([fs], np.int32), torch.int32),
             goal=_dev(goal, torch.float64), start=_dev(start, torch.float64))
    rc = raw_call("lipmpc_grid_path_batch", device=0, B=B, F=1, W=W, H=H, grid_shared=1, r_inflate=2, max_seg=lipmpc.planner.FIELD_NO_CAP,
                  S_max=S_max, **place, **{k: _ptr(v) for k, v in d.items()},
                  **{k: _ptr(out[k]) for k in ("sub_goals", "n_sub", "status", "path_cost")},
                  hip_stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    same_paths({k: v.cpu().numpy() for k, v in out.items() if k not in ("field", "field_status")}, want, S_max)


@pytest.mark.parametrize("name", ["stale", "constant", "local_minimum", "raised"])
def test_frontier_path_call_on_a_field_it_was_not_given_by_the_field_call(name):
    """The same four fields under lipmpc_grid_frontier_path_batch: NO_PATH also leaves target_cell at -1."""
    ev, start = S.frontier_fleet_case()
    fld, _, n_front = FR.field(ev, S.T_FREE, S.T_OCC, 2, S.MU)
    path = FR.plan(ev, S.T_OCC, fld, n_front, ORIGIN, CELL, start[3], 2)["cells"]
    fld = dict(S.foreign_fields(fld, path), stale=fld)[name]
    ev_b = S.moved_wall(ev) if name == "stale" else ev
    B, (W, H), S_max = len(start), ev.shape, 64
    plans = [FR.plan(ev_b, S.T_OCC, fld, n_front, ORIGIN, CELL, s, 2, None, S_max, strict=False) for s in start]
    want = _batch(plans, ("target_cell",))
    if name != "stale":
        assert (want["status"] == Fo.NO_PATH).sum() >= (1 if name == "raised" else 80)
        assert (want["target_cell"][want["status"] == Fo.NO_PATH] == -1).all()
    out = _prefilled(frontier_buffers(B, 1, W, H, S_max))
    place, keep = _placement()
    d = dict(evidence=_dev(ev_b, torch.int32), field=_dev(fld, torch.int32), n_frontier=_dev(np.array([n_front], np.int32), torch.int32),
             start=_dev(start, torch.float64))
    rc = raw_call("lipmpc_grid_frontier_path_batch", device=0, B=B, F=1, W=W, H=H, t_occ=S.T_OCC, r_inflate=2,
                  max_seg=lipmpc.planner.FIELD_NO_CAP, S_max=S_max, **place, **{k: _ptr(v) for k, v in d.items()},
                  **{k: _ptr(out[k]) for k in ("sub_goals", "n_sub", "status", "path_cost", "target_cell")},
                  hip_stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    got = {k: out[k].cpu().numpy() for k in ("sub_goals", "n_sub", "status", "path_cost", "target_cell")}
    assert np.array_equal(got["target_cell"], want["target_cell"])
    same_paths(got, want, S_max)
