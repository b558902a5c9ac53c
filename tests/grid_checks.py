"""What the GPU tests of the grid field planner and of the frontier explorer share (tests/test_field_gpu.py,
tests/test_frontier_gpu.py, tests/test_field_shapes_gpu.py, tests/test_gpu_poison.py): output buffers with a sentinel in the
sub-goal rows, one run of either planner through its Python class, and the comparison of EVERY output with the oracle's
(tests/field_oracle.py, tests/frontier_oracle.py), bit for bit.  Imported by GPU tests only: it needs torch and the library."""
import numpy as np
import torch

import field_oracle as Fo
import frontier_oracle as FR
import lipmpc

SENTINEL = -7.25
ORIGIN, CELL = (-0.35, 0.2), (0.1, 0.125)                     # (anisotropic cells: the metric counts cells)
T_FREE, T_OCC = 1, 3                                          # a mapper's default weights


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def host(out):
    h = {k: v.cpu().numpy() for k, v in out.items() if k != "field"}
    h["field"] = out["field"].view(torch.int32).cpu().numpy().view(np.uint32)
    return h


def _buffers(table):
    out = {k: torch.empty(shape, dtype=dt, device="cuda") for k, (dt, shape, _) in table.items()}
    out["sub_goals"].fill_(SENTINEL)
    return out


def same_paths(got, want, S_max):
    """status, n_sub, the bits of path_cost and of sub_goals[:n_sub], the sentinel in the rows behind n_sub."""
    assert np.array_equal(got["status"], want["status"]), np.nonzero(got["status"] != want["status"])[0][:8]
    assert np.array_equal(got["n_sub"], want["n_sub"]), np.nonzero(got["n_sub"] != want["n_sub"])[0][:8]
    assert np.array_equal(bits(got["path_cost"]), bits(want["path_cost"]))             # (one NaN pattern: __builtin_nan = numpy's)
    for b, sub in enumerate(want["sub_goals"]):
        n = len(sub)
        assert np.array_equal(bits(got["sub_goals"][b, :n]), bits(sub)), b
        assert (got["sub_goals"][b, n:] == SENTINEL).all(), b
    assert got["sub_goals"].shape[1] == S_max


# -- the grid field planner ----------------------------------------------------------------------------------------------
def field_buffers(B, F, W, H, S_max):
    return _buffers(lipmpc.planner.field_plan_outputs(B, F, W, H, S_max))


def run_field(occ, origin, cell, goal, start, r=0, max_seg=None, S_max=64):
    occ, goal, start = np.asarray(occ, np.uint8), np.asarray(goal, np.float64).reshape(-1, 2), np.asarray(start, np.float64).reshape(-1, 2)
    W, H = occ.shape[-2:]
    out = field_buffers(len(start), len(goal), W, H, S_max)
    pl = lipmpc.GridFieldPlanner(r_inflate=r, max_seg=max_seg)
    got = pl.plan_grid_batch(torch.as_tensor(goal, device="cuda"), lipmpc.GridMap(occ, origin, cell), torch.as_tensor(start, device="cuda"),
                             S_max=S_max, out=out)
    torch.cuda.synchronize()
    assert got is out and pl.last is out
    return host(out)


def same_field(got, want, S_max):
    """Every output of the device equals the oracle's, bit for bit; sub-goal rows from n_sub on still hold the sentinel."""
    assert np.array_equal(got["field_status"], want["field_status"]), (got["field_status"], want["field_status"])
    assert np.array_equal(got["field"], want["field"]), int((got["field"] != want["field"]).sum())
    same_paths(got, want, S_max)


def check_field(occ, origin, cell, goal, start, r=0, max_seg=None, S_max=64, want=None):
    """``want``: the oracle's plan_batch of these arguments where the caller has it already."""
    if want is None:
        want = Fo.plan_batch(occ, origin, cell, np.asarray(goal, np.float64).reshape(-1, 2), np.asarray(start, np.float64).reshape(-1, 2),
                             r, max_seg, S_max)
    got = run_field(occ, origin, cell, goal, start, r, max_seg, S_max)
    same_field(got, want, S_max)
    return got, want


# -- the frontier explorer -----------------------------------------------------------------------------------------------
def frontier_buffers(B, F, W, H, S_max):
    return _buffers(lipmpc.planner.frontier_outputs(B, F, W, H, S_max))


def frontier_planner(r, mu, max_seg, t=(T_FREE, T_OCC)):
    return lipmpc.FrontierPlanner(r_inflate=r, min_unknown=mu, t_free=t[0], t_occ=t[1], max_seg=max_seg)


def run_frontier(ev, start, r=2, mu=2, max_seg=None, S_max=64, t=(T_FREE, T_OCC), origin=ORIGIN, cell=CELL):
    ev, start = np.ascontiguousarray(ev, np.int32), np.ascontiguousarray(np.asarray(start, np.float64).reshape(-1, 2))     # (a reversed view has negative strides)
    W, H = ev.shape[-2:]
    out = frontier_buffers(len(start), 1 if ev.ndim == 2 else len(ev), W, H, S_max)
    pl = frontier_planner(r, mu, max_seg, t)
    got = pl.plan(torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda"), origin=origin, cell=cell, S_max=S_max, out=out)
    torch.cuda.synchronize()
    assert got is out and pl.last is out
    return host(out)


def same_frontier(got, want, S_max):
    """Every output of the device equals the oracle's, bit for bit; sub-goal rows from n_sub on still hold the sentinel."""
    assert np.array_equal(got["n_frontier"], want["n_frontier"]), (got["n_frontier"], want["n_frontier"])
    assert np.array_equal(got["frontier"], want["frontier"]), int((got["frontier"] != want["frontier"]).sum())
    assert np.array_equal(got["field"], want["field"]), int((got["field"] != want["field"]).sum())
    assert np.array_equal(got["target_cell"], want["target_cell"]), np.nonzero(got["target_cell"] != want["target_cell"])[0][:8]
    found = want["target_cell"] >= 0
    assert np.array_equal(bits(got["target"][found]), bits(want["target"][found])) and np.isnan(got["target"][~found]).all()
    same_paths(got, want, S_max)


def check_frontier(ev, start, r=2, mu=2, max_seg=None, S_max=64, t=(T_FREE, T_OCC), origin=ORIGIN, cell=CELL, want=None):
    if want is None:
        want = FR.plan_batch(ev, t[0], t[1], origin, cell, np.asarray(start, np.float64).reshape(-1, 2), r, mu, max_seg, S_max)
    got = run_frontier(ev, start, r, mu, max_seg, S_max, t, origin, cell)
    same_frontier(got, want, S_max)
    return got, want
