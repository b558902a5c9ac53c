"""What the GPU tests of the coordinated claim share (tests/test_assign_gpu.py): the maps, one run of CoordinatedFrontierPlanner into
poisoned buffers, and the comparison of EVERY output with tests/assign_oracle.py, bit for bit.  The maps and the oracle side need no
GPU (tests/test_assign_oracle.py uses them too); torch and the library are imported by the functions that run the device."""
import numpy as np

import assign_oracle as A
import field_oracle as FO
import frontier_oracle as FR

SENTINEL = -7.25
ORIGIN, CELL = (-0.35, 0.2), (0.1, 0.125)                     # tests/grid_checks.py's placement (anisotropic cells)
T_FREE, T_OCC = 1, 3
POISON_I32, POISON_WORK = 77, 0x5EEDBEEF


def centres(cells, origin=ORIGIN, cell=CELL):
    return np.array([FO.centre(c, origin, cell) for c in cells]).reshape(-1, 2)


def open_field(W, H, margin=2):
    """Everything unknown but a free rectangle ``margin`` cells inside the grid: its rim is ONE ring of frontier cells."""
    ev = np.zeros((W, H), np.int32)
    ev[margin:W - margin, margin:H - margin] = -T_FREE
    return ev


def two_rooms(W=30, H=14):
    """Two free rooms that no passable cell connects (an unknown band between them), each with its own frontier ring."""
    ev = np.zeros((W, H), np.int32)
    ev[2:12, 2:H - 2] = -T_FREE
    ev[16:W - 2, 2:H - 2] = -T_FREE
    return ev


def block_in_field(W=24, H=24, at=(10, 10)):
    """An open field with one solid cell: with r_inflate = 2 the free cells round it are an inflation band to snap out of."""
    ev = open_field(W, H)
    ev[at] = T_OCC
    return ev


def expected(ev, start, r_claim, max_claims, r=2, mu=2, max_seg=None, S_max=64, may_claim=None, t=(T_FREE, T_OCC), origin=ORIGIN, cell=CELL):
    start = np.asarray(start, np.float64).reshape(-1, 2)
    near = FR.plan_batch(ev, t[0], t[1], origin, cell, start, r, mu, max_seg, S_max)
    return A.plan_batch(ev, t[0], t[1], origin, cell, start, r_claim, max_claims, r, mu, max_seg, S_max, may_claim, nearest=near)


def expected_rows(want, S_max):
    """sub_goals [B,S_max,2] as the device must leave a buffer that held the sentinel: the path call's rows, then the winners'."""
    B = len(want["status"])
    rows = np.full((B, S_max, 2), SENTINEL)
    for b in range(B):
        n = int(want["nearest"]["n_sub"][b])
        rows[b, :n] = want["nearest"]["sub_goals"][b][:n]
        if want["claim_round"][b] >= 0 and want["status"][b] == FR.FOUND:
            rows[b, :want["n_sub"][b]] = want["sub_goals"][b]
    return rows


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def buffers(B, W, H, S_max):
    """Every output poisoned: the sentinel in the sub-goal rows, patterns no call writes in the rest."""
    import torch
    import lipmpc
    out = {k: torch.empty(shape, dtype=dt, device="cuda") for k, (dt, shape, _) in lipmpc.planner.assign_outputs(B, W, H, S_max).items()}
    out["sub_goals"].fill_(SENTINEL)
    for k in ("path_cost", "target"):
        out[k].fill_(SENTINEL)
    for k in ("n_sub", "status", "target_cell", "claim_round", "n_claims", "n_frontier"):
        out[k].fill_(POISON_I32)
    out["frontier"].fill_(9)
    for k in ("field", "work"):
        out[k].view(torch.int32).fill_(POISON_WORK)
    return out


def host(out):
    import torch
    h = {k: v.cpu().numpy() for k, v in out.items() if k not in ("field", "work")}
    h["field"] = out["field"].view(torch.int32).cpu().numpy().view(np.uint32)
    return h


def planner(r_claim, max_claims, r=2, mu=2, max_seg=None, t=(T_FREE, T_OCC)):
    import lipmpc
    return lipmpc.CoordinatedFrontierPlanner(r_claim, max_claims, r_inflate=r, min_unknown=mu, t_free=t[0], t_occ=t[1], max_seg=max_seg)


def run(ev, start, r_claim, max_claims, r=2, mu=2, max_seg=None, S_max=64, may_claim=None, t=(T_FREE, T_OCC), origin=ORIGIN, cell=CELL):
    import torch
    ev, start = np.ascontiguousarray(ev, np.int32), np.ascontiguousarray(np.asarray(start, np.float64).reshape(-1, 2))
    W, H = ev.shape
    out = buffers(len(start), W, H, S_max)
    pl = planner(r_claim, max_claims, r, mu, max_seg, t)
    may = None if may_claim is None else torch.as_tensor(np.asarray(may_claim), device="cuda")
    got = pl.plan(torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda"), origin=origin, cell=cell, S_max=S_max, out=out,
                  may_claim=may)
    torch.cuda.synchronize()
    assert got is out and pl.last is out
    return host(out)


def same(got, want, S_max):
    """Every output of the device equals the oracle's, bit for bit -- the whole sub-goal buffer included: rows below n_sub, the path
    call's rows a shorter claim left behind, the sentinel in the rest."""
    assert int(got["n_claims"][0]) == want["n_claims"], (got["n_claims"], want["n_claims"], want["winners"])
    assert np.array_equal(got["claim_round"], want["claim_round"]), (got["claim_round"][:16], want["claim_round"][:16])
    for k in ("n_frontier", "frontier", "field", "status", "n_sub", "target_cell"):
        assert np.array_equal(got[k], want[k]), (k, np.nonzero(np.asarray(got[k]) != np.asarray(want[k]))[0][:8])
    assert np.array_equal(bits(got["path_cost"]), bits(want["path_cost"]))
    claimed = want["target_cell"] >= 0
    assert np.array_equal(bits(got["target"][claimed]), bits(want["target"][claimed])) and np.isnan(got["target"][~claimed]).all()
    rows = expected_rows(want, S_max)
    assert got["sub_goals"].shape == rows.shape
    bad = np.nonzero((bits(got["sub_goals"]) != bits(rows)).any((1, 2)))[0]
    assert len(bad) == 0, (bad[:8], want["claim_round"][bad[:8]])


def check(ev, start, r_claim, max_claims, r=2, mu=2, max_seg=None, S_max=64, may_claim=None, t=(T_FREE, T_OCC), origin=ORIGIN, cell=CELL,
          want=None):
    if want is None:
        want = expected(ev, start, r_claim, max_claims, r, mu, max_seg, S_max, may_claim, t, origin, cell)
    got = run(ev, start, r_claim, max_claims, r, mu, max_seg, S_max, may_claim, t, origin, cell)
    same(got, want, S_max)
    return got, want
