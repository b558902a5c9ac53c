"""What the tests of claim hysteresis share (tests/test_assign_keep_gpu.py, tests/test_assign_keep_oracle.py): tests/assign_checks.py's
maps and comparison, with a previous target per robot, the three keep parameters and the two new outputs.  The oracle side needs no
GPU; torch and the library are imported by the functions that run the device."""
import numpy as np

import assign_checks as AC
import assign_keep_oracle as K
import frontier_oracle as FR
from assign_checks import CELL, ORIGIN, POISON_I32, T_FREE, T_OCC

POISON_I8 = 55
GENEROUS = (0, 1024, 4096)                                    # (r_keep, keep_ratio16, keep_slack): the target itself, at any cost


def index(c, H):
    return c[0] * H + c[1]


def nearest(ev, start, r=2, mu=2, max_seg=None, S_max=64):
    return FR.plan_batch(ev, T_FREE, T_OCC, ORIGIN, CELL, np.asarray(start, np.float64).reshape(-1, 2), r, mu, max_seg, S_max)


def expected(ev, start, r_claim, max_claims, prev, keep, r=2, mu=2, max_seg=None, S_max=64, may_claim=None, near=None):
    start = np.asarray(start, np.float64).reshape(-1, 2)
    near = nearest(ev, start, r, mu, max_seg, S_max) if near is None else near
    return K.plan_batch(ev, T_FREE, T_OCC, ORIGIN, CELL, start, r_claim, prev, *keep, max_claims, r, mu, max_seg, S_max, may_claim, nearest=near)


def buffers(B, W, H, S_max):
    import torch
    out = AC.buffers(B, W, H, S_max)
    out["kept"] = torch.full((B,), POISON_I8, dtype=torch.int8, device="cuda")
    out["n_kept"] = torch.full((1,), POISON_I32, dtype=torch.int32, device="cuda")
    return out


def planner(r_claim, max_claims, keep, r=2, mu=2, max_seg=None):
    import lipmpc
    return lipmpc.CoordinatedFrontierPlanner(r_claim, max_claims, r_keep=keep[0], keep_ratio16=keep[1], keep_slack=keep[2], r_inflate=r,
                                             min_unknown=mu, t_free=T_FREE, t_occ=T_OCC, max_seg=max_seg)


def run(ev, start, r_claim, max_claims, prev, keep, r=2, mu=2, max_seg=None, S_max=64, may_claim=None):
    import torch
    ev, start = np.ascontiguousarray(ev, np.int32), np.ascontiguousarray(np.asarray(start, np.float64).reshape(-1, 2))
    W, H = ev.shape
    out = buffers(len(start), W, H, S_max)
    pl = planner(r_claim, max_claims, keep, r, mu, max_seg)
    may = None if may_claim is None else torch.as_tensor(np.asarray(may_claim), device="cuda")
    prev = None if prev is None else torch.as_tensor(np.asarray(prev, np.int32), device="cuda")
    got = pl.replan(torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda"), origin=ORIGIN, cell=CELL, S_max=S_max, out=out,
                    may_claim=may, prev_target=prev)
    torch.cuda.synchronize()
    assert got is out and pl.last is out
    return AC.host(out)


def same(got, want, S_max):
    """tests/assign_checks.py's comparison of every output, then kept and n_kept."""
    AC.same(got, want, S_max)
    assert np.array_equal(got["kept"], want["kept"]), (got["kept"][:16], want["kept"][:16])
    assert got["n_kept"].tolist() == [want["n_kept"]]


def check(ev, start, r_claim, max_claims, prev, keep, r=2, mu=2, max_seg=None, S_max=64, may_claim=None, want=None):
    if want is None:
        want = expected(ev, start, r_claim, max_claims, prev, keep, r, mu, max_seg, S_max, may_claim)
    got = run(ev, start, r_claim, max_claims, prev, keep, r, mu, max_seg, S_max, may_claim)
    same(got, want, S_max)
    return got, want


def spaced(want, r_claim):
    """The targets of any two winners, kept or claimed, are more than r_claim apart."""
    t = np.array(want["targets"]).reshape(-1, 2)
    d2 = ((t[:, None] - t[None]) ** 2).sum(2)[np.triu_indices(len(t), 1)]
    return bool((d2 > r_claim * r_claim).all())
