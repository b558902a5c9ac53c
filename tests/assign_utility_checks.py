"""What the tests of the gain-seeded claims share (tests/test_assign_utility_oracle.py, tests/test_assign_utility_gpu.py): the
cases, the consequences the header states, one run of CoordinatedFrontierPlanner with the gain keywords into poisoned buffers, and
the comparison of EVERY output with tests/assign_utility_oracle.py, bit for bit.  The cases and the oracle side need no GPU; torch
and the library are imported by the functions that run the device."""
import functools

import numpy as np

import assign_utility_oracle as AU
import frontier_oracle as FR
import gain_checks as K
import gain_oracle as G
from gain_checks import CELL, ORIGIN, POISON_I32, POISON_WORD, SENTINEL, T_FREE, T_OCC, bits

UWALL_STARTS = np.array([(1.6, 2.72), (1.65, 2.72), (1.6, 2.8), (2.6, 1.0), (2.65, 1.0), (4.3, 3.2)])
UWALL_SETS = ((10, 0, 100, 0), (10, 16, 120, 0), (15, 16, 120, 8), (30, 64, 600, 0))       # (r_view, w_gain, g_cap, min_gain)
UWALL_R_CLAIM = 15
CORRIDOR_STARTS = K.centres(((1, 0), (1, 1)))
CORRIDOR_R_CLAIM = 2


def cells_of(target_cell, H):
    return [(int(t) // H, int(t) % H) for t in target_cell]


def expected(ev, start, r_claim, r_view, w_gain, g_cap, min_gain=0, max_claims=64, r=2, mu=2, max_seg=None, S_max=64, may_claim=None,
             t=(T_FREE, T_OCC), origin=ORIGIN, cell=CELL, gain=None, informed=None):
    start = np.asarray(start, np.float64).reshape(-1, 2)
    return AU.plan_batch(ev, t[0], t[1], origin, cell, start, r_claim, r_view, w_gain, g_cap, min_gain, max_claims, r, mu, max_seg, S_max,
                         may_claim, gain=gain, informed=informed)


@functools.lru_cache(maxsize=None)
def uwall(r_view, w_gain, g_cap, min_gain, max_claims=64, S_max=64):
    """The scanned U-wall map of tests/gain_checks.py (92 x 80, shared evidence) with the six starts of the record."""
    ev, _ = K.scanned_maps()
    return expected(ev, UWALL_STARTS, UWALL_R_CLAIM, r_view, w_gain, g_cap, min_gain, max_claims, S_max=S_max, origin=K.MAP_ORIGIN,
                    cell=K.MAP_CELL)


def corridor(gain_a, max_claims=64):
    ev, gain = K.corridor(gain_a)
    kw = K.CORRIDOR_KW
    return ev, gain, expected(ev, CORRIDOR_STARTS, CORRIDOR_R_CLAIM, kw["r_view"], kw["w_gain"], kw["g_cap"], kw["min_gain"], max_claims,
                              kw["r"], kw["mu"], gain=gain)


def hence(want, r_claim, max_claims):
    """The consequences include/lipmpc.h states, on one result of the oracle (or of the device, with the oracle's records)."""
    inf = want["informed"]
    H = want["field"].shape[2]
    n = want["n_claims"]
    assert n == len(want["winners"]) <= max_claims and n == int((want["claim_round"] >= 0).sum())
    assert sorted(want["claim_round"][want["claim_round"] >= 0].tolist()) == list(range(n))
    assert all(a <= b for a, b in zip(want["costs"], want["costs"][1:])), want["costs"]
    tg = want["targets"]
    assert all((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 > r_claim ** 2 for k, a in enumerate(tg) for b in tg[k + 1:]), tg
    for b in range(len(want["status"])):
        k = int(want["claim_round"][b])
        if k <= 0:                                             # everyone else, and the round-0 winner: the utility path call's rows
            for key in ("status", "n_sub", "target_cell", "target_gain"):
                assert want[key][b] == inf[key][b], (key, b)
            assert np.array_equal(bits(want["path_cost"][b:b + 1]), bits(inf["path_cost"][b:b + 1])), b
            assert np.array_equal(bits(want["sub_goals"][b]), bits(inf["sub_goals"][b])), b
        if k >= 0:
            assert want["status"][b] in (FR.FOUND, FR.PATH_OVERFLOW) and want["target_cell"][b] == tg[k][0] * H + tg[k][1]
            assert want["target_gain"][b] == want["gain"][0][tg[k]]
    if max_claims == 0:
        assert n == 0


def expected_rows(want, S_max):
    """sub_goals [B,S_max,2] as the device must leave a buffer that held the sentinel: the utility path call's rows, then the winners'."""
    B = len(want["status"])
    rows = np.full((B, S_max, 2), SENTINEL)
    for b in range(B):
        n = int(want["informed"]["n_sub"][b])
        rows[b, :n] = want["informed"]["sub_goals"][b][:n]
        if want["claim_round"][b] >= 0 and want["status"][b] == FR.FOUND:
            rows[b, :want["n_sub"][b]] = want["sub_goals"][b]
    return rows


# -- the device --------------------------------------------------------------------------------------------------------------------
def buffers(B, W, H, S_max, table=None):
    """Every output poisoned: the sentinel in the sub-goal rows, patterns no call writes in the rest."""
    import torch
    import lipmpc
    table = lipmpc.planner.assign_utility_outputs(B, W, H, S_max) if table is None else table
    out = {k: torch.empty(shape, dtype=dt, device="cuda") for k, (dt, shape, _) in table.items()}
    poison(out)
    return out


def poison(out):
    import torch
    for k in ("sub_goals", "path_cost", "target"):
        out[k].fill_(SENTINEL)
    for k in ("n_sub", "status", "target_cell", "target_gain", "n_frontier", "n_sources", "gain", "claim_round", "n_claims"):
        out[k].fill_(POISON_I32)
    out["frontier"].fill_(9)
    for k in ("field", "ufield", "work"):
        if k in out:
            out[k].view(torch.int32).fill_(POISON_WORD)


def host(out):
    import torch
    words = ("field", "ufield", "work")
    h = {k: v.cpu().numpy() for k, v in out.items() if k not in words}
    for k in ("field", "ufield"):
        h[k] = out[k].view(torch.int32).cpu().numpy().view(np.uint32)
    return h


def planner(r_claim, r_view, w_gain, g_cap, min_gain=0, max_claims=64, r=2, mu=2, max_seg=None, t=(T_FREE, T_OCC), gain=None, cls=None, **kw):
    """The planner of a case.  ``gain``: a hand-written gain [W,H] that takes the place of the gain call's output."""
    import torch
    import lipmpc
    pl = (cls or lipmpc.CoordinatedFrontierPlanner)(r_claim, max_claims, r_view=r_view, w_gain=w_gain, g_cap=g_cap, min_gain=min_gain,
                                                    r_inflate=r, min_unknown=mu, t_free=t[0], t_occ=t[1], max_seg=max_seg, **kw)
    if gain is not None:
        given = torch.as_tensor(np.ascontiguousarray(gain, np.int32)[None], device="cuda")
        base = pl._informed or lipmpc.InformedFrontierPlanner
        pl._informed = type("GivenGain", (base,), {"_gain": lambda self, ev, t_free, t_occ, out: out["gain"].copy_(given)})
    return pl


def run(ev, start, r_claim, r_view, w_gain, g_cap, min_gain=0, max_claims=64, r=2, mu=2, max_seg=None, S_max=64, may_claim=None,
        t=(T_FREE, T_OCC), origin=ORIGIN, cell=CELL, gain=None):
    import torch
    ev, start = np.ascontiguousarray(ev, np.int32), np.ascontiguousarray(np.asarray(start, np.float64).reshape(-1, 2))
    W, H = ev.shape
    out = buffers(len(start), W, H, S_max)
    pl = planner(r_claim, r_view, w_gain, g_cap, min_gain, max_claims, r, mu, max_seg, t, gain)
    may = None if may_claim is None else torch.as_tensor(np.asarray(may_claim), device="cuda")
    got = pl.plan(torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda"), origin=origin, cell=cell, S_max=S_max, out=out,
                  may_claim=may)
    torch.cuda.synchronize()
    assert got is out and pl.last is out
    return host(out)


def same(got, want, S_max):
    """Every output of the device equals the oracle's, bit for bit -- the whole sub-goal buffer included: rows below n_sub, the
    utility path call's rows a shorter claim left behind, the sentinel in the rest."""
    assert int(got["n_claims"][0]) == want["n_claims"], (got["n_claims"], want["n_claims"], want["winners"])
    assert np.array_equal(got["claim_round"], want["claim_round"]), (got["claim_round"][:16], want["claim_round"][:16])
    for k in ("n_frontier", "frontier", "field", "gain", "n_sources", "ufield", "status", "n_sub", "target_cell", "target_gain"):
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:4].tolist())
    assert np.array_equal(bits(got["path_cost"]), bits(want["path_cost"]))
    claimed = want["target_cell"] >= 0
    assert np.array_equal(bits(got["target"][claimed]), bits(want["target"][claimed])) and np.isnan(got["target"][~claimed]).all()
    rows = expected_rows(want, S_max)
    assert got["sub_goals"].shape == rows.shape
    bad = np.nonzero((bits(got["sub_goals"]) != bits(rows)).any((1, 2)))[0]
    assert len(bad) == 0, (bad[:8], want["claim_round"][bad[:8]])


def check(ev, start, r_claim, r_view, w_gain, g_cap, min_gain=0, max_claims=64, r=2, mu=2, max_seg=None, S_max=64, may_claim=None,
          t=(T_FREE, T_OCC), origin=ORIGIN, cell=CELL, gain=None, want=None):
    if want is None:
        want = expected(ev, start, r_claim, r_view, w_gain, g_cap, min_gain, max_claims, r, mu, max_seg, S_max, may_claim, t, origin, cell, gain)
    got = run(ev, start, r_claim, r_view, w_gain, g_cap, min_gain, max_claims, r, mu, max_seg, S_max, may_claim, t, origin, cell, gain)
    same(got, want, S_max)
    hence(want, r_claim, max_claims)
    return got, want
