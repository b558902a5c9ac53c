"""What the tests of claim hysteresis for the gain-seeded claims share (tests/test_assign_keep_utility_oracle.py,
tests/test_assign_keep_utility_gpu.py and the tiled and fleet tests): the hand-made cases, the consequences the header states, one
run of GainKeepFrontierPlanner.replan into poisoned buffers, and the comparison of EVERY output with
tests/assign_keep_utility_oracle.py, bit for bit.  The cases and the oracle side need no GPU; torch and the library are imported by
the functions that run the device."""
import functools

import numpy as np

import assign_keep_utility_oracle as KU
import assign_utility_checks as U
import frontier_oracle as FR
import gain_checks as K
from assign_checks import open_field
from gain_checks import CELL, ORIGIN, POISON_I32, T_FREE, T_OCC, bits, centres

POISON_I8 = 55
GENEROUS = (0, 1024, 4096)                                    # (r_keep, keep_ratio16, keep_slack): the target itself, at any utility
RECORD_GAIN = (15, 16, 120, 0)                                # (r_view, w_gain, g_cap, min_gain) of the exploration records


def index(c, H):
    return c[0] * H + c[1]


def expected(ev, start, r_claim, gainp, prev, keep, max_claims=64, r=2, mu=2, max_seg=None, S_max=64, may_claim=None, t=(T_FREE, T_OCC),
             origin=ORIGIN, cell=CELL, gain=None, informed=None):
    """``gainp`` = (r_view, w_gain, g_cap, min_gain); ``keep`` = (r_keep, keep_ratio16, keep_slack)."""
    start = np.asarray(start, np.float64).reshape(-1, 2)
    return KU.plan_batch(ev, t[0], t[1], origin, cell, start, r_claim, gainp[0], gainp[1], gainp[2], prev, *keep, gainp[3], max_claims, r,
                         mu, max_seg, S_max, may_claim, gain=gain, informed=informed)


def spaced(want, r_claim):
    """The targets of any two winners, kept or claimed, are more than r_claim apart."""
    t = np.array(want["targets"]).reshape(-1, 2)
    d2 = ((t[:, None] - t[None]) ** 2).sum(2)[np.triu_indices(len(t), 1)]
    return bool((d2 > r_claim * r_claim).all())


def hence(want, r_claim, max_claims):
    """The consequences include/lipmpc.h states that can be read off one result of the oracle."""
    inf = want["informed"]
    H = want["field"].shape[2]
    n, tg = want["n_claims"], want["targets"]
    assert n == len(want["winners"]) <= want["slots"] <= max_claims and n == int((want["claim_round"] >= 0).sum())
    assert sorted(want["claim_round"][want["claim_round"] >= 0].tolist()) == list(range(n))
    assert want["n_kept"] == int(want["kept"].sum()) == sum(r["kept"] for r in want["attempts"]) <= n
    assert want["slots"] == len(want["attempts"]) + n - want["n_kept"]          # a spent slot is a keep attempt or a round with a winner
    assert spaced(want, r_claim), tg
    for b in range(len(want["status"])):
        k = int(want["claim_round"][b])
        if k < 0:                                              # everyone else: the utility path call's rows, and not kept
            assert not want["kept"][b]
            for key in ("status", "n_sub", "target_cell", "target_gain"):
                assert want[key][b] == inf[key][b], (key, b)
            assert np.array_equal(bits(want["path_cost"][b:b + 1]), bits(inf["path_cost"][b:b + 1])), b
            assert np.array_equal(bits(want["sub_goals"][b]), bits(inf["sub_goals"][b])), b
        else:
            assert want["status"][b] in (FR.FOUND, FR.PATH_OVERFLOW) and want["target_cell"][b] == tg[k][0] * H + tg[k][1]
            assert want["target_gain"][b] == want["gain"][0][tg[k]]
    for rec in want["attempts"]:                               # a keeper's target is its anchor
        if rec["kept"]:
            assert want["target_cell"][rec["robot"]] == index(rec["anchor"], H)
    if max_claims == 0:
        assert n == 0 and want["slots"] == 0


# -- the hand-made cases -------------------------------------------------------------------------------------------------------------
POCKET_NEAR, POCKET_FAR = (2, 20), (37, 24)
POCKET_STARTS = centres(((12, 22), (30, 22)))
POCKET_GAIN = (4, 16, 120, 1)
POCKET_R_CLAIM = 6


def two_pockets():
    """(evidence 40 x 44, gain): an open field whose frontier ring holds two pockets of hand-written gain -- NEAR (2, 20), gain 60,
    and FAR (37, 24), gain 110; every other cell has gain 0, and with min_gain 1 the two are the only sources.  Robot 0 stands
    nearer to NEAR, robot 1 nearer to FAR.  With w_gain 16 and g_cap 120 a seed is 120 - gain cost units (5 to a cell)."""
    ev = open_field(40, 44)
    gain = np.zeros((40, 44), np.int32)
    gain[POCKET_NEAR], gain[POCKET_FAR] = 60, 110
    return ev, gain


KEPT_A = (1, 12)
KEPT_START = centres(((1, 1),))
KEPT_KW = dict(r=0, mu=1)
KEPT_GAIN = (2, 16, 100, 1)


def kept_corridor(gain_a=40, gain_b=70):
    """(evidence 3 x 16, gain): tests/gain_checks.py's corridor, longer, with the two sources A = (1, 12) and B = (1, 4) and a robot
    at (1, 1).  With w_gain 16 and g_cap 100: seed(A) = 60 and A is 11 cells = 55 cost units from the robot, so keepfield[s] = 115;
    seed(B) = 30 and B is 3 cells = 15 units away, so near = ufield[s] = 45.  16 * 115 = 1840 = 32 * 45 + 80 * 5 holds with
    equality at keep_ratio16 32 and keep_slack 5, and fails at keep_slack 4."""
    ev = np.full((3, 16), T_OCC, np.int32)
    ev[1, :] = -T_FREE
    ev[0, 12] = ev[0, 4] = 0
    gain = np.zeros((3, 16), np.int32)
    gain[KEPT_A], gain[(1, 4)] = gain_a, gain_b
    return ev, gain


@functools.lru_cache(maxsize=None)
def fleet_prev():
    """Previous targets for the 130 robots of ``K.fleet_case()``: wall cells, -1, W * H, INT32 min and max, and cells all over the
    48 x 36 map."""
    rng = np.random.default_rng(23)
    prev = rng.integers(0, 48 * 36, 130).astype(np.int64)
    prev[::7] = -1
    prev[3], prev[12], prev[13], prev[14], prev[15] = index((5, 5), 36), 48 * 36, -(1 << 31), (1 << 31) - 1, index((38, 20), 36)
    prev[20:40] = [index((43, 2 + (3 * k) % 33), 36) for k in range(20)]      # along the unknown band: frontier cells
    return prev.astype(np.int32)


# -- the device --------------------------------------------------------------------------------------------------------------------
def buffers(B, W, H, S_max, table=None):
    """Every output poisoned: the sentinel in the sub-goal rows, patterns no call writes in the rest."""
    import lipmpc
    out = U.buffers(B, W, H, S_max, lipmpc.planner.assign_keep_utility_outputs(B, W, H, S_max) if table is None else table)
    poison(out)
    return out


def poison(out):
    U.poison(out)
    out["kept"].fill_(POISON_I8)
    out["n_kept"].fill_(POISON_I32)
    for k in ("settled", "usettled", "claims_settled"):
        if k in out:
            out[k].fill_(POISON_I32)


def host(out):
    return U.host(out)


def planner(r_claim, gainp, keep, max_claims=64, r=2, mu=2, max_seg=None, t=(T_FREE, T_OCC), gain=None, cls=None, **kw):
    import lipmpc
    return U.planner(r_claim, *gainp, max_claims, r, mu, max_seg, t, gain, cls or lipmpc.GainKeepFrontierPlanner, r_keep=keep[0],
                     keep_ratio16=keep[1], keep_slack=keep[2], **kw)


def run(ev, start, r_claim, gainp, prev, keep, max_claims=64, r=2, mu=2, max_seg=None, S_max=64, may_claim=None, t=(T_FREE, T_OCC),
        origin=ORIGIN, cell=CELL, gain=None, cls=None, table=None, **kw):
    import torch
    ev, start = np.ascontiguousarray(ev, np.int32), np.ascontiguousarray(np.asarray(start, np.float64).reshape(-1, 2))
    W, H = ev.shape
    out = buffers(len(start), W, H, S_max, None if table is None else table(len(start), W, H, S_max))
    pl = planner(r_claim, gainp, keep, max_claims, r, mu, max_seg, t, gain, cls, **kw)
    may = None if may_claim is None else torch.as_tensor(np.asarray(may_claim), device="cuda")
    prev = None if prev is None else torch.as_tensor(np.asarray(prev, np.int32), device="cuda")
    got = pl.replan(torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda"), origin=origin, cell=cell, S_max=S_max,
                    out=out, may_claim=may, prev_target=prev)
    torch.cuda.synchronize()
    assert got is out and pl.last is out
    return host(out)


def same(got, want, S_max):
    """tests/assign_utility_checks.py's comparison of every output, then kept and n_kept."""
    U.same(got, want, S_max)
    assert np.array_equal(got["kept"], want["kept"]), (got["kept"][:16], want["kept"][:16])
    assert got["n_kept"].tolist() == [want["n_kept"]]


def check(ev, start, r_claim, gainp, prev, keep, max_claims=64, r=2, mu=2, max_seg=None, S_max=64, may_claim=None, t=(T_FREE, T_OCC),
          origin=ORIGIN, cell=CELL, gain=None, want=None):
    if want is None:
        want = expected(ev, start, r_claim, gainp, prev, keep, max_claims, r, mu, max_seg, S_max, may_claim, t, origin, cell, gain)
    got = run(ev, start, r_claim, gainp, prev, keep, max_claims, r, mu, max_seg, S_max, may_claim, t, origin, cell, gain)
    same(got, want, S_max)
    hence(want, r_claim, max_claims)
    return got, want
