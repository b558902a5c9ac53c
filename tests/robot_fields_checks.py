"""What the tests of the claims from per-robot fields share (tests/test_robot_fields_oracle.py on the CPU,
tests/test_robot_fields_gpu.py on the device): the maps, the CASES, one oracle result per case (computed once, read only), one run of
RobotFieldsFrontierPlanner into poisoned buffers, and the comparison of EVERY output with tests/robot_fields_oracle.py, bit for bit.
The maps and the oracle side need no GPU; torch and the library are imported by the functions that run the device."""
import functools

import numpy as np

import assign_checks as AC
import assign_keep_checks as KC
import frontier_oracle as FR
import robot_fields_oracle as RF
from assign_checks import CELL, ORIGIN, SENTINEL, T_FREE, T_OCC, centres, open_field
from assign_keep_checks import GENEROUS, index

POISON = -0x01010102                                          # int32 of the bytes FE FE FE FE: not a status, a count or a flag
TW, TH = 32, 64                                               # the tile sides (tests/test_robot_fields_build.py holds them to the library's)
W2, H2 = TW + 1, TH + 8                                       # 33 x 72: 2 x 2 tiles, the second tile row ONE cell wide
SIX = [(8, 18 + k) for k in range(6)]                         # tests/test_assign_oracle.py's six side-by-side starts


def strips(W=W2, H=H2):
    """Everything known and free but two unknown columns at either end along j: the frontier is the two lines j = 2 and j = H - 3,
    across every tile row."""
    ev = np.full((W, H), -T_FREE, np.int32)
    ev[:, :2] = 0
    ev[:, H - 2:] = 0
    return ev


def serpentine(W=66, H=130, pitch=4):
    """Solid walls across j every ``pitch`` rows, each with a gap at alternating ends: the corridor crosses the tile border j = 64
    once per leg, so a field from one end needs about as many rounds as there are legs.  Unknown: the last corridor's far end."""
    ev = np.full((W, H), -T_FREE, np.int32)
    for n, i in enumerate(range(pitch - 1, W - 1, pitch)):
        ev[i, :] = T_OCC
        ev[i, H - 3:H - 1] = -T_FREE if n % 2 == 0 else T_OCC
        ev[i, 1:3] = -T_FREE if n % 2 == 1 else T_OCC
    ev[W - 2:, :6] = 0
    return ev


def big(W=363, H=362):
    """A map above 2^17 cells, unknown but a free band along its last rows: the cells a field has to relax are few, and those of
    row W - 1 from column 28 on have indices above 2^17."""
    ev = np.zeros((W, H), np.int32)
    ev[W - 30:, 20:H - 20] = -T_FREE
    return ev


def lattice(B, seed):
    """B starts on few distinct cells of the 40 x 44 open field (robots that share a cell share a field: ties go to the lower index)."""
    rng = np.random.default_rng(seed)
    cells = [(i, j) for i in range(5, 36, 6) for j in range(5, 40, 5)]
    return centres([cells[k] for k in rng.integers(0, len(cells), B)]) + rng.uniform(-0.3, 0.3, (B, 2)) * np.array(CELL)


def _case(ev, start, r_claim, max_claims=64, prev=None, keep=None, r=2, mu=2, max_seg=None, S_max=64, may_claim=None):
    start = np.ascontiguousarray(np.asarray(start, np.float64).reshape(-1, 2))
    return dict(ev=np.ascontiguousarray(ev, np.int32), start=start, r_claim=r_claim, max_claims=max_claims, prev=prev, keep=keep, r=r, mu=mu,
                max_seg=max_seg, S_max=S_max, may_claim=may_claim)


def _open6():
    return np.concatenate([centres(SIX), [[np.nan, 0.0]], centres([(0, 0)])])      # + a NaN start + a robot in the unknown corner (snap)


FAR2 = (W2 - 1, H2 - 3)                                       # a frontier cell of ``strips`` in the one-cell tile row
CORNER = [(TW - 1, TH - 1), (TW, TH - 1), (TW - 1, TH), (TW, TH)]      # the four cells round the tile corner

# name -> the case.  Every case is run by the CPU test (the Hence list) and by the GPU test (bit for bit).
CASES = {
    "open6-r5": lambda: _case(open_field(40, 44), _open6(), 5),
    "open6-r15": lambda: _case(open_field(40, 44), _open6(), 15),
    "open6-r0": lambda: _case(open_field(40, 44), _open6(), 0),
    "open6-r4096": lambda: _case(open_field(40, 44), _open6(), 4096),
    "open6-claims0": lambda: _case(open_field(40, 44), _open6(), 5, 0),
    "open6-claims1": lambda: _case(open_field(40, 44), _open6(), 5, 1),
    "open6-claims3": lambda: _case(open_field(40, 44), _open6(), 5, 3),
    "open6-may": lambda: _case(open_field(40, 44), _open6(), 5, may_claim=np.array([0, 1, 1, 0, 1, 0, 1, 1], np.int8)),
    "open6-nobody-may": lambda: _case(open_field(40, 44), _open6(), 5, may_claim=np.zeros(8, np.int8)),
    "tile-corner": lambda: _case(strips(), centres(CORNER), 40, r=0),
    "two-rooms": lambda: _case(AC.two_rooms(), centres([(5, 6), (6, 6), (7, 6), (20, 6), (21, 6)]), 12, r=0),
    "band": lambda: _case(AC.block_in_field(), centres([(12, 10), (10, 11), (10, 11), (11, 10), (4, 12)]), 6),
    "on-frontier": lambda: _case(open_field(40, 44), centres([(2, 20), (8, 20)]), 5),
    "every-cell-marked": lambda: _case(open_field(40, 44), centres(SIX[:3]), 5, max_seg=5),
    "B65": lambda: _case(open_field(40, 44), lattice(65, 65), 4, 65),
    "B300": lambda: _case(open_field(40, 44), lattice(300, 300), 9, 300),
    "big": lambda: _case(big(), centres([(340, 100), (340, 101), (362, 336), (362, 200)]), 25),
    # keep
    "keep-none": lambda: _case(open_field(40, 44), _open6(), 5, prev=np.full(8, -1), keep=(3, 24, 4)),
    "keep-all": lambda: _case(open_field(40, 44), centres(SIX), 5, prev=[index(c, 44) for c in ((2, 10), (2, 18), (2, 26), (2, 34), (10, 2), (10, 41))],
                              keep=GENEROUS),
    "keep-receded": lambda: _case(open_field(40, 44), centres(SIX[:2]), 5, prev=[index((0, 20), 44), -1], keep=(2, 1024, 4096)),
    "keep-vanished": lambda: _case(open_field(40, 44), centres(SIX[:2]), 5, prev=[index((20, 20), 44), -1], keep=(2, 1024, 4096)),
    "keep-strict-fails": lambda: _case(open_field(40, 44), centres(SIX[:3]), 5, prev=[index((37, 21), 44), index((2, 19), 44), -1],
                                       keep=(0, 16, 0)),
    "keep-out-of-range": lambda: _case(open_field(40, 44), centres(SIX[:4]), 5, prev=[40 * 44, -5, 0x7FFFFFFF, index((2, 18), 44)],
                                       keep=GENEROUS),
    "keep-cap": lambda: _case(open_field(40, 44), centres(SIX), 3, 2, prev=[index(c, 44) for c in ((2, 10), (2, 18), (2, 26), (2, 34), (10, 2), (10, 41))],
                              keep=GENEROUS),
    "keep-tile-corner": lambda: _case(strips(), centres(CORNER), 6, prev=[index(FAR2, H2), -1, index((5, 2), H2), -1], keep=(3, 64, 32), r=0),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def nearest(name):
    c = case(name)
    return FR.plan_batch(c["ev"], T_FREE, T_OCC, ORIGIN, CELL, c["start"], c["r"], c["mu"], c["max_seg"], c["S_max"])


def expected_of(c, near=None, **over):
    """The oracle on a case dict (``over``: fields of the case replaced)."""
    c = dict(c, **over)
    if near is None:
        near = FR.plan_batch(c["ev"], T_FREE, T_OCC, ORIGIN, CELL, c["start"], c["r"], c["mu"], c["max_seg"], c["S_max"])
    return RF.plan_batch(c["ev"], T_FREE, T_OCC, ORIGIN, CELL, c["start"], c["r_claim"], c["max_claims"], c["prev"], c["keep"] or (0, 16, 0),
                         c["r"], c["mu"], c["max_seg"], c["S_max"], c["may_claim"], nearest=near)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's result of a named case: computed once, shared by the tests, read only."""
    return expected_of(case(name), nearest(name))


def spaced(want, r_claim):
    return KC.spaced(want, r_claim)


# -- the device side ----------------------------------------------------------------------------------------------------------------
def planner(c, rounds=None, paths="lane"):
    import lipmpc
    keep = {} if c["keep"] is None else dict(r_keep=c["keep"][0], keep_ratio16=c["keep"][1], keep_slack=c["keep"][2])
    return lipmpc.RobotFieldsFrontierPlanner(c["r_claim"], c["max_claims"], **keep, r_inflate=c["r"], min_unknown=c["mu"], t_free=T_FREE,
                                             t_occ=T_OCC, max_seg=c["max_seg"], rounds=rounds, paths=paths)


def poison(out):
    import torch
    for k in ("sub_goals", "path_cost", "target"):
        out[k].fill_(SENTINEL)
    for k in ("n_sub", "status", "target_cell", "claim_round", "n_claims", "n_frontier", "n_kept"):
        if k in out:
            out[k].fill_(AC.POISON_I32)
    if "kept" in out:
        out["kept"].fill_(KC.POISON_I8)
    for k in ("settled", "claims_settled"):
        out[k].fill_(POISON)
    out["frontier"].fill_(9)
    out["field"].view(torch.int32).fill_(AC.POISON_WORK)


def buffers(B, W, H, S_max, keep):
    """Every output poisoned: the sentinel in the sub-goal rows, patterns no call writes in the rest."""
    import torch
    import lipmpc
    table = (lipmpc.planner.tiled_assign_keep_outputs if keep else lipmpc.planner.tiled_assign_outputs)(B, W, H, S_max)
    out = {k: torch.empty(shape, dtype=dt, device="cuda") for k, (dt, shape, _) in table.items()}
    out["settled"] = torch.empty((1,), dtype=torch.int32, device="cuda")
    poison(out)
    return out


def device(c):
    """(evidence, start, may_claim, prev_target) of a case on the device."""
    import torch
    may = None if c["may_claim"] is None else torch.as_tensor(np.asarray(c["may_claim"]), device="cuda")
    prev = None if c["prev"] is None else torch.as_tensor(np.asarray(c["prev"], np.int64).astype(np.int32), device="cuda")
    return torch.as_tensor(c["ev"], device="cuda"), torch.as_tensor(c["start"], device="cuda"), may, prev


def run(c, rounds=None, pl=None, out=None):
    import torch
    pl = pl or planner(c, rounds)
    if out is None:
        out = buffers(len(c["start"]), *c["ev"].shape, c["S_max"], c["keep"] is not None)
    ev, start, may, prev = device(c)
    if c["keep"] is None:
        got = pl.plan(ev, start, origin=ORIGIN, cell=CELL, S_max=c["S_max"], out=out, may_claim=may)
    else:
        got = pl.replan(ev, start, origin=ORIGIN, cell=CELL, S_max=c["S_max"], out=out, may_claim=may, prev_target=prev)
    torch.cuda.synchronize()
    assert got is out and pl.last is out and "work" not in out
    return AC.host(out)


def same(got, want, c):
    """Every output of the device equals the oracle's, bit for bit, the whole sub-goal buffer included."""
    assert got["settled"].tolist() == [1] and got["claims_settled"].tolist() == [1]
    AC.same(got, want, c["S_max"])
    if c["keep"] is not None:
        assert np.array_equal(got["kept"], want["kept"]), (got["kept"][:16], want["kept"][:16])
        assert got["n_kept"].tolist() == [want["n_kept"]]


def unclaimed(got, near, S_max):
    """claims_settled == 0: every row is exactly the path call's, nobody claimed."""
    B = len(near["status"])
    assert got["claims_settled"].tolist() == [0] and got["n_claims"].tolist() == [0] and (got["claim_round"] == -1).all()
    if "kept" in got:
        assert not got["kept"].any() and got["n_kept"].tolist() == [0]
    for k in ("status", "n_sub", "target_cell"):
        assert np.array_equal(got[k], near[k]), k
    assert np.array_equal(AC.bits(got["path_cost"]), AC.bits(np.asarray(near["path_cost"], np.float64)))
    want = dict(nearest=near, claim_round=np.full(B, -1), status=near["status"], n_sub=near["n_sub"], sub_goals=near["sub_goals"])
    assert np.array_equal(AC.bits(got["sub_goals"]), AC.bits(AC.expected_rows(want, S_max)))
