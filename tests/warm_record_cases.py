"""Cases for the warm-start record path of the step entry points (warm_step_kernel), held to the oracle bit for bit.

The idea: a step that does no iteration.  With FLAG_WARM_START | FLAG_INTERIOR and tol_interior = 1e300 the stop test
max|r_p| <= tol and mu <= tol passes at iteration 0, before anything has moved: status SOLVED, 0 iterations, and the step
returns its START POINT.  The record written back is therefore the input record shifted by one stage (the last stage
extrapolated, keeping its own multipliers), multipliers clipped to [3, 100], rows not in the problem and the k = 0 rows 0.0,
word 0 = 1.0; from a cold record it is "stand still" with 30.0 on every present row.  The oracle does the same
(plan_step(..., exact=False, warm=shift_warm_start(q, z)) returns its start), so read, stage, shift, clip, park and scatter
of every warm instantiation can be compared exactly, with a distinct value in every word of the input.

tests/test_warm_record_oracle.py shows on the CPU that the cases reach what they claim; tests/test_warm_record_gpu.py runs
them on the GPU."""
import functools
import json
import os

import numpy as np

import lipmpc_oracle as O
from helpers import closed_loop_problems

IDENTITY_TOL = 1e300
SENTINEL = -7.0e77                       # spare records (past the batch) are filled with SENTINEL - word index
B_MAX = 13                               # problems per case; a record buffer holds B_MAX + SPARE
SPARE = 3

# (N, n_obs_max): one per warm_step_kernel instantiation ...
INSTANTIATION_SHAPES = ((2, 0), (3, 3), (4, 9), (4, 14), (5, 0), (6, 4), (8, 10), (7, 13), (9, 0), (16, 4))
# ... and what completes n_obs_max in {1, 2, 3, 4, 5, 10, 13, 14} (odd counts leave the c = 1 lane of the last slot pair without a
# row) at the ends of the ranges N = 2 | 4, 5 (the NVAR switch) | 8, 9 (the lane-count switch) | 16
EXTRA_SHAPES = ((2, 1), (2, 3), (5, 5), (8, 2), (9, 3))
SHAPES = INSTANTIATION_SHAPES + EXTRA_SHAPES
# the ten instantiations as (lanes per problem, row slots per lane, variables of the factorisation)
WARM_INSTANTIATIONS = tuple((16, nl, nv) for nv in (8, 16) for nl in (0, 2, 5, 7)) + ((32, 0, 32), (32, 2, 32))

# multiplier values written over the distinct base 3.005 + 0.01 x row: both ends of the clip band exactly and from both sides, and
# values far outside it.  (No NaN: fmax and np.clip treat it differently, and include/lipmpc.h promises nothing for it.)
SPECIALS = (3.0, 100.0, np.nextafter(3.0, 0.0), np.nextafter(3.0, np.inf), np.nextafter(100.0, 0.0), np.nextafter(100.0, np.inf),
            0.0, -5.0, 1e300)
SPECIALS_PER_PROBLEM = 4
# word 0 per problem: 1.0 starts warm, "anything else = no result" starts cold (include/lipmpc.h)
WORD0 = (1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 2.0, 1.0, -1.0, 1.0, float(np.nextafter(1.0, 0.0)), 1.0, 1.0)
assert len(WORD0) == B_MAX


# ---- the instantiation rule, restated (csrc/lipmpc_api.hip: lipmpc_create, warm_capable) ---------------------------------------
def instantiation(N, n_obs_max):
    """(lanes per problem G, row slots per lane NOBS_L, variables NVAR) of the handle's kernels."""
    G = 16 if N <= 8 else 32
    need = (n_obs_max + 1) // 2
    nobs_l = 0 if need == 0 else 2 if need <= 2 else 5 if need <= 5 else 7 if need <= 7 else 13 if need <= 13 else 25
    nvar = 8 if (G == 16 and N <= 4 and nobs_l <= 7) else G
    return G, nobs_l, nvar


def warm_capable(N, n_obs_max):
    G, nobs_l, _ = instantiation(N, n_obs_max)
    return N >= 2 and nobs_l <= (2 if G == 32 else 7)


def header_supports_records(N, n_obs_max):
    """include/lipmpc.h on lipmpc_set_warm_start: "LIPMPC_E_UNSUPPORTED for N = 1, for more than 14 obstacle slots, and for
    N > 8 with more than 4 obstacle slots"."""
    return not (N == 1 or n_obs_max > 14 or (N > 8 and n_obs_max > 4))


def groups_per_wave(N):
    return 64 // instantiation(N, 0)[0]


def batch_sizes(N):
    """Batches whose last wave has padding groups: 1, groups per wave + 1, 13."""
    return (1, groups_per_wave(N) + 1, B_MAX)


# ---- record layout -------------------------------------------------------------------------------------------------------------
def warm_words(N, n_obs_max):
    return 1 + 2 * N + O.n_rows(N, n_obs_max)


def to_record_rows(z, N, slots, n_obs_max):
    """oracle z (canonical rows of the obstacles in the slots ``slots``, in that order) -> the record's rows (n_obs_max slots
    per stage; a slot not in ``slots`` is 0.0)"""
    slots = np.asarray(slots, int)
    n_b = len(slots)
    out = np.zeros(9 * N + (N + 1) * n_obs_max)
    out[:9 * N] = z[:9 * N]
    for k in range(N + 1):
        out[9 * N + k * n_obs_max + slots] = z[9 * N + k * n_b: 9 * N + (k + 1) * n_b]
    return out


def from_record_rows(z, N, slots, n_obs_max):
    slots = np.asarray(slots, int)
    n_b = len(slots)
    out = np.zeros(9 * N + (N + 1) * n_b)
    out[:9 * N] = z[:9 * N]
    for k in range(N + 1):
        out[9 * N + k * n_b: 9 * N + (k + 1) * n_b] = z[9 * N + k * n_obs_max + slots]
    return out


def oracle_start(N, n_obs_max, slots, state, record):
    """The start point of a step of the problem with the obstacle slots ``slots`` present, from ``record`` [warm_words]:
    (q0 [2N], z0 in the oracle's rows [9N + (N+1) len(slots)]) -- O.shift_warm_start of the record's rows when word 0 is
    1.0, else the cold start; the constant k = 0 rows, which are not part of the solve, as 0.0."""
    n_b = len(slots)
    if record[0] == 1.0:
        q0, z0 = O.shift_warm_start(record[1:1 + 2 * N], from_record_rows(record[1 + 2 * N:], N, slots, n_obs_max), N, n_b)
    else:
        q0, z0 = np.tile([state[0], state[2]], N), np.full(O.n_rows(N, n_b), O.IPM_Z0)
    z0 = z0.copy()
    z0[9 * N: 9 * N + n_b] = 0.0
    return q0, z0


def expected_record(N, n_obs_max, slots, state, record):
    """The record an identity step leaves: word 0 = 1.0, the start point, rows of absent slots 0.0."""
    q0, z0 = oracle_start(N, n_obs_max, slots, state, record)
    return np.concatenate([[1.0], q0, to_record_rows(z0, N, slots, n_obs_max)])


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def _present_pattern(b, n, rng):
    """Which of the n slots problem b has an obstacle in (obs_nv > 0)."""
    p = np.zeros(n, bool)
    if n == 0:
        return p
    kind = ("all", "none", "last", "hole", "first", "all", "random", "random", "hole", "random", "last", "random", "all")[b]
    if kind == "all":
        p[:] = True
    elif kind == "last":
        p[-1] = True
    elif kind == "first":
        p[0] = True
    elif kind == "hole":                         # a hole in the middle (n = 1: the hole is all there is)
        p[:] = True
        p[n // 2] = False
    elif kind == "random":
        p[:] = rng.random(n) < 0.5
    return p


def _input_record(N, n, state, present, b, rng):
    """A record with a distinct value in every word; returns it with the (canonical row, value) pairs of its special values."""
    m = O.n_rows(N, n)
    rec = np.zeros(1 + 2 * N + m)
    rec[0] = WORD0[b]
    rec[1:1 + 2 * N] = np.tile([state[0], state[2]], N) + rng.uniform(-2.0, 2.0, 2 * N)       # within a few metres of the robot
    z = 3.005 + 0.01 * np.arange(m)
    # the rows the shifted start reads and keeps: stages 1.. of the kinematic families, stages 2.. of the present slots' LDCBF rows
    live = [4 * k + i for k in range(1, N) for i in range(4)] + [4 * N + k for k in range(1, N)] + \
           [5 * N + 4 * k + i for k in range(1, N) for i in range(4)] + \
           [9 * N + k * n + j for k in range(2, N + 1) for j in np.flatnonzero(present)]
    rows = rng.choice(live, SPECIALS_PER_PROBLEM, replace=False)
    special = [(int(r), SPECIALS[(SPECIALS_PER_PROBLEM * b + i) % len(SPECIALS)]) for i, r in enumerate(rows)]
    for r, v in special:
        z[r] = v
    # every third problem: a slot that is present now has 0.0 in all its record rows (it was empty when the record was
    # written) and must start at the band's lower end
    fresh = -1
    if b % 3 == 0 and present.any():
        fresh = int(np.flatnonzero(present)[b % int(present.sum())])
        z[9 * N + fresh + n * np.arange(N + 1)] = 0.0
        special = [(r, v) for r, v in special if not (r >= 9 * N and (r - 9 * N) % n == fresh)]
    rec[1 + 2 * N:] = z
    return rec, special, fresh


@functools.lru_cache(maxsize=None)
def make_case(N, n_obs_max):
    """The case of one shape: B_MAX reachable closed-loop states (no k = 0 row violated), each with its own subset of the
    n_obs_max slots present, a synthetic input record per problem, and what an identity step makes of it."""
    n = n_obs_max
    rng = np.random.default_rng(1000 * N + n)
    OP = oracle_params(N)
    probs = []
    for st, goal, s0, obs, delta in closed_loop_problems(N, n, 4, 5, seed=40 + 17 * N + n):
        # kept: SOLVED under these parameters with every slot present (then so is every subset: a k = 0 row or a degenerate
        # closest point belongs to one obstacle)
        r = O.plan_step(st, goal, s0, obs, delta, OP, exact=False)
        if r["status"] == O.STATUS_SOLVED:
            probs.append((st, goal, s0, obs, delta))
    assert len(probs) >= B_MAX, (N, n, len(probs))
    probs = probs[:B_MAX]
    B = B_MAX
    W = warm_words(N, n)
    case = dict(N=N, n_obs_max=n, B=B, state=np.array([p[0] for p in probs]), goal=np.array([p[1] for p in probs], float),
                foot=np.array([p[2] for p in probs], np.int8), delta=np.array([p[4] for p in probs], float),
                rings=[p[3] for p in probs], present=np.zeros((B, n), bool), fresh_slot=np.full(B, -1),
                rec_in=np.zeros((B + SPARE, W)), rec_out=np.zeros((B + SPARE, W)), q_start=np.zeros((B, 2 * N)), specials=[])
    case["obs_xy"] = np.zeros((B, n, 5, 2)); case["obs_nv"] = np.zeros((B, n), np.int32)
    for b in range(B):
        pres = _present_pattern(b, n, rng)
        case["present"][b] = pres
        for j in np.flatnonzero(pres):
            ring = np.asarray(probs[b][3][j], float)
            case["obs_xy"][b, j, :len(ring)] = ring
            case["obs_nv"][b, j] = len(ring)
        rec, special, fresh = _input_record(N, n, case["state"][b], pres, b, rng)
        case["rec_in"][b], case["fresh_slot"][b] = rec, fresh
        case["specials"].append(special)
        case["rec_out"][b] = expected_record(N, n, np.flatnonzero(pres), case["state"][b], rec)
        case["q_start"][b] = case["rec_out"][b, 1:1 + 2 * N]
    for i in range(SPARE):          # padding groups write nothing: the spare records come back as they are
        case["rec_in"][B + i] = SENTINEL - np.arange(W) - 1000.0 * i
        case["rec_out"][B + i] = case["rec_in"][B + i]
    return case


def oracle_params(N):
    return O.Params(N=N, tol_interior=IDENTITY_TOL, warm_start=True)


def problem_obstacles(case, b):
    """The rings of problem b's present slots, in slot order (what the oracle is given)."""
    return [case["rings"][b][j] for j in np.flatnonzero(case["present"][b])]


def expected_after(case, k, B=None):
    """The records after k identity steps on the same states: the oracle's shift applied k times."""
    N, n = case["N"], case["n_obs_max"]
    rec = case["rec_in"].copy()
    for _ in range(k):
        for b in range(case["B"] if B is None else B):
            rec[b] = expected_record(N, n, np.flatnonzero(case["present"][b]), case["state"][b], rec[b])
    return rec


def expected_trajectory(case, b, q=None):
    """X [N+1, 4], U [N, 2] of problem b's start point (O.recover_trajectory)."""
    return O.recover_trajectory(case["q_start"][b] if q is None else q, case["state"][b, :4], oracle_params(case["N"]))


# ---- the mutations the identity cases must catch, applied to the expectation ---------------------------------------------------
def row_sources(N, n_b):
    """For every oracle row of a warm start: the record row it is read from (O.shift_warm_start on a row-coded z that the clip
    leaves alone)."""
    m = O.n_rows(N, n_b)
    code = 3.0 + 0.125 * np.arange(m)
    assert code[-1] < 100.0
    _, zs = O.shift_warm_start(np.zeros(2 * N), code, N, n_b)
    return np.rint((zs - 3.0) * 8.0).astype(int)


def mutated_record(case, b, mutation):
    """What a kernel with one of the slips of the issue's list would leave for problem b (a warm one), from the same inputs:
    "no_shift" (wsrc = lane instead of lane + 2), "no_clip", "n_obs_stride" (the slot stride taken from the problem's own
    obstacle count), "c1_owns_m" (the c = 1 lane writes its manoeuvrability slot too, over the row the c = 0 lane owns),
    "k0_kept" (the k = 0 rows not zeroed)."""
    N, n = case["N"], case["n_obs_max"]
    slots = np.flatnonzero(case["present"][b])
    n_b = len(slots)
    rec, out = case["rec_in"][b], case["rec_out"][b].copy()
    z_out = out[1 + 2 * N:]
    if mutation == "no_shift":
        z_in = from_record_rows(rec[1 + 2 * N:], N, slots, n)
        z0 = np.clip(z_in, O.WARM_Z_MIN, O.WARM_Z_MAX)
        z0[9 * N: 9 * N + n_b] = 0.0
        qp = rec[1:1 + 2 * N].reshape(N, 2)
        out[1:1 + 2 * N] = np.vstack([qp[:-1], qp[-1] + (qp[-1] - qp[-2])]).ravel()
        out[1 + 2 * N:] = to_record_rows(z0, N, slots, n)
    elif mutation == "no_clip":
        z_in = from_record_rows(rec[1 + 2 * N:], N, slots, n)
        z0 = z_in[row_sources(N, n_b)]
        z0[9 * N: 9 * N + n_b] = 0.0
        out[1 + 2 * N:] = to_record_rows(z0, N, slots, n)
    elif mutation == "n_obs_stride":
        q0, z0 = oracle_start(N, n, slots, case["state"][b], rec)
        z_out[9 * N:] = 0.0
        for k in range(N + 1):                       # slot j of stage k lands at k * n_b + j
            for i, j in enumerate(slots):
                z_out[9 * N + k * n_b + j] = z0[9 * N + k * n_b + i]
    elif mutation == "c1_owns_m":
        # the c = 1 lane of stage a holds 0.0 in the slot (the row is not its own) and writes it to 4N + a after the owner
        z_out[4 * N: 5 * N] = 0.0
    elif mutation == "k0_kept":
        # the solver parks nothing for k = 0 (no lane holds those rows): what the record held there stays
        z_out[9 * N: 9 * N + n] = rec[1 + 2 * N + 9 * N: 1 + 2 * N + 9 * N + n]
    else:
        raise ValueError(mutation)
    return out


MUTATIONS = ("no_shift", "no_clip", "n_obs_stride", "c1_owns_m", "k0_kept")


def record_figures(tag, info):
    """Measured figures of the GPU tests, merged into the JSON file LIPMPC_WARM_RECORD names (profiles/warm_record.json is
    written this way); without the variable nothing is written: the tests print every figure."""
    path = os.environ.get("LIPMPC_WARM_RECORD")
    if not path:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[tag] = info
        json.dump(rec, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass
