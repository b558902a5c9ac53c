"""GPU tests (-m gpu) of lipmpc_fleet_recover_update_batch, called directly, against its numpy restatement
(tests/recover_oracle.py) in the shape of tests/test_params_gpu.py::test_fleet_update_matches_its_contract: 300 robots (two
blocks), N = 5 at the ``tall`` dynamics, samples 0, 1, 3, 4, 6 with k_max = 4, canaries round X_pred / U_pred.

Bars: integers, flags, counters, recover_margin and the U_pred footstep bit for bit; the LIP advance 1e-14 relative to the
terms summed (test_params_gpu._lip_rel_err); theta (and omega_r, its increment) 1e-12 (tests/test_gpu_configs.py holds theta to
that).  Margins are either exactly 0 / +-2^-40 from exactly representable inputs, or farther than 1e-9 from 0, so the device
and numpy cannot part on the sign."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402
import lipmpc_oracle as O  # noqa: E402
import recover_oracle as RO  # noqa: E402
from helpers import lip_params, oracle_params  # noqa: E402

CANARY, GUARD = 4.25e100, 64
BN, K_MAX, N, N_OBS, STOP_OBJ, MAX_RECOVER = 300, 4, 5, 4, 0.05, 3
TINY = 2.0 ** -40
_T = {np.float64: torch.float64, np.int8: torch.int8, np.int32: torch.int32, np.int64: torch.int64}


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=_T[a.dtype.type], device="cuda")


def _guarded(shape, fill=CANARY):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), fill, dtype=torch.float64, device="cuda")
    return big, big[GUARD:GUARD + n].view(shape)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _lip_rel_err(A, Bm, x, u, got):
    exp = x @ A.T + u @ Bm.T
    return np.abs(got - exp) / np.maximum(np.abs(x) @ np.abs(A).T + np.abs(u) @ np.abs(Bm).T, 1e-300)


def _inputs(rng, P, k, with_overflow, rows, with_delta):
    """One call's buffers (numpy).  rows: "rows" (used, empty and NaN slots), "empty" (every slot empty) or None (NULL)."""
    Po = oracle_params(P)
    fleet = dict(state=rng.normal(size=(BN, 5)), first_foot=rng.choice([-1, 1], BN).astype(np.int8),
                 walking=(rng.random(BN) < 0.85).astype(np.int8),
                 last_obj=np.where(rng.random(BN) < 0.15, rng.uniform(0, STOP_OBJ, BN), rng.uniform(STOP_OBJ, 5.0, BN)),
                 n_steps=rng.integers(0, 5, BN).astype(np.int32), last_status=rng.integers(0, 6, BN).astype(np.int32),
                 n_overflow=rng.integers(0, 3, BN).astype(np.int32), sample=np.array([k], np.int32))
    fleet["last_obj"][:3] = STOP_OBJ
    status = rng.integers(0, 6, BN).astype(np.int32)
    status[rng.random(BN) < 0.4] = RO.INFEASIBLE                 # (enough robots at the recovery rule)
    overflow = (rng.random(BN) < 0.1).astype(np.int32) if with_overflow else None
    rec = dict(recover_run=rng.choice([MAX_RECOVER - 1, MAX_RECOVER, 0], BN).astype(np.int32), n_recover=rng.integers(0, 9, BN).astype(np.int32),
               recover_margin=rng.normal(size=BN))
    goal = rng.normal(size=(BN, 2)) * 4.0
    delta = rng.choice([0.0, 0.05, 0.25], BN) if with_delta else None
    c_eta = None
    if rows is not None:
        c_eta = np.zeros((BN, N_OBS, 4))
    if rows == "rows":
        c_eta[:] = rng.normal(size=(BN, N_OBS, 4))
        c_eta[rng.random((BN, N_OBS)) < 0.4] = 0.0               # empty slots (anywhere in the list)
        c_eta[rng.random(BN) < 0.1] = 0.0                        # no rows at all
        c_eta[20:26, 1, 2] = np.nan; c_eta[26:30, 2] = (np.nan, 0.3, 1.0, 0.5); c_eta[30:34, 0, 2:] = (0.0, np.nan)      # NaN rows
    fleet["state"][40:44, 1] = np.inf; fleet["state"][44:47, 0] = np.nan; fleet["state"][47:50, 3] = -np.inf      # a non-finite state word
    # the boundary: robots at rest (cp = p exactly) on multiples of 1/8, one row (1, 0) through p_x - d (- 0, + 2^-40, - 2^-40)
    # with delta = d: margin exactly +0, -2^-40, +2^-40.  They are at the recovery rule (walking, INFEASIBLE / MAX_ITER, run 0)
    if rows == "rows":
        z = np.arange(60, 90)
        fleet["state"][z] = 0.0
        fleet["state"][z, 0] = rng.integers(-16, 17, len(z)) / 8.0
        fleet["state"][z, 2] = rng.integers(-16, 17, len(z)) / 8.0
        fleet["state"][z, 4] = rng.normal(size=len(z))
        d = 0.25 if with_delta else 0.0
        c_eta[z] = 0.0
        c_eta[z, 2] = np.stack([fleet["state"][z, 0] - d + np.tile([0.0, TINY, -TINY], len(z) // 3), rng.normal(size=len(z)),
                                np.ones(len(z)), np.zeros(len(z))], axis=1)
        c_eta[z[::2], 0] = np.stack([fleet["state"][z[::2], 0] - 3.0, fleet["state"][z[::2], 2], np.ones(len(z[::2])), np.zeros(len(z[::2]))], axis=1)
        if with_delta:
            delta[z] = d
        fleet["walking"][z] = 1; fleet["last_obj"][z] = 1.0; rec["recover_run"][z] = 0
        status[z] = np.where(np.arange(len(z)) % 2, RO.INFEASIBLE, RO.MAX_ITER)
        if overflow is not None:
            overflow[z] = 0
        # everywhere else |margin| > 1e-9: a robot whose margin falls closer loses its rows
        for b in np.setdiff1d(np.arange(BN), z):
            m = RO.safety_margin(RO.capture_point(fleet["state"][b], Po.beta), c_eta[b], 0.0 if delta is None else delta[b])
            if abs(m) <= 1e-9:
                c_eta[b] = 0.0
    out = dict(U=rng.normal(size=(BN, N, 2)), X=np.zeros((BN, N + 1, 4)), theta=rng.normal(size=(BN, N + 1)), omega=rng.normal(size=(BN, N)),
               obj=rng.uniform(0, 1, BN), status=status, iters=np.zeros(BN, np.int32), active=np.zeros((BN, P.active_words), np.int64))
    failed = ~np.isin(status, (RO.SOLVED, RO.UNCERTIFIED))
    for n in ("U", "theta", "omega", "obj"):                     # what a failed solve leaves
        out[n][failed] = np.nan
    return fleet, out, overflow, rec, goal, c_eta, delta


def _call(sv, fleet_np, out_np, overflow, rec_np, goal, c_eta, delta, max_recover, plain=False):
    """The device call on fresh buffers; returns (fleet, rec, X_pred block, U_pred block) as numpy."""
    fleet = {k: _dev(v) for k, v in fleet_np.items()}
    xbig, fleet["X_pred"] = _guarded((BN, K_MAX + 1, 5))
    ubig, fleet["U_pred"] = _guarded((BN, K_MAX, 3))
    out, rec = {k: _dev(v) for k, v in out_np.items()}, {k: _dev(v) for k, v in rec_np.items()}
    if plain:
        sv.fleet_update(fleet, out, overflow=_dev(overflow), stop_obj=STOP_OBJ)
    else:
        sv.fleet_update(fleet, out, overflow=_dev(overflow), stop_obj=STOP_OBJ,
                        recover=dict(rec, goal=_dev(goal), c_eta=_dev(c_eta), delta=_dev(delta), max_recover=max_recover))
    torch.cuda.synchronize()
    return ({k: v.cpu().numpy() for k, v in fleet.items() if k not in ("X_pred", "U_pred")}, {k: v.cpu().numpy() for k, v in rec.items()},
            xbig.cpu().numpy(), ubig.cpu().numpy())


@pytest.mark.parametrize("with_overflow", [True, False])
@pytest.mark.parametrize("rows,with_delta", [("rows", True), ("rows", False), ("empty", True), (None, False)])
def test_recover_update_matches_its_contract(with_overflow, rows, with_delta):
    P = lip_params("tall", N=N, n_obs_max=N_OBS, v_max=5)
    Po = oracle_params(P)
    sv = lipmpc.BatchedLipMpc(P)
    A, Bm = O.lip_matrices(Po)
    rng = np.random.default_rng(11 + 2 * with_overflow + (3 if rows is None else len(rows)) + 7 * with_delta)
    seen = dict(recovered=0, refused=0, zero=0, plus=0, minus=0)
    for k in (0, 1, 3, 4, 6):
        fleet_np, out_np, overflow, rec_np, goal, c_eta, delta = _inputs(rng, P, k, with_overflow, rows, with_delta)
        got, grec, xb, ub = _call(sv, fleet_np, out_np, overflow, rec_np, goal, c_eta, delta, MAX_RECOVER)
        exp = {n: v.copy() for n, v in fleet_np.items()}
        exp["X_pred"] = np.full((BN, K_MAX + 1, 5), CANARY); exp["U_pred"] = np.full((BN, K_MAX, 3), CANARY)
        erec = {n: v.copy() for n, v in rec_np.items()}
        w, recovered, evaluated = RO.fleet_update(Po, exp, out_np, overflow, K_MAX, STOP_OBJ, goal, c_eta, delta, MAX_RECOVER, erec)
        assert got["sample"][0] == k + 1
        Xg = xb[GUARD:-GUARD].reshape(BN, K_MAX + 1, 5); Ug = ub[GUARD:-GUARD].reshape(BN, K_MAX, 3)
        assert np.all(xb[:GUARD] == CANARY) and np.all(xb[-GUARD:] == CANARY) and np.all(ub[:GUARD] == CANARY) and np.all(ub[-GUARD:] == CANARY)
        if k >= K_MAX:                                           # ignored: nothing but the sample counter moves
            for n, v in fleet_np.items():
                assert n == "sample" or np.array_equal(_bits(got[n]), _bits(v)), (k, n)
            for n, v in rec_np.items():
                assert np.array_equal(_bits(grec[n]), _bits(v)), (k, n)
            assert np.all(Xg == CANARY) and np.all(Ug == CANARY)
            continue
        for n in ("first_foot", "walking", "n_steps", "last_status", "n_overflow"):
            assert np.array_equal(got[n], exp[n]), (k, n, np.where(got[n] != exp[n])[0][:8])
        assert np.array_equal(_bits(got["last_obj"]), _bits(exp["last_obj"])), k
        for n in ("recover_run", "n_recover"):
            assert np.array_equal(grec[n], erec[n]), (k, n, np.where(grec[n] != erec[n])[0][:8])
        gm, em = grec["recover_margin"], erec["recover_margin"]
        assert np.array_equal(np.isnan(gm), np.isnan(em)) and np.array_equal(_bits(gm[~np.isnan(em)]), _bits(em[~np.isnan(em)])), \
            (k, np.where(~((gm == em) | (np.isnan(gm) & np.isnan(em))))[0][:8])
        assert np.array_equal(~np.isnan(em), evaluated)          # (a NaN row gives -inf: NaN means "not evaluated")
        # the trajectory rows: written at sample k and nowhere else
        other = [j for j in range(K_MAX) if j != k]
        assert np.all(Ug[:, other] == CANARY) and np.all(Xg[:, [j for j in range(K_MAX + 1) if j != k + 1]] == CANARY)
        assert np.array_equal(_bits(Xg[:, k + 1]), _bits(got["state"])), k
        # the footstep: bit for bit (the capture point of a recovered robot, U[b, 0] of every other)
        assert np.array_equal(_bits(Ug[:, k, :2]), _bits(exp["U_pred"][:, k, :2])), k
        assert np.array_equal(_bits(Ug[~recovered, k, 2]), _bits(exp["U_pred"][~recovered, k, 2])), k
        assert np.max(np.abs(Ug[recovered, k, 2] - exp["U_pred"][recovered, k, 2]), initial=0.0) <= 1e-12, k
        # the states: untouched unless solved-and-walking or recovered; the LIP advance to 1e-14, theta to 1e-12
        moved = (w & ~recovered) | recovered
        assert np.array_equal(_bits(got["state"][~moved]), _bits(fleet_np["state"][~moved])), k
        with np.errstate(invalid="ignore"):
            u = np.where(recovered[:, None], RO.capture_point(fleet_np["state"], Po.beta), out_np["U"][:, 0])
        fin = moved & np.isfinite(fleet_np["state"][:, :4]).all(1)
        rel = _lip_rel_err(A, Bm, fleet_np["state"][fin, :4], u[fin], got["state"][fin, :4])
        assert rel.max() <= 1e-14, (k, rel.max())
        solved = w & ~recovered
        assert np.array_equal(_bits(got["state"][solved, 4]), _bits(out_np["theta"][solved, 1])), k
        assert np.max(np.abs(got["state"][recovered, 4] - exp["state"][recovered, 4]), initial=0.0) <= 1e-12, k
        assert w.any() and (~w).any() and (w & ~recovered).any()
        seen["recovered"] += int(recovered.sum()); seen["refused"] += int((evaluated & ~recovered).sum())
        seen["zero"] += int((em == 0.0).sum()); seen["plus"] += int((em == TINY).sum()); seen["minus"] += int((em == -TINY).sum())
        if rows == "rows":
            assert recovered[60:90].sum() == 20 and evaluated[60:90].all(), k       # margin 0 and +2^-40 pass, -2^-40 does not
            assert not evaluated[40:50].any() and (em[20:34][evaluated[20:34]] == -np.inf).all()          # non-finite states; NaN rows refuse
    print(seen)
    assert seen["recovered"] > 40
    if rows == "rows":
        assert seen["refused"] > 40 and seen["zero"] == 30 and seen["plus"] == 30 and seen["minus"] == 30       # 10 each per call
    else:
        assert seen["refused"] == 0                              # no rows: the margin is +inf


@pytest.mark.parametrize("with_overflow", [True, False])
def test_max_recover_0_is_the_plain_fleet_update_bit_for_bit(with_overflow):
    P = lip_params("tall", N=N, n_obs_max=N_OBS, v_max=5)
    sv = lipmpc.BatchedLipMpc(P)
    rng = np.random.default_rng(23 + with_overflow)
    for k in (0, 3, 4):
        fleet_np, out_np, overflow, rec_np, goal, c_eta, delta = _inputs(rng, P, k, with_overflow, "rows", True)
        got, grec, xb, ub = _call(sv, fleet_np, out_np, overflow, rec_np, goal, c_eta, delta, 0)
        ref, _, xr, ur = _call(sv, fleet_np, out_np, overflow, rec_np, goal, c_eta, delta, 0, plain=True)
        for n in ref:
            assert np.array_equal(_bits(got[n]), _bits(ref[n])), (k, n)
        assert np.array_equal(_bits(xb), _bits(xr)) and np.array_equal(_bits(ub), _bits(ur)), k
        assert np.array_equal(grec["recover_run"], rec_np["recover_run"]) and np.array_equal(grec["n_recover"], rec_np["n_recover"])
        assert np.isnan(grec["recover_margin"]).all() if k < K_MAX else np.array_equal(grec["recover_margin"], rec_np["recover_margin"])


def test_a_captured_graph_replayed_three_times_equals_three_eager_calls():
    P = lip_params("tall", N=N, n_obs_max=N_OBS, v_max=5)
    sv = lipmpc.BatchedLipMpc(P)
    rng = np.random.default_rng(31)
    fleet_np, out_np, overflow, rec_np, goal, c_eta, delta = _inputs(rng, P, 0, True, "rows", True)
    # failed robots keep failing over the three calls: runs grow to max_recover and end
    fleet_np["X_pred"] = np.zeros((BN, K_MAX + 1, 5)); fleet_np["U_pred"] = np.zeros((BN, K_MAX, 3))
    fleet = {k: _dev(v) for k, v in fleet_np.items()}
    out, rec = {k: _dev(v) for k, v in out_np.items()}, {k: _dev(v) for k, v in rec_np.items()}
    args = dict(goal=_dev(goal), c_eta=_dev(c_eta), delta=_dev(delta), max_recover=MAX_RECOVER)
    ov = _dev(overflow)

    def reset():
        for k, v in fleet_np.items():
            fleet[k].copy_(_dev(v))
        for k, v in rec_np.items():
            rec[k].copy_(_dev(v))

    def call():
        sv.fleet_update(fleet, out, overflow=ov, stop_obj=STOP_OBJ, recover=dict(rec, **args))

    def snapshot():
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in {**fleet, **rec}.items()}

    reset()
    for _ in range(3):
        call()
    eager = snapshot()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    reset()
    for _ in range(3):
        graph.replay()
    replayed = snapshot()
    assert eager["sample"][0] == 3 and eager["n_recover"].sum() > rec_np["n_recover"].sum() + 60
    for k, v in eager.items():
        assert np.array_equal(_bits(v), _bits(replayed[k])), k


def test_a_recovered_robots_next_solve_starts_cold():
    """With warm-start records: the failed solve has marked the robot's record unusable, so the solve after a recovery sample
    takes exactly the iterations of a cold start from the same state; the robots that solved start warm (other counts)."""
    Bn, n_obs = 64, 2
    P = lipmpc.LipMpcParams(N=3, n_obs_max=n_obs, v_max=5, flags=lipmpc.FLAG_INTERIOR | lipmpc.FLAG_WARM_START, tol_interior=1e-6)
    sv, cold = lipmpc.BatchedLipMpc(P), lipmpc.BatchedLipMpc(P)
    assert sv.set_warm_start(Bn)
    rng = np.random.default_rng(3)
    st = np.zeros((Bn, 5)); st[:, 0] = rng.uniform(0, 2, Bn); st[:, 2] = rng.uniform(0, 2, Bn)
    k_max = 3
    fleet = {k: torch.zeros(s, dtype=dt, device="cuda") for k, (dt, s, _) in lipmpc.solver.fleet_state(Bn, k_max).items()}
    fleet["state"].copy_(_dev(st)); fleet["first_foot"].fill_(1); fleet["walking"].fill_(1); fleet["last_obj"].fill_(float("inf"))
    rec = {k: torch.zeros(s, dtype=dt, device="cuda") for k, (dt, s, _) in lipmpc.solver.recover_state(Bn).items()}
    goal = _dev(np.tile([[6.0, 5.0]], (Bn, 1)))
    free = torch.zeros((Bn, n_obs, 4), dtype=torch.float64, device="cuda")
    out = sv.alloc_outputs(Bn)

    def sample(c_eta):
        sv.plan_step_batch_c_eta(fleet["state"], goal, fleet["first_foot"], c_eta, None, out=out)
        sv.fleet_update(fleet, out, stop_obj=0.05, recover=dict(rec, goal=goal, c_eta=None, delta=None, max_recover=2))
        torch.cuda.synchronize()

    sample(free)                                                 # every robot walks: its record holds a result
    assert (fleet["n_steps"] == 1).all()
    blocked = free.clone()                                       # half the robots: a row that their position violates -> INFEASIBLE
    half = torch.arange(Bn, device="cuda") % 2 == 0
    blocked[half, 0] = torch.stack([fleet["state"][half, 0] + 1.0, fleet["state"][half, 2], torch.ones_like(fleet["state"][half, 0]),
                                    torch.zeros_like(fleet["state"][half, 0])], dim=1)
    sample(blocked)
    assert (out["status"][half] == lipmpc.STATUS_INFEASIBLE).all() and (rec["n_recover"][half] == 1).all() and (rec["n_recover"][~half] == 0).all()
    assert (fleet["walking"] == 1).all() and (fleet["n_steps"][half] == 1).all() and (fleet["n_steps"][~half] == 2).all()
    state, foot = fleet["state"].clone(), fleet["first_foot"].clone()
    ref = cold.plan_step_batch_c_eta(state, goal, foot, free, None)          # no records: every problem starts cold
    sample(free)
    torch.cuda.synchronize()
    it, it_cold, h = out["iters"].cpu().numpy(), ref["iters"].cpu().numpy(), half.cpu().numpy()
    print("iterations after recovery", it[h][:8], "cold", it_cold[h][:8], "| warm", it[~h][:8], "cold", it_cold[~h][:8])
    assert np.isin(out["status"].cpu().numpy(), (0, 4)).all() and (rec["recover_run"] == 0).all()
    assert np.array_equal(it[h], it_cold[h])
    assert (it[~h] != it_cold[~h]).any()                         # ... while a robot that solved starts from its record
