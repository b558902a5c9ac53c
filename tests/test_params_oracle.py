"""CPU tests (-m "not gpu") of the step problem at robot parameters other than the reference's config.yml
(helpers.PARAM_SETS): the oracles' algebra, their agreement and the presolve's soundness where the defaults' symmetries
(l_max = -l_min, equal x / y bounds, dt == sampling_time, h_com = 1) no longer hide a slip, which rows the batches make
tight, and the proof that tests/test_params_gpu.py would see a kernel that read a wrong constant."""
import dataclasses
import functools

import numpy as np
import pytest

import c_oracle
import lipmpc
import lipmpc_oracle as O
from helpers import (HANDLE_ONLY_FIELDS, NON_DEFAULT_SETS, ORACLE_FIELD_MAP, ORACLE_FROM_FLAGS, PARAM_SETS, ROW_FAMILIES,
                     assert_active_sets, closed_loop_problems, compare_active_sets, family_counts, lip_params, oracle_params,
                     row_family_batch)

SETS = tuple(PARAM_SETS)
N_CPU, NOBS_CPU = 6, 10          # 16 lanes per problem on the GPU; small enough for the numpy oracle


@functools.lru_cache(maxsize=None)
def _batch(name, B=384, seed=11):
    return row_family_batch(name, N_CPU, NOBS_CPU, B, seed)


def _c(name, bt, flags=0, goal=None, **over):
    P = dataclasses.replace(lip_params(name, N=N_CPU, n_obs_max=NOBS_CPU, v_max=5, flags=flags), **over)
    return c_oracle.plan_step_batch(P, bt["state"], bt["goal"] if goal is None else goal, bt["foot"], bt["xy"], bt["nv"],
                                    bt["delta"], n_threads=8)


@functools.lru_cache(maxsize=None)
def _numpy_answers(name, n=96):
    """numpy oracle (exact mode) on the first n problems of the set's batch"""
    bt = _batch(name)
    P = oracle_params(lip_params(name, N=N_CPU))
    return [O.plan_step(bt["state"][b], bt["goal"][b], int(bt["foot"][b]), bt["rings"](b), float(bt["delta"][b]), P)
            for b in range(n)]


def test_oracle_params_maps_every_field():
    """helpers.oracle_params carries every field of LipMpcParams that the oracle has a counterpart for, under its own name
    (LipMpcParams.v_max is the vertex-slot count, O.Params.v_max is V_MAX): a field added to either dataclass without
    being mapped fails here."""
    lip_fields = {f.name for f in dataclasses.fields(lipmpc.LipMpcParams)}
    orc_fields = {f.name for f in dataclasses.fields(O.Params)}
    assert set(ORACLE_FIELD_MAP) | set(ORACLE_FROM_FLAGS) == orc_fields
    assert set(ORACLE_FIELD_MAP.values()) | set(HANDLE_ONLY_FIELDS) == lip_fields
    assert set(ORACLE_FIELD_MAP.values()).isdisjoint(HANDLE_ONLY_FIELDS)
    # every mapped value arrives: a LipMpcParams with each field moved off its default
    d = lipmpc.LipMpcParams()
    moved = {}
    for f in ORACLE_FIELD_MAP.values():
        v = getattr(d, f)
        moved[f] = (v[0] * 1.5 + 0.01, v[1] * 0.5 - 0.02) if isinstance(v, tuple) else (v + 3 if isinstance(v, int) else v * 1.25 + 0.001)
    P = oracle_params(lipmpc.LipMpcParams(**moved))
    for o, f in ORACLE_FIELD_MAP.items():
        assert getattr(P, o) == moved[f] and getattr(P, o) != getattr(O.Params(), o), (o, f)
    assert P.v_max == moved["v_max_xy"]
    assert oracle_params(d) == O.Params()
    assert oracle_params(lipmpc.LipMpcParams(flags=lipmpc.FLAG_NO_PRESOLVE)).presolve is False
    assert oracle_params(lipmpc.LipMpcParams(flags=lipmpc.FLAG_WARM_START)).warm_start is True
    # the C struct the handle and the C oracle read takes the same values
    c = lipmpc.LipMpcParams(**moved).to_c()
    for f in ORACLE_FIELD_MAP.values():
        v = getattr(c, f)
        assert (tuple(v) if isinstance(moved[f], tuple) else v) == moved[f], f


def test_closed_loop_problems_default_is_the_reference_config():
    a = list(closed_loop_problems(6, 5, 2, 8, seed=3))
    b = list(closed_loop_problems(6, 5, 2, 8, seed=3, params=O.Params(N=99)))
    assert len(a) == len(b) > 8
    for p, q in zip(a, b):
        assert np.array_equal(p[0], q[0]) and p[1:3] == q[1:3] and all(np.array_equal(r, s) for r, s in zip(p[3], q[3]))
    c = list(closed_loop_problems(6, 5, 2, 8, seed=3, params=oracle_params(lip_params("dyn"))))
    assert not np.array_equal(a[1][0], c[1][0])                  # the walk does use the parameters


@pytest.mark.parametrize("name", SETS)
def test_position_form_is_reference_form(name):
    """test_oracle.py::test_position_form_is_reference_form at each parameter set: the position form (kappa, the reach rows
    in l_max / l_min / ell) is the reference's (X, U) form through A_l, B_l (beta = sqrt(g / h_com), dt)."""
    rng = np.random.default_rng(5)
    for N, n_obs in ((3, 3), (8, 10)):
        P = oracle_params(lip_params(name, N=N))
        x0 = np.array([1.0, 0.2, 2.0, -0.1])
        th, om = O.precompute_theta_omega(x0, 0.3, (10, 10), P)
        assert np.allclose(np.diff(th), om * P.sampling_time, rtol=0, atol=1e-15)
        for s0 in (1, -1):
            s_v = [s0 if i % 2 == 0 else -s0 for i in range(N + 1)]
            cs = rng.uniform(0, 5, (n_obs, 2))
            et = rng.normal(size=(n_obs, 2)); et /= np.linalg.norm(et, axis=1)[:, None]
            Gq, hq, g = O.build_qp_position_form(x0, th, om, (10, 10), s_v, cs, et, 0.1, P)
            Gu, hu, H, f, T, t0 = O.build_qp_reference_form(x0, th, om, (10, 10), s_v, cs, et, 0.1, P)
            assert np.linalg.matrix_rank(T) == 2 * N
            assert np.allclose(Gq @ T, Gu, atol=1e-9 * np.abs(Gu).max())
            assert np.allclose(hq - Gq @ t0, hu, atol=1e-9 * (1 + np.abs(hu).max()))
            assert np.allclose(H, 2 * T.T @ T)


@pytest.mark.parametrize("name", SETS)
def test_oracle_answer_is_the_exact_minimiser(name):
    """The oracle's footsteps at each set are the minimiser an independent method (Lawson-Hanson NNLS on the least-distance
    dual, O.solve_qp_ldp_nnls) finds, within 1e-7, and primal feasible."""
    bt = _batch(name)
    P = oracle_params(lip_params(name, N=N_CPU))
    worst, n = 0.0, 0
    for b, r in enumerate(_numpy_answers(name)):
        if r["status"] != O.STATUS_SOLVED:
            continue
        s0 = int(bt["foot"][b])
        s_v = [s0 if i % 2 == 0 else -s0 for i in range(N_CPU + 1)]
        G, h, g = O.build_qp_position_form(bt["state"][b][:4], r["theta"], r["omega"], bt["goal"][b], s_v, r["c"], r["eta"],
                                           float(bt["delta"][b]), P)
        k0 = slice(9 * N_CPU, 9 * N_CPU + NOBS_CPU)            # constants of the step, checked against k0_tol
        keep = np.ones(len(h), bool); keep[k0] = False
        qt = O.solve_qp_ldp_nnls(G[keep], h[keep], g)
        assert qt is not None, b
        worst = max(worst, float(np.max(np.abs(qt - r["q"]))))
        assert np.min(h[keep] - G[keep] @ r["q"]) > -1e-8, b
        n += 1
    print(name, "solved", n, "max |q_oracle - q_ldp|", worst)
    assert n >= 0.85 * len(_numpy_answers(name)) and worst < 1e-7, (name, n, worst)


@pytest.mark.parametrize("name", SETS)
def test_c_oracle_equals_numpy_oracle(name):
    """test_abi_and_c_oracle.py::test_c_oracle_equals_numpy_oracle at each set: the C oracle reads every constant as the numpy
    oracle does (status, iterations, U, X, theta / omega and c / eta bit for bit, active and working sets)."""
    bt = _batch(name)
    out = _c(name, bt)
    nr = 9 * N_CPU + (N_CPU + 1) * NOBS_CPU
    act, work = lipmpc.unpack_active(out["active"], nr), lipmpc.unpack_active(out["working"], nr)
    for b, r in enumerate(_numpy_answers(name)):
        assert r["status"] == out["status"][b] and r["iters"] == out["iters"][b], (name, b, r["status"], out["status"][b])
        assert np.array_equal(out["theta"][b], r["theta"]) and np.array_equal(out["omega"][b], r["omega"])
        assert np.array_equal(out["c_eta"][b][:, :2], r["c"]) and np.array_equal(out["c_eta"][b][:, 2:], r["eta"])
        if r["status"] in (O.STATUS_SOLVED, O.STATUS_UNCERTIFIED):
            assert np.max(np.abs(out["U"][b] - r["U"])) < 1e-8 and np.max(np.abs(out["X"][b] - r["X"])) < 1e-8, (name, b)
        assert np.array_equal(act[b], r["active"]) and np.array_equal(work[b], r["working"]), (name, b)


@pytest.mark.parametrize("name", SETS)
def test_presolve_is_sound(name):
    """The LDCBF rows the presolve drops (reach_step from l_max, l_min and ell) leave the answer unchanged -- same statuses,
    footsteps within 1e-7, same active sets -- and every dropped row keeps a slack of at least SCREEN_MARGIN at the optimum
    with every row kept, and at the optima for three other goals from the same state (other points of the same feasible
    set).  All three implementations evaluate the same rule, so only this test can see an unsound one."""
    bt = _batch(name)
    B = len(bt["state"])
    on, off = _c(name, bt), _c(name, bt, flags=lipmpc.FLAG_NO_PRESOLVE)
    assert np.array_equal(on["status"], off["status"]), name
    ok = on["status"] == 0
    assert ok.sum() >= 0.85 * B and np.max(np.abs(on["U"][ok] - off["U"][ok])) < 1e-7, name
    info, _ = compare_active_sets(ok, on, off)
    assert_active_sets(f"presolve on / off ({name})", info, 0.97)
    assert info["working_mismatch_decisive"] == 0, info
    rng = np.random.default_rng(4)
    P = oracle_params(lip_params(name, N=N_CPU))
    goals = [bt["goal"]] + [bt["state"][:, [0, 2]] + rng.uniform(-4, 4, (B, 2)) for _ in range(3)]
    dropped, worst = 0, np.inf
    for gi, goal in enumerate(goals):
        res = off if gi == 0 else _c(name, bt, flags=lipmpc.FLAG_NO_PRESOLVE, goal=goal)
        for b in range(B):
            if res["status"][b] not in (O.STATUS_SOLVED, O.STATUS_UNCERTIFIED):
                continue
            x0 = bt["state"][b][:4]
            ce = res["c_eta"][b]
            cs, etas = ce[:, :2], ce[:, 2:]
            red, n_d, _ = O.presolve_ldcbf(x0, cs, etas, float(bt["delta"][b]), P)
            if not n_d:
                continue
            p = res["X"][b][1:, [0, 2]]                                           # p_1..p_N
            slack = np.einsum("jc,kjc->kj", etas, p[:, None, :] - cs[None]) - bt["delta"][b]
            worst = min(worst, float(slack[red].min()))
            dropped += n_d if gi == 0 else 0
    print(name, "rows dropped", dropped, "smallest slack of a dropped row", worst)
    assert dropped > 0.3 * B * N_CPU and worst >= O.SCREEN_MARGIN * (1 - 1e-6), (name, dropped, worst)


def _vx_reachable(P):
    """V_MAX_x bounds v_k (k = 1..N) only where the next stage can still be reached: v_{k+1} = -v_k + kappa (p_{k+1} - p_k)
    >= v_min_x needs v_k <= kappa l_max_x - v_min_x (and v_N has v_{N-1} >= v_min_x before it)."""
    return P.kappa * P.l_max[0] - P.v_min[0]


@pytest.mark.parametrize("name", SETS)
def test_every_row_family_is_tight_somewhere(name):
    """Coverage of the batches the parity tests run on: in each family of rows (reach up / down in x and y,
    manoeuvrability, walking velocity up / down in x and y, LDCBF) some solved problems have a tight row.  At the reference
    config V_MAX_x = 0.8 is out of reach (kappa l_max_x - v_min_x = 0.66): that family is empty there by construction."""
    bt = _batch(name)
    out = _c(name, bt)
    nr = 9 * N_CPU + (N_CPU + 1) * NOBS_CPU
    ok = out["status"] == 0
    cnt = family_counts(lipmpc.unpack_active(out["active"], nr)[ok], N_CPU, NOBS_CPU)
    print(name, cnt)
    P = oracle_params(lip_params(name, N=N_CPU))
    assert tuple(cnt) == ROW_FAMILIES
    for f, c in cnt.items():
        if f == "vel_hi_x" and P.v_max[0] > _vx_reachable(P):
            assert c == 0, (name, cnt)
        else:
            assert c >= 3, (name, f, cnt)
    assert (name == "ref") == (P.v_max[0] > _vx_reachable(P))       # every other set reaches it


# one slip of a kernel that reads a wrong constant, as a mutation of the parameters: name -> LipMpcParams -> overrides
MUTATIONS = {
    "swap_xy_l_max": lambda P: dict(l_max=P.l_max[::-1]),
    "swap_xy_l_min": lambda P: dict(l_min=P.l_min[::-1]),
    "swap_xy_v_min": lambda P: dict(v_min=P.v_min[::-1]),
    "swap_xy_v_max_xy": lambda P: dict(v_max_xy=P.v_max_xy[::-1]),
    "l_max_from_minus_l_min": lambda P: dict(l_max=(-P.l_min[0], -P.l_min[1])),
    "swap_dt_sampling_time": lambda P: dict(dt=P.sampling_time, sampling_time=P.dt),
    "h_com_1": lambda P: dict(h_com=1.0),
    "ell_default": lambda P: dict(ell=0.05),
}


def test_a_slip_in_any_constant_moves_the_answer():
    """Sensitivity: for each non-default set and each mutation that changes a value there, the C oracle's answer on the
    set's batch moves (U by more than 1e-6, or the status) on at least 5 % of the problems -- so a kernel reading the wrong
    field would differ from the oracle where tests/test_params_gpu.py compares them.  Every mutation is live at some set."""
    table, live = {}, set()
    for name in NON_DEFAULT_SETS:
        bt = _batch(name)
        base = _c(name, bt)
        P = lip_params(name)
        for mname, mut in MUTATIONS.items():
            over = {k: tuple(v) if isinstance(v, tuple) else v for k, v in mut(P).items()}
            if all(getattr(P, k) == v for k, v in over.items()):
                continue                                   # the set is symmetric in this field: nothing to see
            live.add(mname)
            m = _c(name, bt, **over)
            both = np.isin(base["status"], (0, 4)) & np.isin(m["status"], (0, 4))
            du = np.zeros(len(both))
            du[both] = np.max(np.abs(base["U"][both] - m["U"][both]), axis=(1, 2))
            moved = (base["status"] != m["status"]) | (du > 1e-6)
            table[(name, mname)] = float(moved.mean())
    for (name, mname), share in sorted(table.items()):
        print(f"{name:8s} {mname:24s} {100 * share:6.1f} % of the problems change")
    assert live == set(MUTATIONS), set(MUTATIONS) - live
    low = {k: v for k, v in table.items() if v < 0.05}
    assert not low, low
