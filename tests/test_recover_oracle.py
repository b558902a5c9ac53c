"""tests/recover_oracle.py (the numpy restatement of lipmpc_fleet_recover_update_batch): the properties the capture step is
taken for, over random states at the ``tall`` dynamics, and max_recover = 0 against the plain fleet update's restatement."""
import numpy as np

import lipmpc_oracle as O
import recover_oracle as RO
from helpers import PARAM_SETS

REL = 1e-14            # the relative bar of tests/test_params_gpu.py::_lip_rel_err on one LIP advance
P = O.Params(N=5, **{("v_max" if k == "v_max_xy" else k): v for k, v in PARAM_SETS["tall"].items()})


def _states(n, seed):
    rng = np.random.default_rng(seed)
    st = rng.normal(size=(n, 5)) * np.array([3.0, 0.6, 3.0, 0.6, 1.5])
    return st, rng.normal(size=(n, 2)) * 4.0, rng


def _scale(A, Bm, x, u):
    """magnitude of the terms summed in A x + B u, per component (as _lip_rel_err)"""
    return np.abs(A) @ np.abs(x) + np.abs(Bm) @ np.abs(u)


def test_the_capture_point_is_a_fixed_point_and_the_velocity_decays():
    A, Bm = O.lip_matrices(P)
    st, goal, _ = _states(2000, 1)
    decay = P.ch - P.sh
    assert abs(decay - np.exp(-P.beta * P.dt)) < 1e-15
    for x, g in zip(st, goal):
        cp, om, new = RO.capture_advance(x.copy(), g, P)
        s = _scale(A, Bm, x[:4], cp)
        cp_new = RO.capture_point(new, P.beta)
        # cp+ = cp: p+ and v+ / beta each carry the rounding of one advance
        assert np.all(np.abs(cp_new - cp) <= REL * (s[[0, 2]] + s[[1, 3]] / P.beta)), (x, cp, cp_new)
        # v+ = (ch - sh) v
        assert np.all(np.abs(new[[1, 3]] - decay * x[[1, 3]]) <= REL * s[[1, 3]]), (x, new)
        assert abs(om) <= P.omega_max and new[4] == x[4] + om * P.sampling_time


def test_the_com_stays_on_the_segment_to_the_capture_point():
    """p+ = p + t (cp - p) with t = 1 - (ch - sh) in (0, 1), to the rounding of one advance: so any half-plane that holds p and
    cp holds p+."""
    A, Bm = O.lip_matrices(P)
    st, goal, rng = _states(2000, 2)
    t = 1.0 - (P.ch - P.sh)
    assert 0.0 < t < 1.0
    for x, g in zip(st, goal):
        cp, _, new = RO.capture_advance(x.copy(), g, P)
        p, pn = x[[0, 2]], new[[0, 2]]
        tol = REL * _scale(A, Bm, x[:4], cp)[[0, 2]]
        assert np.all(np.abs(pn - (p + t * (cp - p))) <= tol), (x, pn)
        # half-planes eta . (q - c) >= 0 through random points that hold p and cp: p+ is in them, to that rounding
        for _ in range(4):
            eta = rng.normal(size=2)
            c = p + rng.normal(size=2)
            if eta @ (p - c) < 0:
                eta = -eta
            if eta @ (cp - c) < 0:
                continue
            assert eta @ (pn - c) >= -np.abs(eta) @ tol, (x, eta, c)
        # ... and the safety margin says so: rows that hold cp give margin >= 0, one that does not a negative margin
        rows = np.array([[*(cp - u * d), *u] for u, d in zip((e / np.hypot(*e) for e in rng.normal(size=(3, 2))), (0.5, 0.25, 1.0))])
        assert RO.safety_margin(cp, rows, 0.0) >= 0.24 and RO.safety_margin(cp, rows, 0.3) < 0.0


def test_safety_margin_rules():
    cp = np.array([1.0, 2.0])
    assert RO.safety_margin(cp, None) == np.inf and RO.safety_margin(cp, np.zeros((5, 4))) == np.inf
    rows = np.array([[0.0, 0.0, 0.0, 0.0], [0.5, 2.0, 1.0, 0.0], [9.0, 9.0, 0.0, 0.0], [1.0, 1.75, 0.0, 2.0]])
    assert RO.safety_margin(cp, rows) == 0.5 and RO.safety_margin(cp, rows, 0.5) == 0.0 and RO.safety_margin(cp, rows, 0.75) == -0.25
    for i, j in ((1, 0), (1, 2), (3, 3), (0, 2)):                # a NaN in a used row, in c or in eta; in the eta of an "empty" slot
        bad = rows.copy(); bad[i, j] = np.nan
        assert RO.safety_margin(cp, bad) == -np.inf
    bad = rows.copy(); bad[0, 0] = np.nan                        # a NaN in c of a slot with eta == (0, 0): not used
    assert RO.safety_margin(cp, bad) == 0.5


def _random_call(rng, Bn, N, k_max, k, with_overflow):
    fleet = dict(state=rng.normal(size=(Bn, 5)), first_foot=rng.choice([-1, 1], Bn).astype(np.int8),
                 walking=(rng.random(Bn) < 0.8).astype(np.int8), last_obj=rng.uniform(0, 1, Bn), n_steps=rng.integers(0, 5, Bn).astype(np.int32),
                 last_status=rng.integers(0, 6, Bn).astype(np.int32), n_overflow=rng.integers(0, 3, Bn).astype(np.int32),
                 sample=np.array([k], np.int32), X_pred=rng.normal(size=(Bn, k_max + 1, 5)), U_pred=rng.normal(size=(Bn, k_max, 3)))
    out = dict(U=rng.normal(size=(Bn, N, 2)), theta=rng.normal(size=(Bn, N + 1)), omega=rng.normal(size=(Bn, N)), obj=rng.uniform(0, 1, Bn),
               status=rng.integers(0, 6, Bn).astype(np.int32))
    return fleet, out, ((rng.random(Bn) < 0.15).astype(np.int32) if with_overflow else None)


def _plain_update(fleet, out, overflow, k_max, stop_obj):
    """lipmpc_fleet_update_batch as tests/test_params_gpu.py::test_fleet_update_matches_its_contract restates it."""
    A, Bm = O.lip_matrices(P)
    k = int(fleet["sample"][0])
    fleet["sample"][0] = k + 1
    if k >= k_max:
        return
    w = (fleet["walking"] != 0) & (fleet["last_obj"] >= stop_obj)
    st = np.where(overflow != 0, 5, out["status"]) if overflow is not None else out["status"]
    if overflow is not None:
        fleet["n_overflow"] += np.where(w, overflow, 0).astype(np.int32)
    fleet["last_status"] = np.where(w, st, fleet["last_status"]).astype(np.int32)
    w &= np.isin(st, (0, 4))
    fleet["walking"] = w.astype(np.int8)
    fleet["last_obj"] = np.where(w, out["obj"], fleet["last_obj"])
    for b in np.where(w)[0]:
        fleet["state"][b, :4] = A @ fleet["state"][b, :4] + Bm @ out["U"][b, 0]
    fleet["state"][w, 4] = out["theta"][w, 1]
    fleet["first_foot"] = np.where(w, -fleet["first_foot"], fleet["first_foot"]).astype(np.int8)
    fleet["n_steps"] = (fleet["n_steps"] + w).astype(np.int32)
    fleet["U_pred"][:, k] = np.concatenate([out["U"][:, 0], out["omega"][:, :1]], axis=1)
    fleet["X_pred"][:, k + 1] = fleet["state"]


def test_max_recover_0_is_the_plain_fleet_update():
    rng = np.random.default_rng(5)
    Bn, N, k_max = 200, 5, 4
    for with_overflow in (True, False):
        for k in (0, 3, 4, 6):
            fleet, out, overflow = _random_call(rng, Bn, N, k_max, k, with_overflow)
            ref = {n: v.copy() for n, v in fleet.items()}
            _plain_update(ref, out, overflow, k_max, 0.5)
            for recover in (None, dict(recover_run=rng.integers(0, 3, Bn).astype(np.int32), n_recover=rng.integers(0, 9, Bn).astype(np.int32),
                                       recover_margin=rng.normal(size=Bn))):
                got = {n: v.copy() for n, v in fleet.items()}
                before = None if recover is None else {n: v.copy() for n, v in recover.items()}
                RO.fleet_update(P, got, out, overflow, k_max, 0.5, goal=rng.normal(size=(Bn, 2)), c_eta=rng.normal(size=(Bn, 3, 4)),
                                max_recover=0, recover=recover)
                for n in RO.FLEET:
                    assert np.array_equal(got[n], ref[n]), (with_overflow, k, n)
                if recover is not None and k < k_max:
                    assert np.array_equal(recover["n_recover"], before["n_recover"]) and np.isnan(recover["recover_margin"]).all()
                    assert np.array_equal(recover["recover_run"], before["recover_run"])


def test_the_update_recovers_exactly_where_the_rule_says():
    rng = np.random.default_rng(6)
    Bn, N, k_max, max_recover = 400, 5, 4, 2
    fleet, out, overflow = _random_call(rng, Bn, N, k_max, 1, True)
    fleet["state"][:7, 1] = np.inf                                # a non-finite state word never recovers
    c_eta = rng.normal(size=(Bn, 3, 4)); c_eta[::3, 1, 2:] = 0.0; c_eta[::7] = 0.0; c_eta[5::4, 2, 3] = np.nan
    goal, delta = rng.normal(size=(Bn, 2)), rng.uniform(0, 0.1, Bn)
    rec = dict(recover_run=rng.integers(0, 4, Bn).astype(np.int32), n_recover=rng.integers(0, 9, Bn).astype(np.int32), recover_margin=np.zeros(Bn))
    before, rb = {n: v.copy() for n, v in fleet.items()}, {n: v.copy() for n, v in rec.items()}
    w, recovered, evaluated = RO.fleet_update(P, fleet, out, overflow, k_max, 0.5, goal, c_eta, delta, max_recover, rec)
    st = np.where(overflow != 0, 5, out["status"])
    want_eval = ((before["walking"] != 0) & (before["last_obj"] >= 0.5) & np.isin(st, (1, 2)) & (rb["recover_run"] < max_recover)
                 & np.isfinite(before["state"][:, :4]).all(1))
    assert np.array_equal(evaluated, want_eval) and evaluated.sum() > 10 and recovered.sum() > 3 and (evaluated & ~recovered).sum() > 3
    assert np.array_equal(recovered, evaluated & (rec["recover_margin"] >= 0)) and np.array_equal(np.isnan(rec["recover_margin"]), ~evaluated)
    assert (rec["recover_margin"] == -np.inf).sum() > 3          # NaN rows: evaluated, refused
    assert np.array_equal(rec["recover_run"][recovered], rb["recover_run"][recovered] + 1)
    assert np.array_equal(rec["n_recover"], rb["n_recover"] + recovered)
    for n in ("last_obj", "n_steps"):
        assert np.array_equal(fleet[n][recovered], before[n][recovered])
    assert np.array_equal(fleet["last_status"][recovered], st[recovered]) and (fleet["walking"][recovered] == 1).all()
    assert np.array_equal(fleet["first_foot"][recovered], -before["first_foot"][recovered])
    assert np.array_equal(fleet["U_pred"][recovered, 1, :2], RO.capture_point(before["state"][recovered], P.beta))
