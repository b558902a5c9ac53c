"""lipmpc_fleet_recover_update_batch (include/lipmpc.h) restated in numpy: the fleet update of one sample in which a failed
solve costs a CAPTURE STEP instead of the robot.  ``P`` is an oracle/lipmpc_oracle.py Params (beta, ch, sh, omega_max,
sampling_time).  Every expression of the safety test is evaluated as the header writes it, in IEEE double, so the margins, the
capture points and every integer agree with the device bit for bit; the heading (atan2) and the LIP advance agree to rounding.

    capture_point      cp = p + v / beta
    safety_margin      min over the used slots of (eta_x (cp_x - c_x) + eta_y (cp_y - c_y)) - delta
    recovery_heading   the step's own heading rule at k = 0, without wrapping
    capture_advance    (A_l x + B_l cp, theta + omega_r * sampling_time)
    fleet_update       one sample for B robots, in place: with max_recover = 0 it is lipmpc_fleet_update_batch
"""
import numpy as np

import lipmpc_oracle as O

SOLVED, MAX_ITER, INFEASIBLE, DEGENERATE, UNCERTIFIED, SENSOR_OVERFLOW = 0, 1, 2, 3, 4, 5
FLEET = ("state", "first_foot", "walking", "last_obj", "n_steps", "last_status", "n_overflow", "sample", "X_pred", "U_pred")
RECOVER = ("recover_run", "n_recover", "recover_margin")


def capture_point(state, beta):
    """[...,2]: (p_x + v_x / beta, p_y + v_y / beta) of state [...,>=4] = (p_x, v_x, p_y, v_y, ...)."""
    state = np.asarray(state, float)
    return np.stack([state[..., 0] + state[..., 1] / beta, state[..., 2] + state[..., 3] / beta], axis=-1)


def safety_margin(cp, c_eta, delta=0.0):
    """The least margin of the rows c_eta [n,4] = (c_x, c_y, eta_x, eta_y) at the capture point: +inf without a used row (or
    c_eta None), -inf if a used row's margin is NaN (an evaluated margin is never NaN).  A slot is used unless eta == (0, 0) -- a NaN in eta is a used row."""
    margin, nan_row = np.inf, False
    for cx, cy, ex, ey in (() if c_eta is None else np.asarray(c_eta, float).reshape(-1, 4)):
        if ex == 0.0 and ey == 0.0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            m = (ex * (cp[0] - cx) + ey * (cp[1] - cy)) - delta
        nan_row = nan_row or m != m
        margin = np.fmin(margin, m)
    return -np.inf if nan_row else float(margin)


def recovery_heading(state, goal, P):
    """omega_r: clip(atan2(g_y - p_y, g_x - p_x) - theta, +-omega_max), the clip as C's fmin(fmax(.)) takes a NaN."""
    psi = np.arctan2(goal[1] - state[2], goal[0] - state[0])
    return float(np.fmin(np.fmax(psi - state[4], -P.omega_max), P.omega_max))


def capture_advance(state, goal, P):
    """(cp, omega_r, new state) of one recovery sample from state [5]."""
    A, Bm = O.lip_matrices(P)
    cp = capture_point(state, P.beta)
    om = recovery_heading(state, goal, P)
    return cp, om, np.concatenate([A @ state[:4] + Bm @ cp, [state[4] + om * P.sampling_time]])


def fleet_update(P, fleet, out, overflow, k_max, stop_obj, goal=None, c_eta=None, delta=None, max_recover=0, recover=None):
    """One call, in place on the dicts ``fleet`` (FLEET) and ``recover`` (RECOVER; None with max_recover = 0 = the plain
    lipmpc_fleet_update_batch).  ``out``: the step's U [B,N,2], theta [B,N+1], omega [B,N], obj [B], status [B].  Returns the
    boolean masks (walking after the call, recovered in this call, safety test evaluated)."""
    A, Bm = O.lip_matrices(P)
    B = len(fleet["state"])
    k = int(fleet["sample"][0])
    fleet["sample"][0] = k + 1
    none = np.zeros(B, bool)
    if k >= k_max:
        return fleet["walking"] != 0, none, none
    w = (fleet["walking"] != 0) & (fleet["last_obj"] >= stop_obj)
    st = np.asarray(out["status"]).copy()
    if overflow is not None:
        st = np.where(np.asarray(overflow) != 0, SENSOR_OVERFLOW, st)
        fleet["n_overflow"] += np.where(w, overflow, 0).astype(fleet["n_overflow"].dtype)
    fleet["last_status"][w] = st[w]
    solved = np.isin(st, (SOLVED, UNCERTIFIED))
    recovered, evaluated = none.copy(), none.copy()
    urow = np.concatenate([out["U"][:, 0], out["omega"][:, :1]], axis=1)
    for b in range(B):
        x = fleet["state"][b]
        if w[b] and solved[b]:
            fleet["last_obj"][b] = out["obj"][b]
            with np.errstate(invalid="ignore"):
                x[:4] = A @ x[:4] + Bm @ out["U"][b, 0]
            x[4] = out["theta"][b, 1]
            fleet["first_foot"][b] = -fleet["first_foot"][b]
            fleet["n_steps"][b] += 1
            if recover is not None and max_recover > 0:
                recover["recover_run"][b] = 0
            continue
        if recover is not None:
            recover["recover_margin"][b] = np.nan
        if not (w[b] and recover is not None and st[b] in (INFEASIBLE, MAX_ITER) and recover["recover_run"][b] < max_recover
                and np.all(np.isfinite(x[:4]))):
            w[b] = False
            continue
        evaluated[b] = True
        cp = capture_point(x, P.beta)
        m = safety_margin(cp, None if c_eta is None else c_eta[b], 0.0 if delta is None else delta[b])
        recover["recover_margin"][b] = m
        if not m >= 0.0:
            w[b] = False
            continue
        recovered[b] = True
        _, om, new = capture_advance(x.copy(), goal[b], P)
        x[:] = new
        fleet["first_foot"][b] = -fleet["first_foot"][b]
        recover["recover_run"][b] += 1
        recover["n_recover"][b] += 1
        urow[b] = (cp[0], cp[1], om)
    if recover is not None:
        recover["recover_margin"][w & solved] = np.nan
    fleet["walking"][:] = w
    fleet["U_pred"][:, k] = urow
    fleet["X_pred"][:, k + 1] = fleet["state"]
    return w, recovered, evaluated
