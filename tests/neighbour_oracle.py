"""numpy restatement of the neighbour LDCBF rows (csrc/lipmpc_neighbours.hip, lipmpc_neighbour_c_eta_batch).

Brute force over all pairs, the contract of include/lipmpc.h expression for expression in float64: which robots are present,
which are in range (strictly), the (d2, j) order, the rows written and the slots zeroed.  Every compared quantity is a
float64 sum / product / quotient / sqrt of the inputs evaluated as written, so the device's outputs equal these bit for bit.

Also here: ``plan_step_rows`` (the step oracle against given (c, eta) rows) and ``swap_run`` (a fleet's closed loop on the
oracle chain rows -> step -> advance), which the tests use to pin the row model.  Used by the tests only.
"""
import math

import numpy as np

import lipmpc_oracle as O


def present(state, radius, group=None):
    """[B] bool: group >= 0, finite position, radius finite and not negative."""
    st, rad = np.asarray(state, float), np.asarray(radius, float)
    ok = np.isfinite(st[:, 0]) & np.isfinite(st[:, 2]) & np.isfinite(rad) & ~(rad < 0.0)
    if group is not None:
        ok &= np.asarray(group) >= 0
    return ok


def neighbour_rows(state, radius, sense_range, k_rows, n_obs_max, share=0.5, group=None, first_slot=None, c_eta=None):
    """dict(c_eta [B,n_obs_max,4], n_rows [B], n_near [B], neighbours [B,k_rows]).  ``c_eta``: the buffer the rows are appended
    to (copied; default zeros): slots below first_slot keep what it holds."""
    st = np.asarray(state, np.float64)
    B = st.shape[0]
    x, y = st[:, 0], st[:, 2]
    rad = np.broadcast_to(np.asarray(radius, np.float64), (B,))
    grp = np.zeros(B, np.int64) if group is None else np.asarray(group, np.int64)
    fs = np.zeros(B, np.int64) if first_slot is None else np.clip(np.asarray(first_slot, np.int64), 0, n_obs_max)
    ce = np.zeros((B, n_obs_max, 4)) if c_eta is None else np.array(c_eta, np.float64, copy=True)
    n_rows, n_near = np.zeros(B, np.int32), np.zeros(B, np.int32)
    nbr = np.full((B, k_rows), -1, np.int32)
    ok = present(st, rad, None if group is None else grp)
    share, R = np.float64(share), np.float64(sense_range)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(B):
            order = []
            if ok[i]:
                dx, dy = x[i] - x, y[i] - y
                d2 = dx * dx + dy * dy
                dist = np.sqrt(d2)
                near = ok & (grp == grp[i]) & (dist < R)
                near[i] = False
                js = np.nonzero(near)[0]
                order = js[np.lexsort((js, d2[js]))]                  # ascending (d2, j)
                n_near[i] = len(js)
            n = min(k_rows, n_obs_max - fs[i], len(order))
            n_rows[i] = n
            for r in range(n):
                j = order[r]
                rs = rad[i] + rad[j]
                offset = rs + share * (dist[j] - rs)
                ex, ey = dx[j] / dist[j], dy[j] / dist[j]
                ce[i, fs[i] + r] = (x[j] + offset * ex, y[j] + offset * ey, ex, ey)
                nbr[i, r] = j
            ce[i, fs[i] + n:] = 0.0
    return dict(c_eta=ce, n_rows=n_rows, n_near=n_near, neighbours=nbr)


def neighbour_rows_sweep(state, radius, sense_range, k_rows, n_obs_max, share=0.5, group=None, first_slot=None, c_eta=None,
                         pairs_per_chunk=1 << 21):
    """``neighbour_rows`` for batches too large for all pairs: the present robots sorted by x, every robot's candidates the
    window |x_i - x_j| <= R (1 + 2^-10) (and the same bound on y), then the contract's expressions unchanged on the candidates.
    dist < R gives |x_i - x_j| < R (1 + 5 2^-53) in exact arithmetic (the argument at cell_of in csrc/lipmpc_neighbours.hip:
    every rounding of dx, dx dx, the sum and the root loses at most a factor 1 - 2^-53, and a dx dx below the normal doubles
    means |dx| < 2^-510), and a double below the rounded window edge is at or below the exact one, so the window holds every
    robot in range.  No grid, no hash: it shares nothing with the kernel's search.  tests/test_neighbour_cases_oracle.py holds it
    to ``neighbour_rows`` bit for bit."""
    st = np.asarray(state, np.float64)
    B = st.shape[0]
    x, y = st[:, 0], st[:, 2]
    rad = np.broadcast_to(np.asarray(radius, np.float64), (B,))
    grp = np.zeros(B, np.int64) if group is None else np.asarray(group, np.int64)
    fs = np.zeros(B, np.int64) if first_slot is None else np.clip(np.asarray(first_slot, np.int64), 0, n_obs_max)
    ce = np.zeros((B, n_obs_max, 4)) if c_eta is None else np.array(c_eta, np.float64, copy=True)
    share, R = np.float64(share), np.float64(sense_range)
    order = np.nonzero(present(st, rad, None if group is None else grp))[0]
    order = order[np.argsort(x[order], kind="stable")]
    xs = x[order]
    I, J, D2 = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0)]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        reach = R * (1.0 + 2.0 ** -10)
        lo, hi = np.searchsorted(xs, xs - reach, "left"), np.searchsorted(xs, xs + reach, "right")
        cnt = hi - lo
        ends = np.cumsum(cnt)
        a = 0
        while a < len(order):
            b = max(a + 1, int(np.searchsorted(ends, (ends[a - 1] if a else 0) + pairs_per_chunk, "right")))
            c = cnt[a:b]
            i = order[np.repeat(np.arange(a, b), c)]
            j = order[np.arange(c.sum()) - np.repeat(np.cumsum(c) - c, c) + np.repeat(lo[a:b], c)]
            keep = (np.abs(y[i] - y[j]) <= reach) & (i != j) & (grp[i] == grp[j])
            i, j = i[keep], j[keep]
            dx, dy = x[i] - x[j], y[i] - y[j]
            d2 = dx * dx + dy * dy
            near = np.sqrt(d2) < R
            I.append(i[near]); J.append(j[near]); D2.append(d2[near])
            a = b
        I, J, D2 = np.concatenate(I), np.concatenate(J), np.concatenate(D2)
        by = np.lexsort((J, D2, I))                                   # robot by robot, ascending (d2, j)
        I, J = I[by], J[by]
        n_near = np.bincount(I, minlength=B)
        rank = np.arange(len(I)) - (np.cumsum(n_near) - n_near)[I]
        n_rows = np.minimum(np.minimum(k_rows, n_obs_max - fs), n_near)
        row = rank < n_rows[I]
        i, j, rank = I[row], J[row], rank[row]
        dx, dy = x[i] - x[j], y[i] - y[j]
        d2 = dx * dx + dy * dy
        dist = np.sqrt(d2)
        rs = rad[i] + rad[j]
        offset = rs + share * (dist - rs)
        ex, ey = dx / dist, dy / dist
        ce[np.arange(n_obs_max)[None, :] >= (fs + n_rows)[:, None]] = 0.0
        ce[i, fs[i] + rank] = np.stack([x[j] + offset * ex, y[j] + offset * ey, ex, ey], 1)
    nbr = np.full((B, k_rows), -1, np.int32)
    nbr[i, rank] = j
    return dict(c_eta=ce, n_rows=n_rows.astype(np.int32), n_near=n_near.astype(np.int32), neighbours=nbr)


def plan_step_rows(state, goal, first_foot, rows, P, exact=False, delta=0.0):
    """lipmpc_oracle.plan_step against given half-spaces ``rows`` [n,4] = (c_x, c_y, eta_x, eta_y): the step oracle derives its
    rows from rings through list_c_and_eta, which is stood in for here (the rows as data, as lipmpc_plan_step_batch_c_eta
    takes them; a NaN eta ends DEGENERATE inside plan_step)."""
    rows = np.asarray(rows, float).reshape(-1, 4)
    keep = O.list_c_and_eta
    O.list_c_and_eta = lambda x0, obstacles: (rows[:, :2].copy(), rows[:, 2:].copy(), False)
    try:
        return O.plan_step(state, goal, first_foot, [None] * len(rows), delta, P, exact=exact)
    finally:
        O.list_c_and_eta = keep


def swap_scenario(n=4, ring=2.0, jitter=0.05, seed=0):
    """n robots on a circle of radius ``ring`` (jittered starts) that walk to the unjittered antipodes: state0 [n,5] heading
    toward the goal at rest, goal [n,2]."""
    a = 2.0 * math.pi * np.arange(n) / n
    circle = ring * np.stack([np.cos(a), np.sin(a)], 1)
    start = circle + jitter * np.random.default_rng(seed).standard_normal((n, 2))
    goal = -circle
    st = np.zeros((n, 5))
    st[:, 0], st[:, 2] = start[:, 0], start[:, 1]
    st[:, 4] = np.arctan2(goal[:, 1] - start[:, 1], goal[:, 0] - start[:, 0])
    return st, goal


def min_pair_distance(X):
    """Smallest pairwise CoM distance over all samples of X [B,K,5] (every robot has a state at every sample: a stopped
    robot stays where it stopped)."""
    p = np.asarray(X)[:, :, [0, 2]]
    d = np.linalg.norm(p[:, None] - p[None, :], axis=-1)
    d[np.arange(len(p)), np.arange(len(p))] = np.inf
    return float(d.min())


def swap_run(state0, goal, k_max=80, radius=0.25, sense_range=1.5, k_rows=4, n_obs_max=12, share=0.5, N=3, tol=1e-6,
             stop_obj=0.05):
    """The fleet's closed loop on the oracle chain: per sample the rows of every robot from the states at the sample's start
    (``share`` None: no rows), the interior-mode step of every walking robot, stop rule and advance as
    lipmpc_fleet_update_batch.  Returns dict(X [B,k_max+1,5] (a stopped robot's state repeats), last_status [B], n_steps [B],
    last_obj [B], n_crowded [B])."""
    st = np.array(state0, float)
    B = len(st)
    P = O.Params(N=N, tol_interior=tol, sampling_time=0.4)
    A, Bm = O.lip_matrices(P)
    foot, walking = np.ones(B, int), np.ones(B, bool)
    last_obj, last_status = np.full(B, math.inf), np.zeros(B, int)
    n_steps, n_crowded = np.zeros(B, int), np.zeros(B, int)
    X = [st.copy()]
    for _ in range(k_max):
        rows = None
        if share is not None:
            rows = neighbour_rows(st, radius, sense_range, k_rows, n_obs_max, share)
            n_crowded += rows["n_near"] > rows["n_rows"]
        new = st.copy()
        for b in range(B):
            walking[b] &= last_obj[b] >= stop_obj
            if not walking[b]:
                continue
            ce = rows["c_eta"][b, : rows["n_rows"][b]] if rows is not None else np.zeros((0, 4))
            r = plan_step_rows(st[b], goal[b], foot[b], ce, P)
            last_status[b] = r["status"]
            if r["status"] not in (O.STATUS_SOLVED, O.STATUS_UNCERTIFIED):
                walking[b] = False
                continue
            last_obj[b] = r["obj"]
            new[b, :4] = A @ st[b, :4] + Bm @ r["U"][0]
            new[b, 4] = r["theta"][1]
            foot[b] = -foot[b]
            n_steps[b] += 1
        st = new
        X.append(st.copy())
    return dict(X=np.stack(X, 1), last_status=last_status, n_steps=n_steps, last_obj=last_obj, n_crowded=n_crowded)
