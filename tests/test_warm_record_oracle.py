"""The warm-record cases (tests/warm_record_cases.py) reach what they claim -- CPU only: every warm_step_kernel instantiation,
every row family with slots present and absent, both ends of the clip band from both sides; the oracle's identity step returns
the expectation exactly; and each slip the GPU comparison is there to catch changes the expectation."""
import re
import os

import numpy as np
import pytest

import lipmpc_oracle as O
import warm_record_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_rule_matches_the_sources():
    """The Python restatement against the lines it restates (lipmpc_create's G / nobs_l / nvar, warm_capable) and against the
    header's sentence over every handle lipmpc_create admits."""
    api = open(os.path.join(ROOT, "humanoid-navigation-using-mpc-ldcbf_amd", "csrc", "lipmpc_api.hip")).read()
    squeeze = lambda s: re.sub(r"\s+", " ", s)
    for line in ("h->G = (p->N <= 8) ? 16 : 32;",
                 "const int need = (p->n_obs_max + 1) / 2;",
                 "h->nobs_l = need == 0 ? 0 : need <= 2 ? 2 : need <= 5 ? 5 : need <= 7 ? 7 : need <= 13 ? 13 : 25;",
                 "h->nvar = (h->G == 16 && p->N <= 4 && h->nobs_l <= 7) ? 8 : h->G;",
                 "return h->p.N >= 2 && h->nobs_l <= (h->G == 32 ? 2 : 7);"):
        assert line in squeeze(api), line
    hdr = squeeze(open(os.path.join(ROOT, "include", "lipmpc.h")).read().replace("\n *", " "))
    assert "LIPMPC_E_UNSUPPORTED for N = 1, for more than 14 obstacle slots, and for N > 8 with more than 4 obstacle slots" in hdr
    for N in range(1, 17):
        for n in range(0, 51):
            assert W.warm_capable(N, n) == W.header_supports_records(N, n), (N, n)


def test_every_warm_instantiation_is_reached():
    reached = {W.instantiation(N, n) for N, n in W.INSTANTIATION_SHAPES}
    assert reached == set(W.WARM_INSTANTIATIONS) and len(W.WARM_INSTANTIATIONS) == 10
    assert [W.instantiation(N, n) for N, n in W.INSTANTIATION_SHAPES] == \
        [(16, 0, 8), (16, 2, 8), (16, 5, 8), (16, 7, 8), (16, 0, 16), (16, 2, 16), (16, 5, 16), (16, 7, 16), (32, 0, 32), (32, 2, 32)]
    assert all(W.warm_capable(N, n) for N, n in W.SHAPES)
    # the ends of each range, and every slot count the issue names
    assert {2, 4, 5, 8, 9, 16} <= {N for N, _ in W.SHAPES}
    assert {1, 2, 3, 4, 5, 10, 13, 14} <= {n for _, n in W.SHAPES}
    # the 8-variable factorisation at its last horizon, the 16-variable one at its first; 16 lanes at their last horizon, 32 at theirs
    assert W.instantiation(4, 14)[2] == 8 and W.instantiation(5, 0)[2] == 16
    assert W.instantiation(8, 10)[0] == 16 and W.instantiation(9, 0)[0] == 32
    for N, _ in W.SHAPES:
        gpw = W.groups_per_wave(N)
        assert all(B % gpw != 0 for B in W.batch_sizes(N)), N            # the last wave has padding groups


@pytest.mark.parametrize("N,n", W.SHAPES)
def test_oracle_identity_step_returns_the_expectation(N, n):
    """Every problem kept: SOLVED with 0 iterations in the oracle, q_ipm / z_ipm equal to the expectation exactly; U and X are
    recover_trajectory of the start."""
    case = W.make_case(N, n)
    OP = W.oracle_params(N)
    for b in range(case["B"]):
        slots = np.flatnonzero(case["present"][b])
        obs = W.problem_obstacles(case, b)
        st, rec = case["state"][b], case["rec_in"][b]
        warm = None
        if rec[0] == 1.0:
            warm = O.shift_warm_start(rec[1:1 + 2 * N], W.from_record_rows(rec[1 + 2 * N:], N, slots, n), N, len(slots))
        r = O.plan_step(st, case["goal"][b], int(case["foot"][b]), obs, case["delta"][b], OP, exact=False, warm=warm)
        assert r["status"] == O.STATUS_SOLVED and r["iters"] == 0, (b, r["status"], r["iters"])
        out = case["rec_out"][b]
        assert out[0] == 1.0
        assert np.array_equal(np.asarray(r["q_ipm"]).ravel(), out[1:1 + 2 * N]), b
        assert np.array_equal(W.to_record_rows(r["z_ipm"], N, slots, n), out[1 + 2 * N:]), b
        X, U = W.expected_trajectory(case, b)
        assert np.array_equal(X, r["X"]) and np.array_equal(U, r["U"])
        if warm is None:           # the cold start: 0.0 and 30.0 only
            assert set(np.unique(out[1 + 2 * N:])) <= {0.0, O.IPM_Z0}
            assert np.array_equal(out[1:1 + 2 * N], np.tile(st[[0, 2]], N))
    # the spare records are sentinels no step result could hold
    assert np.all(case["rec_in"][case["B"]:] < -1e77) and np.array_equal(case["rec_in"][case["B"]:], case["rec_out"][case["B"]:])


def test_cases_cover_rows_slots_and_clip_ends():
    fam_present = set()          # (family, stage) seen with a row in the problem
    fam_absent = set()           # ... and with the row's slot empty (LDCBF rows; the kinematic rows are in every problem)
    below = {3.0: 0, 100.0: 0}; above = {3.0: 0, 100.0: 0}; exact = {3.0: 0, 100.0: 0}
    kinds = set()
    distinct_words = True
    for N, n in W.SHAPES:
        case = W.make_case(N, n)
        for b in range(case["B"]):
            pres, rec, out = case["present"][b], case["rec_in"][b], case["rec_out"][b]
            z_in, z_out = rec[1 + 2 * N:], out[1 + 2 * N:]
            warm = rec[0] == 1.0
            # every word of an input record is distinct, but for the rows deliberately set to 0.0
            nz = rec[1:][rec[1:] != 0.0]
            distinct_words &= len(np.unique(nz)) == len(nz)
            if n:
                kinds.add(("none" if not pres.any() else "all" if pres.all() else "last" if (pres[-1] and pres.sum() == 1)
                           else "hole" if (not pres[n // 2] and pres.sum() == n - 1) else "some", warm))
            for k in range(N):
                for fam, lo, cnt in (("reach", 4 * k, 4), ("man", 4 * N + k, 1), ("vel", 5 * N + 4 * k, 4)):
                    assert np.all(z_out[lo:lo + cnt] >= 3.0) and np.all(z_out[lo:lo + cnt] <= 100.0)
                    fam_present.add((fam, "warm" if warm else "cold"))
            for k in range(N + 1):
                row = z_out[9 * N + k * n: 9 * N + (k + 1) * n]
                if k == 0:
                    assert np.all(row == 0.0)
                else:
                    assert np.all(row[~pres] == 0.0) and np.all(row[pres] >= 3.0)
                for j in range(n):
                    (fam_present if pres[j] else fam_absent).add(("ldcbf", N, k))
                    if not pres[j] and warm:
                        assert z_in[9 * N + k * n + j] != 0.0      # non-zero in the record, empty now: comes back 0.0
            if warm and case["fresh_slot"][b] >= 0:                   # 0.0 in the record, present now: starts at 3.0
                j = case["fresh_slot"][b]
                assert pres[j] and np.all(z_in[9 * N + j + n * np.arange(N + 1)] == 0.0)
                assert np.all(z_out[9 * N + j + n * np.arange(1, N + 1)] == 3.0)
                kinds.add("fresh")
            if warm:
                slots = np.flatnonzero(pres)
                src = W.row_sources(N, len(slots))
                z_or_in = W.from_record_rows(z_in, N, slots, n)
                z_or_out = W.from_record_rows(z_out, N, slots, n)
                live = np.ones(len(src), bool); live[9 * N: 9 * N + len(slots)] = False
                v_in, v_out = z_or_in[src][live], z_or_out[live]
                assert np.array_equal(v_out, np.clip(v_in, 3.0, 100.0))
                for end in (3.0, 100.0):
                    below[end] += int(np.sum(v_in == np.nextafter(end, -np.inf)))
                    above[end] += int(np.sum(v_in == np.nextafter(end, np.inf)))
                    exact[end] += int(np.sum(v_in == end))
                # every special value sits in a row the start really reads
                for r, v in case["specials"][b]:
                    assert v in v_in, (N, n, b, r, v)
                assert np.sum(v_in == 1e300) == np.sum(v_out[v_in == 1e300] == 100.0)
    assert distinct_words
    for fam in ("reach", "man", "vel"):
        assert (fam, "warm") in fam_present and (fam, "cold") in fam_present
    for N, n in W.SHAPES:
        if n:
            for k in range(N + 1):      # LDCBF rows of every stage 1..N and the k = 0 rows: with the slot present and with it empty
                assert ("ldcbf", N, k) in fam_present and ("ldcbf", N, k) in fam_absent, (N, k)
    for kind in ("none", "all", "last", "hole"):
        assert (kind, True) in kinds, kind
    assert "fresh" in kinds
    for end in (3.0, 100.0):
        assert below[end] >= 3 and above[end] >= 3 and exact[end] >= 3, (end, below, above, exact)


@pytest.mark.parametrize("N,n", [(2, 3), (4, 14), (8, 10), (16, 4)])
def test_repeated_identity_steps_settle_on_the_last_stage(N, n):
    """After N - 1 shifts every stage holds the last stage's clipped multipliers; the positions have been extrapolated once per
    step.  (What the GPU test of N + 1 launches in a row compares with.)"""
    case = W.make_case(N, n)
    rec = W.expected_after(case, N - 1)
    for b in range(case["B"]):
        if case["rec_in"][b, 0] != 1.0:
            continue
        z_in, z = case["rec_in"][b, 1 + 2 * N:], rec[b, 1 + 2 * N:]
        pres = case["present"][b]
        for k in range(N):
            assert np.array_equal(z[4 * k:4 * k + 4], np.clip(z_in[4 * (N - 1):4 * N], 3.0, 100.0))
            assert z[4 * N + k] == np.clip(z_in[5 * N - 1], 3.0, 100.0)
            assert np.array_equal(z[5 * N + 4 * k:5 * N + 4 * k + 4], np.clip(z_in[9 * N - 4:9 * N], 3.0, 100.0))
            assert np.array_equal(z[9 * N + (k + 1) * n: 9 * N + (k + 2) * n][pres], np.clip(z_in[9 * N + N * n:][pres], 3.0, 100.0))
        q_in = case["rec_in"][b, 1:1 + 2 * N].reshape(N, 2)
        q = rec[b, 1:1 + 2 * N].reshape(N, 2)
        assert np.array_equal(q[0], q_in[N - 1])
        assert np.allclose(q[N - 1], q_in[N - 1] + (N - 1) * (q_in[N - 1] - q_in[N - 2]), rtol=0, atol=1e-12)
    assert not np.array_equal(W.expected_after(case, N + 1)[:, 1:2 * N + 1], rec[:, 1:2 * N + 1])     # positions keep moving


@pytest.mark.parametrize("mutation", W.MUTATIONS)
def test_each_slip_changes_an_expectation_at_every_instantiation(mutation):
    """The GPU comparison is np.array_equal with rec_out: a kernel with one of these slips would leave mutated_record instead,
    and that differs from rec_out in at least one warm problem of every instantiation's case (the slips in the slot stride and
    in the k = 0 rows need slots: every instantiation with row slots)."""
    needs_slots = mutation in ("n_obs_stride", "k0_kept")
    for N, n in W.INSTANTIATION_SHAPES:
        if needs_slots and n == 0:
            continue
        case = W.make_case(N, n)
        caught = [b for b in range(case["B"]) if case["rec_in"][b, 0] == 1.0
                  and not np.array_equal(W.mutated_record(case, b, mutation), case["rec_out"][b])]
        assert caught, (mutation, N, n)
