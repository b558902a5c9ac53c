"""CPU: the inputs of tests/path_wave_cases.py reach what they are for, shown on the numpy oracles -- which sight tests the walks
make (their lengths round the wave width of 64, the index of the first impassable cell, the slopes and the sign of the closed form's
numerators), which snaps, which spacings and slot counts, which batch shapes -- and the read counts of a walk on a large walled map:
serial cell reads of the one-lane walk against load rounds of the wave walk.  No GPU: tests/test_path_wave_gpu.py runs the same
inputs through both path calls."""
import numpy as np
import pytest

import field_oracle as Fo
import path_wave_cases as P


def test_the_replay_is_the_oracles_string_pulling_and_its_closed_form_is_los():
    """``replay`` asserts its sub-goal cells against field_oracle.string_pull; here every recorded test is held against
    field_oracle.los, and the first impassable index against the incremental quotient / remainder walk of the one-lane kernel."""
    def incremental(fld, a, b):
        if tuple(b) < tuple(a):
            a, b = b, a
        di, dj = b[0] - a[0], b[1] - a[1]
        m = max(abs(di), abs(dj))
        qi, ri, qj, rj = 0, m, 0, m
        for k in range(m + 1):
            if fld[a[0] + qi, a[1] + qj] == Fo.INF:
                return k
            ri, rj = ri + 2 * di, rj + 2 * dj
            if ri >= 2 * m:
                ri, qi = ri - 2 * m, qi + 1
            elif ri < 0:
                ri, qi = ri + 2 * m, qi - 1
            if rj >= 2 * m:
                rj, qj = rj - 2 * m, qj + 1
            elif rj < 0:
                rj, qj = rj + 2 * m, qj - 1
        return None

    for id_ in ("sight_lengths", "snaps", "seg35_fit"):
        c, want = P.case(id_), P.oracle(id_, "field")
        for b, cells in enumerate(want["cells"]):
            if not cells:
                continue
            fld = want["field"][0 if len(want["field"]) == 1 else b]
            for t in P.replay(fld, cells, c["max_seg"])[1]:
                assert (t["blocked"] is None) == Fo.los(fld, t["a"], t["b"])
                assert t["blocked"] == incremental(fld, t["a"], t["b"])
                # the wave kernel's exact floor of a numerator that may be negative: floor((m + 2k (dj + m)) / (2m)) - k
                m, dj = t["m"], t["dj"]
                assert all((m + 2 * k * (dj + m)) // (2 * m) - k == (2 * k * dj + m) // (2 * m) for k in range(m + 1) if m)


def test_sight_lengths_round_the_wave_width():
    """Tests that pass with exactly 63, 64, 65, 128 and 129 cells; tests that fail with the first impassable cell at segment index
    1, 62, 63, 64, 65 and 127; on maps of about a thousand cells."""
    c = P.case("sight_lengths")
    assert c["occ"].shape == (len(P.JOGS), 4, P.JOG_H) and 4 * P.JOG_H < 4096
    tests = P.tests_of("sight_lengths")
    passed = {t["cells"] for t in tests if t["blocked"] is None}
    failed = {t["blocked"] for t in tests if t["blocked"] is not None}
    print("cells of the tests that pass:", min(passed), "..", max(passed), "; first impassable index of those that fail:", sorted(failed))
    assert {63, 64, 65, 128, 129} <= passed
    assert {1, 62, 63, 64, 65, 127} <= failed
    want = P.oracle("sight_lengths", "field")
    assert (want["status"] == Fo.FOUND).all() and (want["n_sub"] >= 2).all()


def test_slopes_and_orders():
    """Over the ring of starts the tests include dj < 0 after the swap, |dj| > di, di > |dj|, axial and diagonal segments, and
    segments whose closed form meets a negative numerator."""
    c = P.case("slopes")
    assert c["occ"].shape == (P.ROOM, P.ROOM) and 200 <= len(c["start"]) <= 400
    tests = [t for t in P.tests_of("slopes") if t["m"]]
    assert all(t["di"] >= 0 and t["blocked"] is None for t in tests)
    kinds = dict(negative_dj=sum(t["dj"] < 0 for t in tests), steep=sum(abs(t["dj"]) > t["di"] > 0 for t in tests),
                 shallow=sum(t["di"] > abs(t["dj"]) > 0 for t in tests), along_i=sum(t["dj"] == 0 for t in tests),
                 along_j=sum(t["di"] == 0 for t in tests), diagonal_down=sum(t["di"] == t["dj"] for t in tests),
                 diagonal_up=sum(t["di"] == -t["dj"] for t in tests), negative_numerator=sum(t["negative"] for t in tests))
    print(len(c["start"]), "starts,", len(tests), "tests:", kinds)
    assert all(v > 0 for v in kinds.values()), kinds
    assert (P.oracle("slopes", "field")["status"] == Fo.FOUND).all()


@pytest.mark.parametrize("max_seg", P.SPACINGS)
def test_spacing_and_slots(max_seg):
    name = f"seg{'_none' if max_seg is None else max_seg}"
    counts = {}
    for kind in ("field", "frontier"):
        fit, less, one = (P.oracle(f"{name}_{s}", kind) for s in ("fit", "one_less", "one"))
        n = P.s_max(P.case(f"{name}_fit"), kind)
        counts[kind] = n
        assert n >= 2 and fit["n_sub"].max() == n and not (fit["status"] == Fo.PATH_OVERFLOW).any()
        longest = fit["n_sub"] == n
        assert (less["status"][longest] == Fo.PATH_OVERFLOW).all() and (less["n_sub"][longest] == 0).all()
        assert np.array_equal(less["path_cost"][longest], fit["path_cost"][longest])           # overflow: the cost is still written
        assert (less["status"][~longest] == fit["status"][~longest]).all()
        assert (one["status"][fit["n_sub"] > 1] == Fo.PATH_OVERFLOW).all() and (one["status"] == Fo.FOUND).any()
    print(name, "most sub-goals", counts)
    if max_seg == 5:
        assert min(counts.values()) > P.WAVE                   # more sub-goals than a wave has lanes


def test_snaps():
    c, want = P.case("snaps"), P.oracle("snaps", "field")
    fld, H = want["field"][0], c["occ"].shape[1]
    # the tie: both cells are finite, equal in (d^2, field), and the least of the window; the lower index wins
    a, b = P.TIE
    d2 = lambda q, s: (q[0] - s[0]) ** 2 + (q[1] - s[1]) ** 2
    assert fld[P.TIE_START] == Fo.INF and fld[a] == fld[b] != Fo.INF and d2(a, P.TIE_START) == d2(b, P.TIE_START)
    window = [(i, j) for i in range(P.TIE_START[0] - 2, P.TIE_START[0] + 3) for j in range(P.TIE_START[1] - 2, P.TIE_START[1] + 3)]
    keys = sorted((d2(q, P.TIE_START), int(fld[q]), q[0] * H + q[1]) for q in window if fld[q] != Fo.INF)
    assert keys[0][:2] == keys[1][:2] and want["snapped"][0] == a == min(a, b)
    # the corner: the window is clipped on two sides
    for b_ in (1, 2):
        s = Fo.cell_of(c["start"][b_], P.ORIGIN, P.CELL, *c["occ"].shape)
        assert fld[s] == Fo.INF and min(s) - 2 < 0 and want["status"][b_] == Fo.FOUND and want["snapped"][b_] != s
    # the pocket: no finite cell in the window
    assert c["occ"][P.POCKET] == 0 and want["status"][3] == Fo.NO_PATH and want["snapped"][3] is None
    assert want["status"][4] == Fo.FOUND
    # r_inflate 16: a window of 35 x 35 cells, more than 19 chunks of 64
    w, wide = P.case("wide_snap"), P.oracle("wide_snap", "field")
    assert w["r"] == 16 and (2 * (w["r"] + 1) + 1) ** 2 > 19 * P.WAVE
    snapped = 0
    for b_, p in enumerate(w["start"]):
        s = Fo.cell_of(p, P.ORIGIN, P.CELL, *w["occ"].shape)
        if wide["field"][0][s] == Fo.INF:
            assert wide["status"][b_] == Fo.FOUND and wide["snapped"][b_] != s
            assert min(s[0] - 17, s[1] - 17) >= 0 and s[0] + 17 < 64 and s[1] + 17 < 128          # the whole window is inside the map
            snapped += 1
    assert snapped >= 4


def test_batch_shapes():
    """B = 1, 3, 5, 65, 257 -- no multiple of the four robots of a workgroup, one workgroup and many -- with one shared field (F = 1)
    and with a map, a field and a layer per robot (F = B)."""
    assert P.BATCHES == (1, 3, 5, 65, 257) and all(B % 4 for B in P.BATCHES)
    for B in P.BATCHES:
        for per_robot in (False, True):
            id_ = f"batch{B}_{'per_robot' if per_robot else 'shared'}"
            c = P.case(id_)
            assert len(c["start"]) == B and c["occ"].shape == ((B,) if per_robot else ()) + (P.BATCH_W, P.BATCH_H) == c["cost"].shape
            assert len(c["goal"]) == (B if per_robot else 1)
            for kind in ("field", "frontier"):
                for weighted in (False, True):
                    want = P.oracle(id_, kind, weighted)
                    assert want["status"][0] == Fo.FOUND and len(want["status"]) == B
            if B >= 65:
                plain, soft = P.oracle(id_, "field"), P.oracle(id_, "field", True)
                assert len(set(plain["status"].tolist())) >= 3
                assert any(len(a) != len(b) or not np.array_equal(a, b) for a, b in zip(plain["sub_goals"], soft["sub_goals"]))


def test_read_counts_of_a_walk_on_a_large_walled_map():
    """The derivation behind the wave calls: on 362 x 362 cells with a wall every 60 rows (gaps of four cells at alternating ends,
    r_inflate 1), the one-lane walk's sight tests read a number of cells that is quadratic in the straight stretches, one dependent
    load after the other; the wave walk makes ceil(cells / 64) load rounds per test and one round per descent step.  Counts, not
    times."""
    for side in (200, 362):
        n = P.walled_counts(side)
        serial, wave = n["serial_sight"] + n["serial_descent"], n["wave_sight"] + n["wave_descent"]
        print(f"{side} x {side}: path {n['path']} cells, {n['n_sub']} sub-goals, {n['tests']} sight tests per pass; sight-test loads per pass: "
              f"{n['serial_sight']} cell reads serial, {n['wave_sight']} rounds by waves; descent loads per pass: up to {n['serial_descent']} "
              f"reads serial, {n['wave_descent']} rounds by waves; dependent steps of two passes: {2 * serial} reads serial, "
              f"{2 * wave} rounds by waves")
        assert n["tests"] >= n["path"] - 1 and n["wave_sight"] >= n["tests"]
        if side == 362:
            assert n["path"] > 1500 and n["serial_sight"] > 30 * n["wave_sight"] and serial > 30 * wave
