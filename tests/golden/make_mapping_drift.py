"""Mapping under odometry drift, with and without the scan matcher, as a CPU chain of the committed oracles -> MAPPING_DRIFT.md.

    python tests/golden/make_mapping_drift.py

One robot walks a fixed path of 80 samples through the room of tests/scan_match_cases.py (no solver: the path is given).  Per
sample, as UnknownEnvFleet's drift model does it: the drift grows by a draw of N(0, sigma^2) per axis; the true pose is scanned
(grid scan oracle, readings with N(0, 0.01) noise); the believed pose and readings are true + drift; with the matcher on they are
matched against the evidence so far (tests/scan_match_oracle.py) and the offset is added; the map oracle integrates the believed
scan.  Six seeds, sigma in {0.01, 0.02, 0.04}.  The document records what comes out, also where the matcher does not help.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import map_oracle as M  # noqa: E402
import scan_match_cases as K  # noqa: E402
import scan_match_oracle as S  # noqa: E402

SAMPLES, SEEDS, SIGMAS = 80, range(6), (0.01, 0.02, 0.04)
WAYPOINTS = np.array([(0.75, 0.62), (3.35, 0.95), (4.1, 1.1), (4.1, 2.6), (2.8, 3.2), (0.8, 2.8), (0.6, 1.5), (0.75, 0.62)])
# min_score / min_gain: of (20, 80, 160) x (4, 24, 60) tried on this very chain, the pair whose largest error at sigma 0.02 and 0.04
# was smallest (a scan of 90 rays scores at most 90 * clamp = 720); with (20, 4) the walk was lost (errors above 1.0) in half the runs
MATCH = dict(n_x=4, n_y=4, clamp=8, min_score=160, min_gain=24)
W_HIT, W_MISS = 3, 1


def path():
    seg = np.sqrt((np.diff(WAYPOINTS, axis=0) ** 2).sum(1))
    s = np.linspace(0.0, seg.sum(), SAMPLES, endpoint=False)
    cum = np.concatenate([[0.0], np.cumsum(seg)])
    i = np.minimum(np.searchsorted(cum, s, side="right") - 1, len(seg) - 1)
    t = (s - cum[i]) / seg[i]
    return WAYPOINTS[i] + t[:, None] * (WAYPOINTS[i + 1] - WAYPOINTS[i])


def chain(seed, sigma, matcher):
    rng_noise, rng_drift = np.random.default_rng(1000 + seed), np.random.default_rng(2000 + seed)
    ev = np.zeros((K.W, K.H), np.int64)
    drift, err, accepted = np.zeros(2), [], 0
    for p in path():
        drift = drift + sigma * rng_drift.standard_normal(2)
        hits = K.scan(p[None], 0.01 * rng_noise.standard_normal((1, K.R, 2)))[0]
        bpos, bhits = p + drift, hits + drift
        if matcher:
            m = S.match_one(bpos, bhits, ev, K.ORIGIN, K.CELL, K.RANGE, K.DEPTH, MATCH["n_x"], MATCH["n_y"], MATCH["clamp"], MATCH["min_score"],
                            MATCH["min_gain"])
            off = np.array(m["offset"], float)
            drift, bpos, bhits, accepted = drift + off, bpos + off, bhits + off, accepted + m["matched"]
        M.update(ev, bpos[None], bhits[None], K.ORIGIN, K.CELL, K.RANGE, K.table(), depth=K.DEPTH, w_hit=W_HIT, w_miss=W_MISS)
        err.append(float(np.sqrt((drift * drift).sum())))
    return ev, err, accepted


def classes(ev):
    return np.where(ev >= W_HIT, 1, np.where(ev <= -W_MISS, -1, 0))


def main():
    rows = []
    for sigma in SIGMAS:
        for seed in SEEDS:
            clean = classes(chain(seed, 0.0, False)[0])
            row = [sigma, seed]
            for matcher in (False, True):
                ev, err, accepted = chain(seed, sigma, matcher)
                row += [err[-1], max(err), int((classes(ev) != clean).sum())] + ([accepted] if matcher else [])
            rows.append(row)
            print(row, flush=True)
    lines = ["# Mapping under odometry drift: the scan matcher off and on", "",
             "Written by `tests/golden/make_mapping_drift.py`, a CPU chain of the committed oracles (grid scan, scan matcher, map update):",
             f"one robot on a fixed closed path of {SAMPLES} samples through the 48 x 40 room of `tests/scan_match_cases.py` (cells of 0.1, range 1.5,",
             "90 rays, N(0, 0.01) noise on the readings), its drift a random walk of sigma per sample and axis.  Matcher: "
             f"n = {MATCH['n_x']}, clamp {MATCH['clamp']}, min_score {MATCH['min_score']}, min_gain {MATCH['min_gain']}.",
             "`cells` counts the cells of the final map whose class (occupied: evidence >= 3, free: <= -1, unknown) differs from the map the",
             "same seed builds without drift.  Pose errors in map units (a cell is 0.1).", "",
             "| sigma | seed | final error, off | largest, off | cells, off | final error, on | largest, on | cells, on | accepted offsets |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r[0]} | {r[1]} | {r[2]:.3f} | {r[3]:.3f} | {r[4]} | {r[5]:.3f} | {r[6]:.3f} | {r[7]} | {r[8]} |")
    lines += ["", "## Per sigma (ranges over the six seeds)", "", "| sigma | largest error, off | largest error, on | cells, off | cells, on | seeds where `on` has the smaller largest error |",
              "|---|---|---|---|---|---|"]
    for sigma in SIGMAS:
        rs = [r for r in rows if r[0] == sigma]
        rng = lambda i, f="{:.2f}": f.format(min(r[i] for r in rs)) + " to " + f.format(max(r[i] for r in rs))
        lines.append(f"| {sigma} | {rng(3)} | {rng(6)} | {rng(4, '{}')} | {rng(7, '{}')} | {sum(r[6] < r[3] for r in rs)} of {len(rs)} |")
    lines += ["", "## Reading", "",
              "The thresholds were chosen on this very chain: of min_score in (20, 80, 160) and min_gain in (4, 24, 60) the pair above had the",
              "smallest largest error at sigma 0.02 and 0.04; with (20, 4) the matcher accepted offsets on thin evidence while the robot walked",
              "into parts of the room the map did not hold yet, and lost the pose (largest error above 1.0) in 6 of those 12 runs.  Nobody has",
              "measured the thresholds anywhere else, which is why `ScanMatcher` has no defaults for them.",
              "The matcher corrects in whole cells, so it cannot hold the error below about a cell (0.1); where the drift itself stays near a cell",
              "(sigma 0.01) there is little or nothing to gain, and a wrong acceptance can cost more than it saves.  A pose that sees mostly walls",
              "the map does not hold yet is matched against little evidence: `min_score` and `min_gain` are the only guards there.  Nothing already",
              "written into the map is corrected afterwards, so the `cells` columns include what was smeared before a correction.  No test asserts",
              "that the matcher helps; this document records what it did."]
    with open(os.path.join(HERE, "MAPPING_DRIFT.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
