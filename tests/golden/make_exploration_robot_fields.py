"""Claims from per-robot fields with the walker in the loop, recorded on the CPU (tests/golden/EXPLORATION_ROBOT_FIELDS.md):

    python tests/golden/make_exploration_robot_fields.py [--write]

make_exploration_kept.py's CPU chain of UnknownEnvFleet.run_exploring, unchanged -- the same two scenes (the open field with the four
side-by-side starts, the three rooms), the same six noise seeds, ``recover`` = 6, ``r_claim`` = 15 -- with every replan made by
tests/robot_fields_oracle.py's plan_batch (RobotFieldsFrontierPlanner) and ``max_claims`` = B, once without memory and once with the
keep parameters 6 / 24 / 8.  The chain's two planning hooks are handed the new rule: ``robot fields`` stands where that script's
``assigned`` stands and ``robot fields kept 6/24/8`` where its ``kept 6/24/8`` stands, so everything else in a chain is that script's,
line for line.  The rows are printed beside the rows EXPLORATION_KEPT.md already holds for ``nearest``, ``assigned`` and ``kept 6/24/8``
(read from exploration_kept.npz, not recomputed).  Nothing is asserted in advance and nothing here is a tuned default: the table says
what came out.  --write records the counts as exploration_robot_fields.npz (what tests/test_robot_fields_fleet_gpu.py takes its
coverage bar from) and the table as EXPLORATION_ROBOT_FIELDS.md.
"""
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_exploration_kept as EK  # noqa: E402
import robot_fields_oracle as RF  # noqa: E402

KEEP = EK.KEEPS[0]
assert KEEP == (6, 24, 8) and EK.MAX_RECOVER == 6 and EK.R_CLAIM == 15
RULES = {"robot fields": "assigned", "robot fields kept 6/24/8": "kept 6/24/8"}      # the new rule -> the hook of the chain it takes
BESIDE = ("nearest", "assigned", "kept 6/24/8")                                       # the recorded rows shown beside the new ones


class _Memoryless:
    """What the chain calls as tests/assign_oracle.py: the new rule, every robot allowed a claim."""

    @staticmethod
    def plan_batch(ev, t_free, t_occ, origin, cell, start, r_claim, max_claims, r_inflate, min_unknown, max_seg, S_max, may_claim=None):
        return RF.plan_batch(ev, t_free, t_occ, origin, cell, start, r_claim, len(start), None, (0, 16, 0), r_inflate, min_unknown, max_seg,
                             S_max, may_claim)


class _Keeping:
    """What the chain calls as tests/assign_keep_oracle.py: the new rule with the previous targets."""

    @staticmethod
    def plan_batch(ev, t_free, t_occ, origin, cell, start, r_claim, prev, r_keep, keep_ratio16, keep_slack, max_claims, r_inflate,
                   min_unknown, max_seg, S_max, may_claim=None):
        return RF.plan_batch(ev, t_free, t_occ, origin, cell, start, r_claim, len(start), prev, (r_keep, keep_ratio16, keep_slack), r_inflate,
                             min_unknown, max_seg, S_max, may_claim)


def chain(args):
    scene, rule, seed = args
    EK.AS, EK.AK = _Memoryless, _Keeping                       # (in this worker process alone)
    return dict(EK.chain((scene, RULES[rule], seed)), rule=rule)


def markdown(rows):
    k = np.load(os.path.join(HERE, "exploration_kept.npz"))
    old_rules = k["rules"].tolist()
    out = ["# Claims from per-robot fields with the walker in the loop", "",
           "Written by `tests/golden/make_exploration_robot_fields.py --write`; the rule is stated in `include/lipmpc.h`",
           "(`lipmpc_grid_frontier_assign_robot_fields_batch`) and restated in `tests/robot_fields_oracle.py`; the argument for it is in DESIGN.md §24.",
           "", f"One CPU chain of `UnknownEnvFleet.run_exploring` per scene, rule and noise seed, `recover` = {EK.MAX_RECOVER}, `r_claim` = {EK.R_CLAIM},",
           "`max_claims` = B for the new rule.  `robot fields` = `RobotFieldsFrontierPlanner(r_claim, B)`, `robot fields kept 6/24/8` = the same with",
           "`r_keep=6, keep_ratio16=24, keep_slack=8`.  The columns are those of `EXPLORATION_KEPT.md`; the rows of `nearest`, `assigned` and",
           "`kept 6/24/8` are copied from its record (`exploration_kept.npz`), the same scenes, starts, seeds and noise.", ""]
    for scene, sc in EK.SCENES.items():
        out += [f"## {scene}: {len(sc['starts'])} robots, `k_max` = {sc['k_max']}, `split_rays` = {sc['split']}", "",
                "| rule | finished (of 6) | finishing samples | failed solves | capture steps | jumps | keeps | claims | lost | least coverage |",
                "|---|---|---|---|---|---|---|---|---|---|"]
        for rule in BESIDE:
            r = old_rules.index(rule)
            col = lambda key: k[f"{scene}/{key}"][r]
            out.append(f"| {rule} (recorded) | {int((col('finished_at') >= 0).sum())} | {col('finished_at').tolist()} | {int(col('n_failed_solves').sum())} | "
                       f"{int(col('n_recover').sum())} | {int(col('n_jumps').sum())} | {int(col('n_kept').sum())} | {int(col('n_claims').sum())} | "
                       f"{int(col('n_failed').sum())} | {float(col('coverage').min()):.4f} |")
        for rule in RULES:
            rs = EK.rows_of(rows, scene, rule)
            out.append(f"| {rule} | {sum(x['finished'] for x in rs)} | {[x['finished_at'] for x in rs]} | {sum(x['n_failed_solves'] for x in rs)} | "
                       f"{sum(x['n_recover'] for x in rs)} | {sum(x['n_jumps'] for x in rs)} | {sum(x['n_kept'] for x in rs)} | "
                       f"{sum(x['n_claims'] for x in rs)} | {sum(x['n_failed'] for x in rs)} | {min(x['coverage'] for x in rs):.4f} |")
        out.append("")
    out += ["Six seeds of two scenes are what was run; nothing here is a tuned default, and no test asserts \"sooner\".", ""]
    return "\n".join(out)


def main():
    jobs = [(sc, r, s) for sc in EK.SCENES for r in RULES for s in EK.SEEDS]
    with Pool(min(12, os.cpu_count() or 1)) as pool:
        rows = pool.map(chain, jobs, chunksize=1)
    text = markdown(rows)
    print(text)
    if "--write" in sys.argv:
        rec = {"seeds": np.array(EK.SEEDS), "keep": np.array(KEEP), "max_recover": EK.MAX_RECOVER, "r_claim": EK.R_CLAIM, "rules": np.array(list(RULES))}
        for scene in EK.SCENES:
            for key in EK.COUNTS + ("coverage",):
                rec[f"{scene}/{key}"] = np.array([[x[key] for x in EK.rows_of(rows, scene, rule)] for rule in RULES])
        np.savez(os.path.join(HERE, "exploration_robot_fields.npz"), **rec)
        with open(os.path.join(HERE, "EXPLORATION_ROBOT_FIELDS.md"), "w") as f:
            f.write(text)
        print("recorded", list(EK.SEEDS))


if __name__ == "__main__":
    main()
