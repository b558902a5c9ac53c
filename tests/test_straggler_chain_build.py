"""Build figures of the headline kernel after the listing-led pass over the slowest wave's chain (no GPU needed): the pivot
test of the factorisation is a running minimum, the finish round takes its extrema without canonicalising moves, and the
group minima / maxima cross four lanes with one rotation."""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "_ZN10lipmpc_dev16plan_step_kernelILi16ELi5ELi16ELb1"          # plan_step_kernel<16, 5, 16, true>
CANON = re.compile(r"\s+v_max_f64(?:_e64)? (v\[\d+:\d+\]), (v\[\d+:\d+\]), \2\s*$")     # v_max_f64 d, x, x


def _loops(listing, prefix):
    """Instruction lines per depth-1 loop of the function whose symbol starts with ``prefix``, keyed by the header block,
    the way tools/loop_hist.py attributes them; and whether the header is an innermost loop's."""
    lines = listing.split("\n")
    start = [i for i, l in enumerate(lines) if l.startswith(prefix)][0]
    end = [i for i, l in enumerate(lines) if l.startswith(".Lfunc_end") and i > start][0]
    cur, loops, inner = None, collections.defaultdict(list), {}
    for l in lines[start:end]:
        m = re.match(r"\.LBB\d+_(\d+):\s*;\s*(.*)", l)
        if m:
            c = m.group(2)
            h = re.search(r"Header=BB\d+_(\d+) Depth=1", c)
            if "Loop Header: Depth=1" in c:
                cur = m.group(1)
                inner[cur] = "Inner Loop Header" in c
            elif h:
                cur = h.group(1)
            elif "Parent Loop BB" in c:
                cur = re.search(r"Parent Loop BB\d+_(\d+)", c).group(1)
            else:
                cur = None
            continue
        if re.match(r"\.LBB", l):
            cur = None if "Loop" not in l else cur
            continue
        if cur and re.match(r"\s+[a-z]", l) and not l.strip().startswith("."):
            loops[cur].append(l)
    return loops, inner


def test_headline_chain_figures(tmp_path):
    """plan_step_kernel<16, 5, 16, true>: the interior-point loops (innermost loops of more than 1000 instructions: 5-, 2-
    and 1-slot bodies) and the finish loops (the other loops of more than 1000 instructions, same order).

      * interior point: one v_min_f64 per elimination step after the first (15) and no more than 12 s_or_b64 per loop -- the
        parent had a v_cmp_nlt_f64 and an s_or_b64 per step, 23 s_or_b64 in all;
      * finish: at most 4 canonicalising moves (v_max_f64 d, x, x) per round -- the parent had 33 / 24 / 21;
      * no loop longer than the parent's 1534 / 1258 / 1197 and 1879 / 1506 / 1426 instructions;
      * no scratch, and no more SGPR spills than the parent's 86.

    This listing has 1527 / 1219 / 1170 and 1703 / 1419 / 1330 instructions, 9 s_or_b64 per interior-point loop, 58 SGPR
    spills, no scratch."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "humanoid-navigation-using-mpc-ldcbf_amd", "csrc", "lipmpc_inst.hip")
    out = tmp_path / "inst_16_5.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-DINST_G=16", "-DINST_NL=5", "-DINST_NV=16", "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(out)],
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    loops, inner = _loops(out.read_text(), HEADLINE)
    big = [k for k, v in loops.items() if len(v) > 1000]
    ipm, fin = [k for k in big if inner.get(k)], [k for k in big if not inner.get(k)]
    assert len(ipm) == 3 and len(fin) == 3, {k: (len(loops[k]), inner.get(k)) for k in big}
    ops = lambda k: collections.Counter(re.sub(r"_e32$|_e64$", "", l.split()[0]) for l in loops[k])
    for k, cap in zip(ipm, (1534, 1258, 1197)):
        n = ops(k)
        print(f"interior-point loop BB_{k}: {len(loops[k])} instructions, {n['v_min_f64']} v_min_f64, {n['s_or_b64']} s_or_b64")
        assert len(loops[k]) <= cap, (k, len(loops[k]))
        assert n["v_min_f64"] == 15 and n["s_or_b64"] <= 12, (k, n["v_min_f64"], n["s_or_b64"])
    for k, cap in zip(fin, (1879, 1506, 1426)):
        canon = sum(1 for l in loops[k] if CANON.match(l))
        print(f"finish loop BB_{k}: {len(loops[k])} instructions, {canon} canonicalising moves")
        assert len(loops[k]) <= cap, (k, len(loops[k]))
        assert canon <= 4, (k, canon)
    blk = [b for b in re.split(r"remark: Function Name: ", r.stderr)[1:] if b.split()[0].startswith(HEADLINE)]
    assert len(blk) == 1
    val = lambda key: int(re.search(key + r"[^:]*: (\d+)", blk[0]).group(1))
    assert val("ScratchSize") == 0
    assert val("SGPRs Spill") <= 86, val("SGPRs Spill")
