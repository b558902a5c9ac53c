"""Warm-start records of the step entry points: ABI and compiled resources (no GPU needed)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import lipmpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_warm_words_and_exports():
    lib = lipmpc._lib.load()
    assert "lipmpc_set_warm_start" in lipmpc._lib.EXPORTS and "lipmpc_warm_words" in lipmpc._lib.EXPORTS
    assert hasattr(lib, "lipmpc_set_warm_start") and hasattr(lib, "lipmpc_warm_words")
    for N, n_obs in ((1, 0), (3, 0), (3, 12), (8, 10), (12, 14), (16, 50)):
        p = lipmpc.LipMpcParams(N=N, n_obs_max=n_obs).to_c()
        assert lib.lipmpc_warm_words(C.byref(p)) == 1 + 2 * N + 9 * N + (N + 1) * n_obs
        assert lib.lipmpc_warm_words(C.byref(p)) == 1 + 2 * N + lib.lipmpc_num_rows(C.byref(p))
    assert lib.lipmpc_warm_words(None) < 0
    assert lib.lipmpc_set_warm_start(None, None, 0) < 0


@pytest.mark.parametrize("g,nl,nv", [(16, 5, 16), (16, 2, 16), (16, 7, 16), (16, 0, 16), (32, 2, 32), (32, 0, 32), (16, 5, 8),
                                     (32, 5, 32), (32, 7, 32)])
def test_warm_step_kernel_resource_report(g, nl, nv):
    """warm_step_kernel compiles without scratch, at one wave per SIMD, with SGPR spills within the bounds of the step
    kernels (test_headline_kernel_resource_report: 120 at 16 lanes, 160 at 32).  The 32-lane objects with 5 and 7 register
    row slots hold none: their body spills to scratch (lipmpc_set_warm_start refuses those handles)."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "humanoid-navigation-using-mpc-ldcbf_amd", "csrc", "lipmpc_inst.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-DINST_G={g}", f"-DINST_NL={nl}",
                        f"-DINST_NV={nv}", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    blk = [b for b in blocks if "warm_step_kernel" in b.split()[0]]
    if g == 32 and nl > 2:
        assert blk == []
        return
    assert len(blk) == 1
    val = lambda b, key: int(re.search(key + r"[^:]*: (\d+)", b).group(1))
    assert val(blk[0], "ScratchSize") == 0 and val(blk[0], "Occupancy") == 1
    assert val(blk[0], "SGPRs Spill") <= (120 if g == 16 else 160), val(blk[0], "SGPRs Spill")
