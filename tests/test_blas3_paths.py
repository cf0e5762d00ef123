"""The case table of tests/blas3_cases.py reaches what it claims (no GPU).

Every row is driven through the product's own object files on the recording stand-in (tests/hipshim/run_blas3.py, one child process for
all rows).  The stand-in's trace carries each launch's device-side kernel name, which separates template instances, and the CPU models log
the run-time modes of the tile-kernel launches.  Two things are asserted:

  * every row launches exactly the instance(s) it names, with split-K and the XCD band mapping where it says so - and the CPU models'
    result equals the exact reference bit for bit with every NaN where it was, which checks the table and the reference helper before a
    GPU sees them (the large-pitch rows: kernel name only, in trace mode, no memory touched);
  * completeness: every registered kernel whose name contains `dgemm_`, `scale_kernel` or `splitk_reduce_kernel` is launched by at
    least one row or listed in NOT_REACHED_FROM_THE_OPERATORS with the reason and the test that covers it - an instance added later
    fails here until someone gives it a row.

The stand-in may classify pointers differently from a device, so the atomic-epilogue flag (a run-time field) is not checked here:
tests/test_gpu_blas3_exact.py covers it through the beta == 1 pairs."""
import json
import os
import subprocess
import sys

import pytest

from tests import blas3_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# registered instances no GEMM / SYRK / TRMM call can launch: why, and where they are tested instead
NOT_REACHED_FROM_THE_OPERATORS = {
    "dgemm_tn_dma_kernel<1,0,0,1,0>": "TAG 1 = the trailing update of the blocked Cholesky (same code, its own name for the profiler): tests/test_gpu_cholinv.py::test_matches_oracle",
    "dgemm_tn_dma_kernel<1,0,0,0,0>": "TAG 1 without buffer-addressed DMA: a factorization plan with a leading dimension beyond 4.19e6 - no test reaches it; the same code "
                                      "as <0,0,0,0,0>, which the large-pitch rows run",
    "dgemm_kernel<1,1,0,0>": "EDGE 0 of the TN form: launch_variant instantiates it, no call launches it - an aligned TN product always takes the LDS-DMA kernel, split-K "
                             "included; no test (nothing can reach it)",
    "dgemm_kernel<1,1,0,1>": "the same under TAG 1 (the trailing update's name): instantiated, never launched; no test (nothing can reach it)",
    "dgemm_kernel<1,1,1,1>": "TAG 1, ragged trailing update of a blocked factorization (n = 1000, 777): tests/test_gpu_cholinv.py::test_matches_oracle",
    "dgemm_kernel<1,1,2,1>": "TAG 1, odd-sized trailing update (n = 777): tests/test_gpu_cholinv.py::test_matches_oracle",
    "dgemm_tn_skinny_kernel<1>": "op(A) stored in fp32 (cap_skinny_f32a_launch, the mixed-precision refinement sweeps): tests/test_gpu_mixed.py::test_substitution_and_one_sweep_against_host_fp64",
    "dgemm_nn_skinny_kernel<1>": "op(A) stored in fp32 (cap_skinny_f32a_launch, the mixed-precision refinement sweeps): tests/test_gpu_mixed.py::test_substitution_and_one_sweep_against_host_fp64",
    "scqr_unscale_kernel": "not a GEMM kernel (the name merely contains `scale_kernel`): the column un-scaling of shifted CholeskyQR3, tests/test_gpu_scqr.py::test_shifted_factor",
}
# (the -1 LDS request of the occupancy-1 trailing updates and the CAP_EXPERIMENTS-only DIAG instance are not instances of their own in a
#  release build: the former is a launch parameter of <1,0,0,1,0>, the latter is not compiled in)

TILE_KERNELS = ("dgemm_kernel", "dgemm_tn_dma_kernel")


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    from capital_amd import build
    build.build(verbose=False)
    out = str(tmp_path_factory.mktemp("blas3") / "paths.json")
    env = dict(os.environ)
    env["SHIM_FILTER"] = ""; env["SHIM_KEEP_TRACE"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hipshim", "run_blas3.py"), out, "--table"], capture_output=True, text=True, timeout=1500, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout)                       # the case -> kernel instance table (pytest -s; a copy is kept as profiles/r11_blas3_paths.txt)
    return json.load(open(out))


@pytest.mark.parametrize("case", T.CASES + T.BIG_CASES, ids=lambda c: c.id)
def test_row_launches_the_instances_it_names(paths, case):
    runs = paths["cases"][case.id]
    assert len(runs) == len(case.ab)
    for r in runs:
        what = "%s alpha=%s beta=%s" % (case.id, r["alpha"], r["beta"])
        assert r["status"] == 0, (what, r["detail"])
        assert r["kernels"] == case.kernels, what
        if "which" in case:               # large pitch: the name is all there is (trace mode)
            assert r["exact"] is None and not r["detail"], (what, r["detail"])
            continue
        tiles = [k for k in case.kernels if k.split("<")[0] in TILE_KERNELS]
        assert len(r["modes"]) == len(tiles), what
        for m in r["modes"]:
            assert (m["ksplit"] > 1) == case.ksplit, (what, m)
            assert (m["stm"], m["stn"]) == (case.band or (m["stm"], m["stm"])), (what, m)
            assert bool(m["etri"]) == (case.op == "syrk"), (what, m)          # square tile spaces under a mask walk the supertile triangle
        assert r["exact"] is True and not r["detail"], (what, r["detail"])


def test_no_kernel_instance_without_a_row(paths):
    registered = set(paths["registered"])
    assert paths["unmodelled"] == 0
    launched = {k for runs in paths["cases"].values() for r in runs for k in r["kernels"]}
    assert launched <= registered, launched - registered
    named = {k for c in T.CASES + T.BIG_CASES for k in c.kernels}
    assert named == launched
    orphans = registered - launched - set(NOT_REACHED_FROM_THE_OPERATORS)
    assert not orphans, "kernel instances no row of tests/blas3_cases.py launches and NOT_REACHED_FROM_THE_OPERATORS does not explain: %s" % sorted(orphans)
    stale = {k for k in NOT_REACHED_FROM_THE_OPERATORS if k not in registered or k in launched}
    assert not stale, "NOT_REACHED_FROM_THE_OPERATORS lists instances that do not exist or that a row does launch: %s" % sorted(stale)
    # the families the table is about are all there
    for base in ("dgemm_small_kernel", "dgemm_tn_skinny_kernel", "dgemm_nn_skinny_kernel", "dgemm_tn_dma_kernel", "dgemm_kernel", "scale_kernel", "splitk_reduce_kernel"):
        assert any(k.split("<")[0] == base for k in launched), base


def test_table_stays_inside_the_exactness_argument():
    """the table's own premises: scalars and sizes inside the exactness argument, distinct ids, every pair list non-empty"""
    ids = [c.id for c in T.CASES + T.BIG_CASES]
    assert len(ids) == len(set(ids))
    for c in T.CASES + T.BIG_CASES:
        assert c.k <= 6000 and c.ab and all(a in T.SCALARS and b in T.SCALARS for a, b in c.ab), c.id
    gemm_tiles = [c for c in T.GEMM_CASES if c.kernels[0].split("<")[0] in TILE_KERNELS]
    assert any((-1.0, 1.0) in c.ab for c in gemm_tiles)                      # the atomic epilogue is among the pairs
    assert T.BIG_LD_LAST % 2 == 0 and 128 * T.BIG_LD_LAST * 8 + T.BIG_K * 8 < 0xfffffff0 <= 128 * T.BIG_LD_FIRST * 8 + T.BIG_K * 8
