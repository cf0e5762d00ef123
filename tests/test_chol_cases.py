"""The case table of tests/chol_cases.py reaches what it claims, and its exact references are exact (no GPU).

Every row is driven through the product's own object files on the recording stand-in (tests/hipshim/run_chol.py, one child process for
all rows, compute mode): the CPU models of leaf_cholinv_kernel, panel64_solve_update_kernel, chain64_coop_kernel, trinv_merge_kernel,
copy_window_kernel and the GEMM kernels must reproduce the exact references bit for bit on all-NaN scratch, which checks the table, the
reference helpers and the host side's pointers before a GPU sees them.  Asserted:

  * every row launches exactly what it names: the launches per kernel of the factor's own family, the number of dgemm_* launches, how
    many of them read their C input from A (the fused first-step copy) and how many paired far updates (K = 2 NB) the plan counted -
    all predicted by chol_cases.expected_launches from the row's options alone;
  * completeness: every registered instance of the family is launched by some row (panel64_solve_update_kernel in its folded form with
    many workgroups and in its `direct` form, the last step's single workgroup), every GEMM instance and run-time mode the factor uses
    appears (the tile kernels with and without the atomic tag, the Cin mode, K = 2 NB, the small-matrix kernel of the recursion), and
    every option key of cap_cholinv_set_option that changes the schedule appears in at least one row;
  * the exactness premise of tests/chol_cases.py holds for every row;
  * the reference helpers are right: at n <= 40 R and R^-1 equal a fractions.Fraction Cholesky factor and inverse of the stored A, and
    the empty root block of complete_inv = 0 is where the oracle's recursion leaves it.

Not reached, with the reason: panel64_solve_update_kernel without the folded leaf (only with CAP_FOLD_LEAF=0 in an experiment build, an
A/B switch the release library ignores; the same kernel instance with its Dnext argument NULL) and cap_gemm_small_batched for the merges
(only with CAP_TRINV_MERGE=0 in an experiment build; trinv_merge_kernel<RBW> replaced it)."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import chol_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    from capital_amd import build
    build.build(verbose=False)
    out = str(tmp_path_factory.mktemp("chol") / "paths.json")
    env = dict(os.environ)
    env["SHIM_FILTER"] = ""; env["SHIM_KEEP_TRACE"] = ""
    for k in [k for k in env if k.startswith("CAP_")]:          # (the table describes the defaults)
        del env[k]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hipshim", "run_chol.py"), out, "--table"], capture_output=True, text=True, timeout=1500, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout)                       # the row -> kernel table (pytest -s; a copy is kept in profiles/r19_chol_exact.txt)
    return json.load(open(out))


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_row_launches_what_it_names(paths, case):
    r = paths["cases"][case.id]
    assert r["status"] == 0, (case.id, r["detail"])
    assert r["kernels"] == case.kernels, case.id
    assert (r["gemms"], r["cin"], r["paired"]) == (case.gemms, case.cin, case.k2), case.id
    assert not r["detail"] and r["exact"] is True, (case.id, r["detail"])          # (pivot rows: info == pivot + 1)
    if case.k2:
        kn = T.knobs(case)
        assert 2 * max(kn["nb"], kn["outer"] // kn["nb"] * kn["nb"]) in r["ks"], (case.id, r["ks"])


def test_no_kernel_instance_without_a_row(paths):
    registered = set(paths["registered"])
    assert paths["unmodelled"] == 0
    launched = {k for r in paths["cases"].values() for k in r["kernels"]}
    assert {k for c in T.CASES for k in c.kernels} == launched
    assert registered == launched, "instances of the family without a row (or rows that name none): %s" % sorted(registered ^ launched)
    assert launched == {T.LEAF, T.PANEL, T.CHAIN, T.MERGE(1), T.MERGE(2), T.MERGE(4)}
    # panel64_solve_update_kernel: r (r + 1) / 2 workgroups for r blocks left - every step of a 16-block chain, the `direct` last step included
    grids = {g for r in paths["cases"].values() for g in r["panel_grids"]}
    assert grids == {r * (r + 1) // 2 for r in range(1, 16)}
    # the GEMM instances and modes of the factor
    gemm = {k for r in paths["cases"].values() for k in r["gemm_names"]}
    tiles = {k for k in gemm if k.startswith("dgemm_tn_dma_kernel")}
    assert len(tiles) >= 4 and any(k.startswith("dgemm_kernel<") for k in gemm) and any(k.startswith("dgemm_small_kernel<") for k in gemm), sorted(gemm)
    assert any(r["cin"] > 0 for r in paths["cases"].values()) and any(r["paired"] > 0 and r["cin"] > 0 for r in paths["cases"].values())
    # the atomic-free tag of caller memory (cap_dpotrf) and the atomic form (plans) of the update kernels
    plan_gemm = {k for c in T.CASES if c.entry == "plan" for k in paths["cases"][c.id]["gemm_names"]}
    potrf_gemm = {k for c in T.CASES if c.entry == "dpotrf" for k in paths["cases"][c.id]["gemm_names"]}
    assert potrf_gemm - plan_gemm and plan_gemm - potrf_gemm, (sorted(plan_gemm), sorted(potrf_gemm))


def test_table_covers_the_paths_it_is_about():
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids))
    used = {k for c in T.CASES for k, _ in c.opts}
    assert used == set(T.SCHEDULE_KEYS), used ^ set(T.SCHEDULE_KEYS)
    src = open(os.path.join(ROOT, "capital_amd", "csrc", "cholinv.hip")).read()
    for k in T.SCHEDULE_KEYS:
        assert 'k == "%s"' % k in src, k
    # leaf paddings, both entries, every leaf size
    plan_leaf = [c for c in T.LEAF_CASES if c.entry == "plan"]
    assert {TC_pad(c.n) for c in plan_leaf if c.ci < 0} == {16, 32, 64} == {TC_pad(c.n) for c in T.LEAF_CASES if c.entry == "dpotrf"}
    assert {T.knobs(c)["leaf"] for c in T.LEAF_CASES} == {16, 32, 64}
    # one diagonal block: every width, fastdiag on and off, every G; stepwise and one-launch chain; every merge level
    for nb in (128, 256, 512, 1024):
        rows = [c for c in T.BLOCK_CASES if c.opt.get("nb") == nb and c.n == nb]
        assert {c.opt.get("chain_coop") for c in rows if c.opt["fastdiag"]} == set(T.COOP_G) and any(not c.opt["fastdiag"] for c in rows), nb
        assert any(c.ci == 1 and c.opt.get("nb") == nb and T.CHAIN in c.kernels for c in T.BLOCK_CASES) == (nb >= 256)
        assert any(c.ci == 1 and c.opt.get("nb") == nb and T.PANEL in c.kernels for c in T.BLOCK_CASES)
    assert {c.n for c in T.BLOCK_CASES} >= {65, 100, 130, 200, 300}
    # the sweep: every complete_inv with split 1 and 2, both values of pair_rest on every pairing row, the pair counts of the existing test
    assert {(c.ci, c.split) for c in T.SWEEP_CASES} >= {(ci, s) for ci in (-1, 0, 1) for s in (1, 2)}
    for n, ci, o, _ in T.PAIRED:
        k2 = {c.opt["pair_rest"]: c.k2 for c in T.SWEEP_CASES if c.n == n and c.ci == ci and all(c.opt.get(k) == v for k, v in o.items()) and "pair_rest" in c.opt}
        nstrip = -(-n // o["outer"])
        assert k2[0] == 0 and (k2[1] >= 1 if "tail" in o else k2[1] == max(0, (nstrip - 3) // 2)), (n, o, k2)
    assert {(c.opt["fuse_copy"], c.opt["use_sb"]) for c in T.SWEEP_CASES if c.n == 1024 and "fuse_copy" in c.opt and "use_sb" in c.opt} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c.cin > 0 and c.opt.get("use_sb") == 0 for c in T.SWEEP_CASES) and any(c.cin == 0 and c.opt.get("fuse_copy") == 0 for c in T.SWEEP_CASES)
    # cap_dpotrf: the sizes and pitches; the look-ahead starts at 4096
    assert {c.n for c in T.DPOTRF_CASES} == {1, 64, 65, 129, 640, 1100, 2304, 4096}
    assert {(c.n + c.pad) % 2 for c in T.DPOTRF_CASES} == {0, 1} and {c.pad for c in T.DPOTRF_CASES} == {0, 2, 3}
    assert [T.knobs(c)["lookahead"] for c in T.DPOTRF_CASES if c.n == 4096] == [1] and not any(T.knobs(c)["lookahead"] for c in T.DPOTRF_CASES if c.n < 4096)
    # failing pivots on both chains
    assert {(c.pivot, c.opt["chain_coop"]) for c in T.PIVOT_CASES} == {(r, g) for r in (0, 63, 64, T.PIVOT_NB - 1, T.PIVOT_NB, T.PIVOT_N - 1) for g in (0, 32)}
    assert any(c.second for c in T.REUSE_CASES)


def TC_pad(n):
    return T.TC.leaf_padding(n)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_exactness_premise(case):
    for name, v in T.check_premise(case).items():
        assert v < 2.0 ** 53, (case.id, name, v)


def test_operands_have_the_stated_structure():
    for n, second in ((129, False), (300, True), (1536, True)):
        R, Rinv, N, d = T.factor_pair(n, second)
        assert np.all(d > 0) and set(np.unique(d)) <= {0.5, 1.0, 2.0, 4.0} and set(np.unique(N)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        assert set(np.unique(d * d)) <= set(T.PROBE_PIVOTS)
        assert np.array_equal(R @ Rinv, np.eye(n)) and np.array_equal(R, d[:, None] * (np.eye(n) + N))
        A = T.spd(n, second)
        assert np.array_equal(A, A.T) and np.array_equal(A, R.T @ R)
        if second:
            assert np.array_equal(R, 2.0 * np.diag(d) - T.factor_pair(n)[0]) and not np.array_equal(A, T.spd(n))
    c = T.PIVOT_CASES[0]
    S = T.operand(c)
    assert np.all(np.isnan(S[np.tril_indices(c.n, -1)])) and not np.any(np.isnan(np.triu(S)))


def _frac(a):
    return [[Fraction(float(x)) for x in row] for row in np.asarray(a)]


def _fchol_upper(a):
    """upper Cholesky factor of a symmetric matrix of Fractions whose pivots are squares of rationals; also the pivots"""
    n = len(a)
    r = [[Fraction(0)] * n for _ in range(n)]
    piv = []
    for k in range(n):
        p = a[k][k] - sum((r[q][k] * r[q][k] for q in range(k)), Fraction(0))
        piv.append(p)
        root = Fraction(int(np.sqrt(float(p.numerator))), int(np.sqrt(float(p.denominator)))) if p > 0 else Fraction(0)
        assert p <= 0 or root * root == p, "the pivot is the square of a rational"
        r[k][k] = root
        if p <= 0:
            break
        for j in range(k + 1, n):
            r[k][j] = (a[k][j] - sum((r[q][k] * r[q][j] for q in range(k)), Fraction(0))) / root
    return r, piv


def _finv_upper(t):
    n = len(t)
    x = [[Fraction(0)] * n for _ in range(n)]
    for c in range(n):
        for i in range(c, -1, -1):
            s = Fraction(1 if i == c else 0) - sum((t[i][p] * x[p][c] for p in range(i + 1, c + 1)), Fraction(0))
            x[i][c] = s / t[i][i]
    return x


@pytest.mark.parametrize("second", (False, True))
@pytest.mark.parametrize("n", (1, 2, 7, 17, 33, 40))
def test_references_against_fractions(n, second):
    """R and R^-1 recomputed in rational arithmetic from the stored A alone (its upper triangle); the pivots are d^2; a lowered diagonal
    element makes that pivot exactly -1"""
    from oracle import capital_oracle as orc
    S = T.operand(T.Case(entry="plan", n=n, ci=1, split=1, opts=(), pad=0, second=second, pivot=None), second)
    a = np.triu(np.nan_to_num(S))
    a = a + np.triu(a, 1).T
    r, piv = _fchol_upper(_frac(a))
    assert set(piv) <= {Fraction(v) for v in T.PROBE_PIVOTS}
    R, Rinv = T.references(T.Case(entry="plan", n=n, ci=1, split=1), second)
    assert _frac(R) == r and _frac(Rinv) == _finv_upper(r)
    for ci in (0, 1):
        for split in (1, 2):
            _, ri = T.references(T.Case(entry="plan", n=n, ci=ci, split=split), second)
            _, ri_orc = orc.cholinv(a, ci, split, T.BC, 1, 1)
            assert np.array_equal(ri != 0, np.triu(ri_orc) != 0), (n, ci, split)
    if n > 1 and not second:
        for pivot in (0, n // 2, n - 1):
            Sp = T.operand(T.Case(entry="plan", n=n, ci=1, split=1, opts=(), pad=0, second=False, pivot=pivot))
            ap = np.triu(np.nan_to_num(Sp))
            _, piv = _fchol_upper(_frac(ap + np.triu(ap, 1).T))
            assert len(piv) == pivot + 1 and piv[-1] == -1 and all(p > 0 for p in piv[:-1])


def test_host_model_matches_the_defaults_of_the_library():
    """chol_cases.knobs restates plan_create's and potrf_knobs' defaults: checked against the library where it can be asked without a GPU
    (the work size of cap_dpotrf depends on nb alone)"""
    src = open(os.path.join(ROOT, "capital_amd", "csrc", "cholinv.hip")).read()
    assert "int64_t nb = n >= 8192 ? 512 : 256;" in src and "p.lookahead = n >= 4096;" in src and "p->depth2 = n >= 24576;" in src
    assert T.default_nb(1536) == 256 and T.default_nb(640) == 128 and T.default_nb(300) == 128 and T.default_nb(4096) == 256
    assert not T.root_is_base(2, 1) and T.root_is_base(1, 1) and T.root_is_base(3, 2) and not T.root_is_base(1536, 2)
