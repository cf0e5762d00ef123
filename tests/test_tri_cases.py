"""The case table of tests/tri_cases.py reaches what it claims, and its exact references are exact (no GPU).

Every row is driven through the product's own object files on the recording stand-in (tests/hipshim/run_tri.py, one child process for
all rows).  TRTRI, TRSM and POTRI rows run in compute mode: the CPU models of leaf_trtri_kernel, copy_window_kernel, dlauum_nt_kernel and
the GEMM kernels must reproduce the exact reference bit for bit with all-NaN scratch, which checks the table, the reference helpers and
the host side's pointers before a GPU sees them.  POTRS rows run in trace mode (kernel names and grids; potrs_subst_kernel has no CPU
model).  Asserted:

  * every row launches exactly what it names: the leaf launches rec_trtri's partition gives, the right potrs_subst_kernel<NR> four times
    (two substitutions, each with its recovery launch of one workgroup), dlauum_nt_kernel where a whole tile exists, and the number of
    GEMM and scaling launches of its route;
  * completeness: every registered kernel whose name contains leaf_trtri_kernel, potrs_subst_kernel or potrs_nan_kernel is launched by
    some row or listed in NOT_REACHED with the reason and the test that covers it;
  * the exactness premise of tests/tri_cases.py holds for every row;
  * the reference helpers are right: at n <= 40 every reference equals the same quantity computed with fractions.Fraction."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import tri_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NOT_REACHED = {
    "potrs_nan_kernel": "launched only when a plan hands its pivot report `info` to the blocked route (cap_cholinv_solve after a failed factor); cap_dpotrs "
                        "passes none: tests/test_gpu_cholinv_solve.py::test_not_spd_gives_nan_and_no_error",
}


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    from capital_amd import build
    build.build(verbose=False)
    out = str(tmp_path_factory.mktemp("tri") / "paths.json")
    env = dict(os.environ)
    env["SHIM_FILTER"] = ""; env["SHIM_KEEP_TRACE"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hipshim", "run_tri.py"), out, "--table"], capture_output=True, text=True, timeout=1500, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout)                       # the row -> kernel table (pytest -s; a copy is kept in profiles/r16_tri_exact.txt)
    return json.load(open(out))


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_row_launches_what_it_names(paths, case):
    r = paths["cases"][case.id]
    assert r["status"] == 0, (case.id, r["detail"])
    assert r["kernels"] == case.kernels, case.id
    assert (r["gemms"], r["scales"]) == (case.gemms, case.scales), case.id
    assert not r["detail"], (case.id, r["detail"])
    if case.op == "potrs":
        assert r["exact"] is None                                # trace mode
        if case.other <= 16:
            nb = len(T.blocks(case.n, T.POTRS_BLOCK))
            items = nb * (nb + 1) // 2
            g = r["grids"][-4:]
            assert g[1] == 1 and g[3] == 1 and g[0] == g[2] and 1 <= g[0] <= items, (case.id, g)      # each substitution, then its recovery launch
    else:
        assert r["exact"] is True, (case.id, r["detail"])


def test_no_kernel_instance_without_a_row(paths):
    registered = set(paths["registered"])
    assert paths["unmodelled"] == 0
    launched = {k for r in paths["cases"].values() for k in r["kernels"]}
    named = {k for c in T.CASES for k in c.kernels}
    assert named == launched
    listed = {k for k in launched if any(w in k for w in ("leaf_trtri_kernel", "potrs_subst_kernel", "potrs_nan_kernel"))}
    assert listed <= registered, listed - registered
    orphans = registered - launched - set(NOT_REACHED)
    assert not orphans, "kernel instances no row of tests/tri_cases.py launches and NOT_REACHED does not explain: %s" % sorted(orphans)
    stale = {k for k in NOT_REACHED if k not in registered or k in launched}
    assert not stale, "NOT_REACHED lists instances that do not exist or that a row does launch: %s" % sorted(stale)
    for k in [T.LEAF, T.LAUUM] + [T.SUBST(nr) for nr in (1, 2, 4, 8, 16)]:
        assert k in launched, k


def test_refusals_launch_nothing_and_touch_nothing(paths):
    assert len(paths["refusals"]) == len(T.REFUSALS)
    for r in paths["refusals"]:
        assert r["status"] == r["want"] and r["launches"] == 0 and r["untouched"] and not r["detail"], r


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_exactness_premise(case):
    for name, v in T.check_premise(case).items():
        assert v < 2.0 ** 53, (case.id, name, v)


def test_table_covers_the_paths_it_is_about():
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids))
    # leaf paddings 16 / 32 / 64, pick_split's three regimes
    assert {T.leaf_padding(s) for c in T.TRTRI_CASES for s in T.leaf_sizes(c.n)} == {16, 32, 64}
    splits = {(n, T.pick_split(n)) for n in T.TRTRI_N if n > T.LEAF_MAX}
    assert any(n < 512 and h % 64 == 0 for n, h in splits) and any(n >= 512 and h % 128 == 0 for n, h in splits)
    assert T.pick_split(65) == 64 and T.pick_split(127) == 64 and T.pick_split(100) == 64 and (100, 64) in splits        # the min(leaf, n - 1) fallback: h = 0 below 128
    assert {c.pads[0] for c in T.TRTRI_CASES} == {0, 2, 3}
    # TRSM: every block width, one block / whole blocks / ragged last blocks of 1, 44 and 128, every form, every alpha, even and odd pitches
    widths = {T.trsm_block(c.n) for c in T.TRSM_CASES}
    assert widths >= {2, 8, 100, 128, 256, 512}
    ragged = {T.blocks(c.n, T.trsm_block(c.n))[-1] for c in T.TRSM_CASES if len(T.blocks(c.n, T.trsm_block(c.n))) > 1}
    assert ragged >= {1, 44, 128, 256, 512}
    for form in T.TRSM_FORMS:
        rows = [c for c in T.TRSM_CASES if c.form == form]
        assert {c.alpha for c in rows} == set(T.ALPHAS) and {c.other for c in rows} == set(T.TRSM_OTHER), form
    assert {(T.lds(c)["T"] % 2, T.lds(c)["B"] % 2) for c in T.TRSM_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # POTRS: every right-hand-side count at the three sizes, every NR instance, more items than any device has workgroups, the blocked widths
    for n in T.POTRS_ALL_NRHS_N:
        assert {c.other for c in T.POTRS_CASES if c.n == n} >= set(T.POTRS_NRHS)
    assert {c.n for c in T.POTRS_CASES if c.other <= 16} == set(T.POTRS_N)
    assert {(c.n, c.other) for c in T.POTRS_CASES if c.other > 16} == {(n, r) for n, _ in T.POTRS_BLOCKED for r in T.POTRS_BLOCKED_NRHS}
    assert all(T.trsm_block(n) == tb for n, tb in T.POTRS_BLOCKED)
    assert T.RECOVERY_CASE.kernels[-1] == T.SUBST(8) and T.AGREEMENT_CASE.other <= 16
    # POTRI: even and odd lda at every size
    for n in T.POTRI_N:
        assert {T.lds(c)["T"] % 2 for c in T.POTRI_CASES if c.n == n and not c.woff} == {0, 1}


def test_families_have_the_stated_structure():
    for n in (129, 1153):
        T_, Tinv, N, d = T.family("F1", n, False)
        assert np.all(d > 0) and set(np.unique(d)) <= set(T.DIAG) and set(np.unique(N)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        for tile_of in (T_, Tinv):            # a third of every off-diagonal 16 x 16 tile is nonzero, the one-column last tiles included
            for j0 in range(16, n, 16):
                for i0 in range(0, j0, 16):
                    tile = tile_of[i0:i0 + 16, j0:j0 + 16]
                    assert np.count_nonzero(tile) >= tile.size // 6, (n, i0, j0)
    T_, Tinv, _, _ = T.family("F2", 65, True)
    assert np.count_nonzero(np.triu(T_)) == 65 * 66 // 2 and np.count_nonzero(Tinv) == 65 + 64 and np.abs(T_).max() <= 4
    Ti, Tiinv, _, _ = T.family("F2i", 65, True)
    assert np.array_equal(Ti, Tinv) and np.array_equal(Tiinv, T_)
    assert np.any(T.family("F1", 300, True)[3] < 0)


def _frac(a):
    return [[Fraction(float(x)) for x in row] for row in np.asarray(a)]


def _fmul(a, b):
    return [[sum((a[i][k] * b[k][j] for k in range(len(b))), Fraction(0)) for j in range(len(b[0]))] for i in range(len(a))]


def _ft(a):
    return [list(r) for r in zip(*a)]


def _finv_upper(t):
    """inverse of an upper triangular matrix of Fractions by back substitution"""
    n = len(t)
    x = [[Fraction(0)] * n for _ in range(n)]
    for c in range(n):
        for i in range(c, -1, -1):
            s = Fraction(1 if i == c else 0) - sum((t[i][p] * x[p][c] for p in range(i + 1, c + 1)), Fraction(0))
            x[i][c] = s / t[i][i]
    return x


@pytest.mark.parametrize("n", (1, 2, 7, 17, 33, 40))
@pytest.mark.parametrize("fam", ("F1", "F2", "F2i"))
def test_references_against_fractions(fam, n):
    """every reference of the module, recomputed in rational arithmetic from the stored T alone"""
    for signed in (True, False):
        T_, Tinv, _, _ = T.family(fam, n, signed)
        ft = _frac(T_)
        finv = _finv_upper(ft)
        assert _frac(Tinv) == finv
        if fam != "F1":
            continue
        if signed:
            c = T.Case(op="trtri", fam=fam, n=n, other=0, form="", alpha=1.0, pads=(0, 0), woff=0)
            ref = T.reference(c, {"T": T_, "Tinv": Tinv})
            assert _frac(np.triu(np.nan_to_num(ref))) == finv and np.all(np.isnan(ref[np.tril_indices(n, -1)]))
            for form in T.TRSM_FORMS:
                for alpha in T.ALPHAS:
                    c = T.Case(op="trsm", fam=fam, n=n, other=3, form=form, alpha=alpha, pads=(0, 0), woff=0)
                    B = T.rhs(c)
                    ref = T.reference(c, {"T": T_, "Tinv": Tinv, "B": B})
                    op = _ft(finv) if form[1] == "T" else finv
                    want = _fmul(op, _frac(B)) if form[0] == "L" else _fmul(_frac(B), op)
                    assert _frac(ref) == [[Fraction(alpha) * x for x in row] for row in want], (form, alpha)
        else:
            c = T.Case(op="potrs", fam=fam, n=n, other=5, form="", alpha=1.0, pads=(0, 0), woff=0)
            B = T.rhs(c)
            assert _frac(T.reference(c, {"T": T_, "Tinv": Tinv, "B": B})) == _fmul(finv, _fmul(_ft(finv), _frac(B)))
            c = T.Case(op="potri", fam=fam, n=n, other=0, form="", alpha=1.0, pads=(0, 0), woff=0)
            ref = T.reference(c, {"T": T_, "Tinv": Tinv})
            full = _fmul(finv, _ft(finv))
            assert _frac(np.triu(np.nan_to_num(ref))) == [[full[i][j] if i <= j else Fraction(0) for j in range(n)] for i in range(n)]
            assert np.all(np.isnan(ref[np.tril_indices(n, -1)]))
