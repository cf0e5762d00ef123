"""CPU-only: the tables of tests/gemm_batched_cases.py are what the GPU tests assume - the exactness premise holds for every block of every
row (fixed size and plan), both kernel paths and every trans pair have rows, the shapes the issue names are there, and every row is
predicted to launch once (once per occurring size class for `combine`)."""
import numpy as np
import pytest

from tests import gemm_batched_cases as GC
from tests import trsm_batched_cases as TC
from tests import vbatched_cases as VC


@pytest.mark.parametrize("row", GC.exact_rows(), ids=GC.row_id)
def test_the_exactness_premise_holds_for_every_block_of_a_row(row):
    m, n, k, batch, ta, tb, (alpha, beta) = row[:7]
    for idx in range(min(batch, GC.DISTINCT)):
        A, B, C = GC.operands(m, n, k, idx)
        assert A.shape == (m, k) and B.shape == (k, n) and C.shape == (m, n)
        assert GC.premise_holds(A, B, C, alpha, beta), GC.premise(A, B, C, alpha, beta)
        E = GC.expected(A, B, C, alpha, beta)
        assert np.array_equal(2.0 * E, np.round(2.0 * E)) and np.abs(E).max(initial=0.0) < GC.LIMIT
        # any order: the reversed sum and the float128 sum agree with NumPy's
        R = alpha * (A[:, ::-1] @ B[::-1, :]) + (beta * C if beta != 0.0 else 0.0)
        assert np.array_equal(R + 0.0, E)


@pytest.mark.parametrize("row", GC.plan_rows(), ids=GC.plan_row_id)
def test_the_exactness_premise_holds_for_every_block_of_a_plan_row(row):
    entry, name, kind, (a, b), (alpha, beta) = row
    sizes = GC.PLAN_LISTS[name]
    ops = GC.plan_operands(entry, name, a, b)
    assert len(ops) == len(sizes)
    for n, (A, B, C) in zip(sizes, ops):
        assert A.shape == ((a, n) if entry == "inner" else (n, b)) and C.shape == ((a, b) if entry == "inner" else (n, a))
        assert GC.premise_holds(A, B, C, alpha, beta)


def test_both_paths_every_trans_pair_and_the_named_shapes_have_rows():
    rows = GC.exact_rows()
    shapes = [(r[0], r[1]) for r in rows]
    assert len(set(shapes)) == len(shapes)
    for r in GC.RECTANGLES:
        assert r in shapes
    for n in TC.WAVE_N + TC.GROUP_N:
        assert (n, n) in shapes
        assert any(m == n and c != n for m, c in shapes)
    for path in ("wave", "group"):
        mine = [r for r in rows if GC.path(r[0], r[1]) == path]
        assert {(r[4], r[5]) for r in mine} == set(GC.TRANS_PAIRS), path
        assert {r[2] for r in mine} == set(GC.KS), path
        assert any(r[6][1] == 0.0 for r in mine) and any(r[6][1] != 0.0 for r in mine) and any(r[6][0] == 0.0 for r in mine)
        assert {r[9] for r in mine} == set(GC.LAYOUTS) and {r[7] for r in mine} == set(GC.LAYOUTS) and {r[8] for r in mine} == set(GC.LAYOUTS)
    assert {r[3] for r in rows} == set(GC.BATCHES)
    assert all(r[3] <= 3 for r in rows if max(r[0], r[1]) > 80)
    assert any(r[0] <= 64 < r[1] for r in rows) and any(r[1] <= 64 < r[0] for r in rows)       # pairs that straddle the two paths
    assert all(0 < r[0] <= GC.MAX_DIM and 0 < r[1] <= GC.MAX_DIM for r in rows)


def test_the_plan_rows_cover_the_lists_and_the_shape_pairs():
    rows = GC.plan_rows()
    assert set(GC.PLAN_LISTS) == {"EVERY", "WAVES", "JACOBI", "EMPTIES", "LONE256"}
    assert GC.PLAN_LISTS["EVERY"] is VC.EVERY and GC.PLAN_LISTS["WAVES"] is VC.WAVES
    assert 0 in GC.PLAN_LISTS["EMPTIES"] and GC.PLAN_LISTS["LONE256"] == (256,)
    jac = GC.PLAN_LISTS["JACOBI"]
    assert sum(n <= 16 for n in jac) > len(jac) // 2 and any(100 <= n <= 200 for n in jac) and all(n <= 16 or 100 <= n <= 200 for n in jac)
    for name in GC.PLAN_LISTS:
        assert {r[3] for r in rows if r[0] == "inner" and r[1] == name} == set(GC.INNER_PQ)
        assert {r[3] for r in rows if r[0] == "combine" and r[1] == name} == set(GC.COMBINE_NK)
    assert {r[2] for r in rows} == set(VC.LAYOUTS)


def test_every_row_is_predicted_to_launch_once():
    assert all(GC.launches(r) == 1 for r in GC.exact_rows())
    for r in GC.plan_rows():
        sizes = GC.PLAN_LISTS[r[1]]
        if r[0] == "inner":
            assert GC.plan_launches(r) == 1, r                       # whatever the classes, empty blocks included
        else:
            want = sum(1 for l in VC.expected_lists(sizes) if l)
            assert GC.plan_launches(r) == want and 1 <= want <= 7, r
    assert GC.plan_launches(("combine", "EVERY", "packed", (3, 0), (1.0, 0.0))) == 7
    assert GC.plan_launches(("combine", "LONE256", "packed", (1, 1), (1.0, 0.0))) == 1
