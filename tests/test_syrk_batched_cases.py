"""CPU-only: the exact operands of tests/syrk_batched_cases.py are what they claim to be - the exactness premise per row, the expected
results independent of the summation order, the rows covering every size, k, batch, layout and every (path, trans, fill, beta == 0,
shift) combination the GPU tests name."""
import itertools

import numpy as np
import pytest

from tests import syrk_batched_cases as SC

ROWS = SC.exact_rows()


@pytest.mark.parametrize("row", ROWS, ids=SC.row_id)
def test_exactness_premise_per_row(row):
    n, k, batch, trans, fill, (alpha, beta), shift, _, _ = row
    for idx in range(min(batch, SC.DISTINCT)):
        V, C, lam = SC.operands(n, k, idx)
        assert V.shape == (n, k) and C.shape == (n, n) and np.array_equal(C, C.T)
        assert set(np.unique(V)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        assert np.array_equal(C, 2.0 * np.round(C / 2.0)) and lam == round(lam) and abs(lam) <= 3
        p = SC.premise(V, C, lam, alpha, beta)
        assert p["bound"] < SC.LIMIT and p["|C|"] <= 8 and p["|V|"] <= 2
        assert p["2 alpha"] == round(p["2 alpha"]) and p["2 beta"] == round(p["2 beta"])
        # any order gives the same float64: the reversed and an interleaved order of the terms against NumPy's
        E = SC.expected(V, C, lam, alpha, beta, shift)
        assert np.array_equal(2.0 * E, np.round(2.0 * E)) and np.array_equal(E, E.T)
        s = np.zeros((n, n))
        for q in list(range(1, k, 2))[::-1] + list(range(0, k, 2)):
            s = s + np.outer(V[:, q], V[:, q])
        t = alpha * s
        out = t if beta == 0.0 else beta * C + t
        if shift:
            out = out + lam * np.eye(n)
        assert np.array_equal(out + 0.0, E)


def test_rows_cover_what_the_gpu_tests_name():
    assert {r[0] for r in ROWS} == set(SC.WAVE_N) | set(SC.GROUP_N)
    assert {r[1] for r in ROWS} == set(SC.KS) | {0}
    assert {r[2] for r in ROWS} == set(SC.BATCHES) and {r[2] for r in ROWS if r[0] <= 64} == set(SC.BATCHES)
    assert all(r[2] <= 3 for r in ROWS if r[0] > 80)
    assert {r[7] for r in ROWS} == set(SC.LAYOUTS) and {r[8] for r in ROWS} == set(SC.LAYOUTS)
    assert {r[5] for r in ROWS if r[1] > 0} == set(SC.AB)
    assert all(r[5] == (1.0, 0.0) for r in ROWS if r[1] == 0)
    for p in ("wave", "group"):
        sub = [r for r in ROWS if SC.path(r[0]) == p]
        have = {(r[3], r[4], r[5][1] == 0.0, r[6]) for r in sub}
        assert have == set(itertools.product((0, 1), (0, 1), (False, True), (0, 1))), (p, sorted(have))
        assert {r[1] % 4 for r in sub if r[1] > 0} == {0, 1, 3} and any(r[1] == 0 for r in sub)
        assert {r[5] for r in sub if r[1] > 0} == set(SC.AB)
    assert SC.WAVE_N == (1, 2, 7, 8, 9, 16, 17, 32, 33, 63, 64) and SC.GROUP_N == (65, 80, 127, 128, 129, 191, 192, 193, 255, 256)
    assert SC.KS == (1, 3, 4, 5, 16, 17, 40) and SC.BATCHES == (1, 3, 65, 257) and SC.LAYOUTS == ((0, 0), (0, 3), (1, 3), (6, 0))
    assert SC.AB == ((1.0, 0.0), (-1.0, 1.0), (2.0, -1.0), (0.5, 0.5), (0.0, 1.0))


def test_expected_ignores_c_when_beta_is_zero():
    V, C, lam = SC.operands(9, 5, 0)
    E = SC.expected(V, np.full((9, 9), np.nan), lam, 1.0, 0.0, 1)
    assert np.array_equal(E, V @ V.T + lam * np.eye(9))
