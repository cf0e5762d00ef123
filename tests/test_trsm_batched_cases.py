"""CPU-only: the exact operands of tests/trsm_batched_cases.py are what they claim to be - the exactness premise per row, the products formed
exactly, the rows covering every size, right-hand-side count, batch and layout the GPU tests name - and the host model of the sumsq
recurrence is a correctly rounded fused multiply-add."""
import math

import numpy as np
import pytest

from tests import trsm_batched_cases as TC

ROWS = TC.exact_rows()


@pytest.mark.parametrize("row", ROWS, ids=TC.row_id)
def test_exactness_premise_per_row(row):
    n, fam, batch, nrhs, _ = row
    for idx in range(min(batch, TC.DISTINCT)):
        T, Ti, X, BT, BN = TC.operands(fam, n, nrhs, idx)
        assert np.all(np.diagonal(T) > 0) and np.array_equal(T, np.triu(T))
        assert set(np.unique(X)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        for name, v in TC.premise(T, Ti, X).items():
            assert np.isfinite(v) and v < TC.LIMIT, "%s block %d: %s = 2^%.1f is not below 2^53" % (TC.row_id(row), idx, name, math.log2(v))
        # the products are exact: the closed-form inverse takes them back, and every entry is a multiple of 2^-f
        assert np.array_equal(Ti.T @ BT, X) and np.array_equal(Ti @ BN, X)
        f = 2.0 ** TC.fraction_bits(T)
        assert np.array_equal(np.round(BT * f), BT * f) and np.array_equal(np.round(BN * f), BN * f)


def test_rows_cover_what_the_gpu_tests_name():
    assert {r[0] for r in ROWS} == set(TC.WAVE_N) | set(TC.GROUP_N)
    assert {r[3] for r in ROWS} == set(TC.NRHS) and {r[2] for r in ROWS} == set(TC.BATCHES) and {r[4] for r in ROWS} == set(TC.LAYOUTS)
    for sizes in (TC.WAVE_N, TC.GROUP_N):
        sub = [r for r in ROWS if r[0] in sizes]
        assert {r[3] for r in sub} == set(TC.NRHS) and {r[4] for r in sub} == set(TC.LAYOUTS)
        assert {r[1] for r in sub} == set(TC.P.FAMILIES)
    assert {r[2] for r in ROWS if r[0] <= 64} == set(TC.BATCHES)
    assert TC.WAVE_N == (1, 2, 7, 8, 9, 16, 17, 32, 33, 63, 64) and TC.GROUP_N == (65, 80, 127, 128, 129, 191, 192, 193, 255, 256)
    assert TC.NRHS == (1, 3, 16, 17, 40) and TC.BATCHES == (1, 3, 65, 257) and TC.LAYOUTS == ((0, 0), (0, 3), (1, 3), (6, 0))


def test_fraction_bits():
    assert TC.fraction_bits(np.array([[1.0, 2.0]])) == 0 and TC.fraction_bits(np.array([[0.5, 0.75]])) == 2


def test_sumsq_model_is_a_correctly_rounded_fma_chain():
    x = [1.0 + 2.0 ** -30, 3.0, 2.0 ** -40]
    # (1 + 2^-30)^2 = 1 + 2^-29 + 2^-60: the fused step rounds once (2^-60 is lost), a separate product would round the same way here;
    # the second step 9 + (1 + 2^-29) is exact; the third adds 2^-80, which is lost
    assert TC.sumsq_model(x) == 10.0 + 2.0 ** -29
    # (2^27 + 1)^2 = 2^54 + 2^28 + 1 is not a float64 (spacing 4 there): one rounding drops the 1.  With q = 2 the fused step sees
    # ... + 3 and rounds up to + 4; a rounded product plus 2 would be a tie that goes back to + 0
    assert TC.sumsq_model([2.0 ** 27 + 1.0]) == 2.0 ** 54 + 2.0 ** 28
    assert TC.sumsq_model([1.0, 1.0, 2.0 ** 27 + 1.0]) == 2.0 ** 54 + 2.0 ** 28 + 4.0
    if hasattr(math, "fma"):
        q = 0.0
        for v in x:
            q = math.fma(v, v, q)
        assert q == TC.sumsq_model(x)
    assert TC.sumsq_model([1.0, 2.0, -2.0, 0.0]) == 9.0 and math.isnan(TC.sumsq_model([1.0, float("nan")]))
