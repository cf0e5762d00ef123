"""CPU-only: the table of the ragged block-tridiagonal tests (tests/blocktri_ragged_cases.py) really has the properties its users rely
on - no NP, no first-mode and no length class without a row - and the exactness premise of tests/test_blocktri_cases.py holds for every
(n, T_c) pair the table uses: all numbers of the recurrence are small integers, the factor of the assembled chain is R itself."""
import numpy as np

from tests import blocktri_cases as BC
from tests import blocktri_ragged_cases as RC


def test_the_table_covers_what_the_kernels_can_get_wrong():
    rows = RC.rows()
    assert {r[0] for r in rows} == {1, 3, 8, 9, 16, 17, 32, 33, 63, 64}
    assert {r[2] for r in rows} == set(RC.FIRST_MODES) and {r[4] for r in rows} == set(RC.LAYOUTS) and {r[3] for r in rows} == {1, 3, 17, 70}
    for NP in (8, 16, 32, 64):
        mine = [r for r in rows if RC.padded(r[0]) == NP]
        assert any(len(set(r[1])) > 1 for r in mine) and any(0 in r[1] for r in mine)
        assert {min(t, 3) for r in mine for t in r[1]} == {0, 1, 2, 3}                      # every length class: 0, 1, 2, more
        G = 64 // NP
        if G > 1:
            assert any(len(r[1]) % G for r in mine)                                            # a ragged last wavefront
            waves = [[r[1][c] for c in RC.order(r[1])[w:w + G]] for r in mine for w in range(0, len(r[1]), G)]
            full = [w for w in waves if len(w) == G and len(set(w)) == G]
            assert full, NP                                                                    # one wavefront whose chains all differ
            if G >= 4:
                assert any({0, 1, 2} <= set(w) for w in full), NP
            else:
                assert any({1, 2} <= set(w) for w in full) and any(0 in w for w in waves), NP
            assert any(r[1][0] != max(r[1]) for r in mine)                                     # the longest chain is not first in batch order
    assert any(set(r[1]) == {1, 257} and r[0] == 8 for r in rows)
    assert any(r[1] == (2, 1, 3, 0) and RC.padded(r[0]) == 64 for r in rows)
    assert any(len(set(r[1])) == 1 and len(r[1]) > 1 for r in rows)
    assert all(r in rows for r in RC.STREAM_ROWS) and {RC.padded(r[0]) for r in RC.STREAM_ROWS} == {8, 64}


def test_the_geometry_of_every_row_is_a_legal_plan():
    for row in RC.rows():
        n, lengths, mode, nrhs, lay = row
        first, rows_at, slots, eslots, total = RC.geometry(row)
        spans = sorted((f, f + t) for f, t in zip(first, lengths) if t)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and total == sum(lengths) and slots >= total
        if mode == "gaps":
            assert slots > total
        if mode == "reversed":
            assert first[0] == max(first)
        assert RC.order(lengths) == sorted(range(len(lengths)), key=lambda c: (-lengths[c], c))
        ld, step, ldb = RC.layout(row)
        assert ld >= n and step >= ld * n and ldb >= total * n


def test_every_chain_of_the_table_is_exact():
    seen = set()
    for row in RC.rows():
        n, lengths, _, nrhs, _ = row
        for c, T in enumerate(lengths):
            if (n, T, nrhs) in seen or T == 0:
                continue
            seen.add((n, T, nrhs))
            D, Bc, X, rhs, U, W, logdet = RC.exact_chain(row, c)
            assert D.shape == (T, n, n) and Bc.shape == (max(T - 1, 0), n, n) and X.shape == (T * n, nrhs)
            A = BC.dense(D[None], Bc[None])[0]
            R = BC.dense_factor(U[None], W[None])[0]
            assert np.array_equal(R.T @ R, A) and np.array_equal(A @ X, rhs)
            assert (np.diagonal(R) > 0).all() and np.abs(A).max() < 2 ** 20 and np.abs(rhs).max() < 2 ** 30
            assert np.isclose(logdet, 2.0 * np.log(np.diagonal(R).astype(np.float64)).sum(), rtol=1e-13, atol=1e-12)   # det A = (prod diag R)^2
        for c, T in enumerate(lengths):
            if T == 0:
                D, Bc, X, rhs, U, W, logdet = RC.exact_chain(row, c)
                assert D.shape[0] == 0 and rhs.shape[0] == 0 and logdet == 0.0
