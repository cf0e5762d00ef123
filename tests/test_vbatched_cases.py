"""No GPU: the plans of the variable-size batched Cholesky (cap_vbatch_plan_create / _info / _table) hold what tests/vbatched_cases.py says
they must, and the operands of the GPU tests are what they claim to be.  A plan made in a process without a device is a description: its
tables and counts are complete, only the three entries refuse it."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import vbatched_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")
BATCH, TOTAL, ROWS, NMAX, LAUNCHES, COUNT = 0, 1, 2, 3, 4, 5


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


def make_plan(L, lay):
    arr = lambda a: None if a is None else (C.c_int64 * max(len(a), 1))(*[int(x) for x in a])
    p = C.c_void_p()
    st = L.cap_vbatch_plan_create(lay.batch, arr(lay.sizes), arr(lay.ld_arg), arr(lay.off_arg), C.byref(p))
    return st, p


def tables(L, p):
    out = []
    for c in range(7):
        cnt = L.cap_vbatch_plan_info(p, COUNT + c)
        buf = (C.c_int64 * max(cnt, 1))()
        assert L.cap_vbatch_plan_table(p, c, buf, cnt) == 0
        out.append([int(buf[k]) for k in range(cnt)])
    return out


@pytest.mark.parametrize("kind", V.LAYOUTS)
@pytest.mark.parametrize("name", sorted(V.LISTS))
def test_class_lists_partition_the_blocks_sorted_by_size(L, name, kind):
    sizes = V.LISTS[name]
    lay = V.Layout(sizes, kind)
    st, p = make_plan(L, lay)
    assert st == 0
    try:
        got = tables(L, p)
        flat = sorted(i for l in got for i in l)
        assert flat == [i for i, n in enumerate(sizes) if n > 0]                       # a partition of the non-empty blocks
        for c, l in enumerate(got):
            assert all(V.class_of(sizes[i]) == c for i in l), V.CLASS_NAMES[c]         # only sizes of its class
            ns = [sizes[i] for i in l]
            assert ns == sorted(ns)
            assert all(a < b for a, b, na, nb in zip(l, l[1:], ns, ns[1:]) if na == nb), "not stable"
        assert got == V.expected_lists(sizes)
        info = lambda w: int(L.cap_vbatch_plan_info(p, w))
        assert info(BATCH) == len(sizes) and info(ROWS) == int(np.sum(sizes)) and info(NMAX) == max(sizes)
        assert info(TOTAL) == lay.total
        assert info(LAUNCHES) == sum(1 for l in got if l)
        assert [info(COUNT + c) for c in range(7)] == [len(l) for l in V.expected_lists(sizes)]
        assert info(COUNT + 7) == -1 and info(-1) == -1
        # a short buffer gets the head of the list and nothing behind it
        c = max(range(7), key=lambda c: len(got[c]))
        buf = (C.c_int64 * (len(got[c]) + 1))(*([-5] * (len(got[c]) + 1)))
        assert L.cap_vbatch_plan_table(p, c, buf, 1) == 0
        assert buf[0] == got[c][0] and all(buf[k] == -5 for k in range(1, len(got[c]) + 1))
    finally:
        assert L.cap_vbatch_plan_destroy(p) == 0


def test_every_class_and_both_kernel_paths_are_reached():
    reached = set()
    for sizes in V.LISTS.values():
        reached |= {V.class_of(n) for n in sizes if n}
    assert reached == set(range(7))
    # the lists the bit-equality tests run (EVERY, WAVES, EDGES) reach every class too, each with more than one size in some class
    for name in ("EVERY", "WAVES", "EDGES"):
        ex = V.expected_lists(V.LISTS[name])
        assert any(len({V.LISTS[name][i] for i in l}) > 1 for l in ex[:4]) or name == "EDGES"
    assert {V.class_of(n) for n in V.EVERY if n} == set(range(7))
    assert {V.class_of(n) for n in V.EDGES} == {3, 4, 5, 6}
    w = V.expected_lists(V.WAVES)
    assert len(w[0]) == 70 and len(w[0]) > 2 * 8 and w[1] == [70] and w[6] == [71]     # several waves of NP = 8, a lone block, a lone workgroup
    # a wave of NP = 8 takes eight consecutive entries of the sorted list: some wave mixes sizes
    ns = [V.WAVES[i] for i in w[0]]
    assert any(len(set(ns[k:k + 8])) > 1 for k in range(0, 70, 8))
    assert len(V.EVERY) == len(set(V.EVERY)) + 1 and V.EVERY.count(0) == 2
    assert len(V.EDGES) == 21 and V.EDGES[:8] == (33, 64, 65, 128, 129, 192, 193, 33)


@pytest.mark.parametrize("name", sorted(V.LISTS))
def test_exact_operands_pass_their_premise(name):
    """every exact block of the GPU tests: potri_batched_cases.block asserts T T^-1 = I and the three exactness bounds; here also that
    A = T^T T is formed exactly and that the diagonal is a power of two (the exact log det)"""
    sizes = V.LISTS[name]
    for fam in V.FAMILIES:
        for i, b in enumerate(V.exact_blocks(fam, sizes)):
            if b is None:
                assert sizes[i] == 0
                continue
            T, Ti, Cm = b
            assert T.shape == (sizes[i], sizes[i]) and np.all(np.diagonal(T) > 0)
            A = T.T @ T
            assert np.array_equal(A.astype(np.longdouble), T.T.astype(np.longdouble) @ T.astype(np.longdouble))
            ld, scale = V.exact_logdet(T)
            assert np.isfinite(float(ld)) and scale >= abs(ld)


@pytest.mark.parametrize("kind", V.LAYOUTS)
def test_layouts_do_not_overlap_and_buffers_round_trip(kind):
    sizes = V.EVERY
    lay = V.Layout(sizes, kind)
    seen = np.zeros(lay.total + V.GUARD, dtype=int)
    for i in range(lay.batch):
        if sizes[i]:
            seen[lay.index(i, "window")[0]] += 1
    assert seen.max() == 1 and not seen[lay.total:].any()
    assert lay.written("upper").sum() == sum(n * (n + 1) // 2 for n in sizes)
    mats = [np.arange(n * n, dtype=np.float64).reshape(n, n) + 1 for n in sizes]
    buf = lay.buffer(mats)
    assert np.isnan(buf[~lay.written("upper")]).all() and not np.isnan(buf[lay.written("upper")]).any()
    for i, n in enumerate(sizes):
        if n:
            got = lay.block(buf, i)
            assert np.array_equal(np.triu(got), np.triu(mats[i])) and np.isnan(got[np.tril_indices(n, -1)]).all()
    if kind == "reverse" and lay.batch > 1:
        nz = [i for i in range(lay.batch) if sizes[i]]
        assert all(lay.off[a] > lay.off[b] for a, b in zip(nz, nz[1:]))
