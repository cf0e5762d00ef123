"""-m gpu: gram256 and qrapply256 (csrc/cqr_kernels.hip) on their own, against EXACT results.

The rows of tests/cqr256_cases.py (tests/test_cqr256_cases.py shows, without a GPU, that they reach every class of the kernels' row
partitions) through cap_dgram256 and cap_dqrapply256.  Operands are small integers, so the float64 NumPy product is the exact result
whatever the summation order, the slab split or the ring phase, and the device must reproduce it bit for bit: a K tile read from a stage
that was not yet (or no longer) its own, a slab left out of the sum or a block column stored from the wrong accumulator changes an
integer, it cannot hide in rounding.  Everything a call must not write holds NaNs (pad rows, the sentinel behind the work buffer), and so
does everything it must write without reading (G, Qout, the work slabs: an empty workgroup that skipped its zero slab would put NaNs
into G); whole buffers are compared as bit patterns.  There is no tolerance in this file except the one random-data test that says so."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cqr256_cases as T  # noqa: E402
from tests.blas3_cases import describe_mismatch, same_bits  # noqa: E402
from tests.gpu_util import DEV, relerr  # noqa: E402

N = T.N
TAIL = 4096                     # sentinel doubles behind the work buffer
_PANELS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_panels():
    yield
    _PANELS.clear()
    torch.cuda.empty_cache()


def _L():
    from capital_amd import _lib
    return _lib.lib()


def _stream():
    from capital_amd._util import cur_stream
    return cur_stream()


def _panel(m):
    """the shared integer panel of m rows on the device, image [256][m]; uploaded once, never written"""
    if m not in _PANELS:
        _PANELS[m] = torch.from_numpy(T.panel(m).copy()).to(DEV)
    return _PANELS[m]


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


def _padded(img, ld):
    """device buffer [256][ld] of the device image img [256][rows], NaN in the pad rows"""
    buf = _nan(img.shape[0], ld)
    buf[:, :img.shape[1]] = img
    return buf


def _bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def _assert_same(got, want, ld, what):
    assert same_bits(got, want), "%s: %s" % (what, describe_mismatch(got, want, ld))


# ------------------------------------------------------------------------------------------------ gram256
def _gram(qbuf, m, ldq, ldg, cap):
    """cap_dgram256 on the device buffer qbuf; G all NaN, work all NaN with a sentinel tail -> (G buffer on the host, sentinel untouched)"""
    L = _L()
    ws = int(L.cap_dgram256_work_size(m))
    assert ws >= N * N and ws % (N * N) == 0
    gbuf = _nan(N, ldg)
    work = _nan(ws + TAIL)
    st = L.cap_dgram256(m, qbuf.data_ptr(), ldq, gbuf.data_ptr(), ldg, work.data_ptr(), cap, _stream())
    assert st == 0, st
    torch.cuda.synchronize()
    return gbuf.cpu().numpy(), bool(torch.isnan(work[ws:]).all()) and _bits_equal(work[ws:], _nan(TAIL))


_GRAM_PARAMS = [(m, cap, pq, pg) for m, cap, _ in T.GRAM_CASES for pq in T.GRAM_LDQ_PADS for pg in T.GRAM_LDG_PADS]


@pytest.mark.parametrize("m,cap,pq,pg", _GRAM_PARAMS, ids=["m%d-wgs%d-ldq+%d-ldg+%d" % p for p in _GRAM_PARAMS])
def test_gram_exact(m, cap, pq, pg):
    ldq, ldg = m + pq, N + pg
    qbuf = _padded(_panel(m), ldq)
    keep = qbuf.clone()
    g, tail_ok = _gram(qbuf, m, ldq, ldg, cap)
    want = T.place_cols(T.gram_reference(m), ldg)           # upper triangle exact, strictly-lower part +0.0, pad rows NaN
    _assert_same(g, want, ldg, "G of m=%d max_wgs=%d ldq=%d ldg=%d (K tiles per workgroup on %d CUs: %s)" % (
        m, cap, ldq, ldg, T.CUS, T.gram_partition(m, cap)[:40]))
    assert tail_ok, "the sentinel behind cap_dgram256_work_size(m) doubles of work was written"
    assert _bits_equal(qbuf, keep), "Q (or its pad rows) changed"


def test_gram_is_bit_identical_from_run_to_run():
    """the one test of this file on random data and with a tolerance: the fixed summation order (258 row tiles, 64 slabs), and the
    figure tests/test_gpu_cacqr_solve.py::test_tall_tn_is_bit_identical_from_run_to_run uses for the same kind of sum"""
    m = 33024
    q = np.random.default_rng(7).standard_normal((N, m))          # image [256][m]
    qbuf = torch.from_numpy(q).to(DEV)
    g0, ok0 = _gram(qbuf, m, m, N, 0)
    g1, ok1 = _gram(qbuf, m, m, N, 0)
    assert ok0 and ok1
    assert same_bits(g0, g1)
    assert relerr(np.tril(g0), np.tril(q @ q.T)) < 1e-14            # (images: row <= col is the image's lower triangle)
    assert np.array_equal(np.triu(g0, 1), np.zeros_like(g0))


def test_gram_large_pitch_exact():
    """the last legal even ldq (128 ldq 8 < 0xfffffff0): the panel spans 8.6 GB of address space, of which only the 128 leading rows of
    its 256 columns are written and read - the largest 32-bit offsets the kernel's descriptors ever carry"""
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip("less than 12 GiB of device memory free (%.1f GiB): the large-pitch panel needs 8.6 GB of address space" % (free / 2 ** 30))
    m, ldq, ldg = T.BIG_GRAM_M, T.GRAM_LD_LAST, N + 3
    qbuf = torch.empty(N * ldq, dtype=torch.float64, device=DEV)
    qbuf.view(N, ldq)[:, :m] = _panel(m)
    g, tail_ok = _gram(qbuf, m, ldq, ldg, 0)
    _assert_same(g, T.place_cols(T.gram_reference(m), ldg), ldg, "G of m=%d ldq=%d" % (m, ldq))
    assert tail_ok
    assert _bits_equal(qbuf.view(N, ldq)[:, :m], _panel(m)), "Q changed"
    del qbuf
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ qrapply256
def _apply(m, cap, ri, pin=2, pout=6):
    """out of place (ldout != ldin, NaN in Qout and in its pad rows), then in place: both must be the exact product"""
    L = _L()
    ldin, ldout = m + pin, m + pout
    q = _panel(m)
    want = T.apply_reference(T.panel(m), ri)
    ridev = torch.from_numpy(ri).to(DEV)
    rikeep = ridev.clone()
    what = "m=%d max_wgs=%d (row tiles per workgroup on %d CUs: %s)" % (m, cap, T.CUS, T.apply_partition(m, cap)[:40])
    qin = _padded(q, ldin)
    keep = qin.clone()
    qout = _nan(N, ldout)
    st = L.cap_dqrapply256(m, qin.data_ptr(), ldin, ridev.data_ptr(), qout.data_ptr(), ldout, cap, _stream())
    assert st == 0, st
    torch.cuda.synchronize()
    out = qout.cpu().numpy()
    _assert_same(out, T.place_cols(want, ldout), ldout, "Qout, out of place, " + what)
    assert _bits_equal(qin, keep), "Qin (or its pad rows) changed"
    st = L.cap_dqrapply256(m, qin.data_ptr(), ldin, ridev.data_ptr(), qin.data_ptr(), ldin, cap, _stream())
    assert st == 0, st
    torch.cuda.synchronize()
    _assert_same(qin.cpu().numpy(), T.place_cols(want, ldin), ldin, "Qout, in place, " + what)
    assert same_bits(qin[:, :m].cpu().numpy(), out[:, :m]), "in place and out of place differ"
    assert _bits_equal(ridev, rikeep), "Ri changed"


@pytest.mark.parametrize("m,cap", [(m, cap) for m, cap, _ in T.APPLY_CASES], ids=["m%d-wgs%d" % (m, cap) for m, cap, _ in T.APPLY_CASES])
def test_apply_exact(m, cap):
    _apply(m, cap, T.ri_dense(m + cap))


@pytest.mark.parametrize("m,cap", [(m, cap) for m, cap, _ in T.APPLY_CASES if m <= 1664], ids=["m%d-wgs%d" % (m, cap) for m, cap, _ in T.APPLY_CASES if m <= 1664])
def test_apply_never_moves_the_blocks_below_the_block_diagonal(m, cap):
    """the kernel's header: 16 x 16 blocks of Rinv below the diagonal are skipped.  With NaN in every one of them the result is still exact -
    a piece of such a block that reached LDS and an MFMA would turn whole columns of Qout into NaN"""
    _apply(m, cap, T.ri_dense(m + cap, below=T.NAN))


@pytest.mark.parametrize("br,bc", T.APPLY_BLOCKS)
def test_apply_single_block(br, bc):
    """Ri = one nonzero 16 x 16 block (br, bc): exactly block column bc of Qout is nonzero, and it is block column br of Qin times the block"""
    _apply(T.APPLY_BLOCK_M, T.APPLY_BLOCK_CAP, T.ri_block(br, bc, 16 * br + bc))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("entry,over,why", T.REFUSALS, ids=["%s-%s" % (e, w.replace(" ", "_")) + "-%d" % i for i, (e, _, w) in enumerate(T.REFUSALS)])
def test_refusals(entry, over, why):
    """what the launchers cannot run is refused before anything is launched: fake pointers, never dereferenced (the same rows are run on
    the recording stand-in by tests/test_cqr256_cases.py, which shows that no launch follows)"""
    assert T.refusal_call(_L(), entry, over, ptr=ctypes.c_void_p) == T.UNSUPPORTED, why


def test_work_size():
    L = _L()
    assert L.cap_dgram256_work_size(0) == 0 and L.cap_dgram256_work_size(-16) == 0
    assert L.cap_dgram256_work_size(16) == N * N == L.cap_dgram256_work_size(1023)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for m in (1024, 14848, 131072, 131088, 1 << 21):
        assert L.cap_dgram256_work_size(m) == T.gram_work_size(m, cus)
