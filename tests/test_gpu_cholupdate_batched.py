"""-m gpu: the batched rank-k update / downdate of fp64 Cholesky factors (cap_dcholupdate_batched, cap_dcholupdate_vbatched,
batched.update / downdate, VarBatch.update / downdate).

1. an exact family that needs no other kernel (diagonal factors 3 2^e with V = diag(4 2^e): 3-4-5), 2. THE BIT CONTRACT against
cap_dcholupdate on every block alone, 3. accuracy under the gates of tests/cholupdate_model.py, 4. what is never touched, 5. failing and
skipped blocks, 6. independence of position and layout, 7. variable sizes on a plan, 8. factor -> update -> solve chains through the Python
layer, 9. stream order.  Blocks are column-major n x n windows of a flat buffer that starts as NaN everywhere."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import cholupdate_model as cm
from tests import stream_order as SO
from tests import vbatched_cases as VC
from tests.gpu_util import NanWork

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OK = 0
GUARD = 16


def _L():
    from capital_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _np_bits(a):
    return np.array(a, dtype=np.float64, order="C").view(np.int64)       # (a copy: torch.from_numpy wants writable memory)


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


class Flat:
    """`batch` column-major rows x cols windows, window i at i * stride with leading dimension ld, in a flat NaN buffer with a NaN guard
    behind the last one; tri: only the elements with row <= col are laid in (the rest of the window stays NaN)"""

    def __init__(self, mats, ld, stride, tri, lead=0):
        rows, cols = mats[0].shape
        self.rows, self.cols, self.ld, self.stride, self.batch, self.lead = rows, cols, ld, stride, len(mats), lead
        size = lead + stride * (len(mats) - 1) + ld * cols + GUARD
        host = np.full(size, np.nan)
        r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
        self.mask = (r <= c) if tri else (r >= 0)
        self.r, self.c = r[self.mask], c[self.mask]
        self.touched = np.zeros(size, dtype=bool)
        for i, M in enumerate(mats):
            host[self.index(i)] = np.asarray(M, dtype=np.float64)[self.r, self.c]
            self.touched[self.index(i)] = True
        self.dev = torch.from_numpy(host).to(DEV)

    def index(self, i):
        return self.lead + i * self.stride + self.r + self.c * self.ld

    def ptr(self):
        return self.dev.data_ptr() + 8 * self.lead

    def get(self, i, host=None):
        host = self.dev.cpu().numpy() if host is None else host
        out = np.zeros((self.rows, self.cols))
        out[self.r, self.c] = host[self.index(i)]
        return out

    def all(self):
        host = self.dev.cpu().numpy()
        return [self.get(i, host) for i in range(self.batch)]

    def rest_is_nan(self):
        host = self.dev.cpu().numpy()
        return bool(np.isnan(host[~self.touched]).all()) and bool(np.isfinite(host[self.touched]).all())


def _batched(sign, Rf, Vf, info=None, batch=None):
    st = _L().cap_dcholupdate_batched(1, sign, Rf.rows, Vf.cols, Rf.ptr(), Rf.ld, Rf.stride, Vf.ptr(), Vf.ld, Vf.stride,
                                      Rf.batch if batch is None else batch, info.data_ptr() if info is not None else None, _stream())
    torch.cuda.synchronize()
    return st


def _run(sign, Rs, Vs, ldr=None, sr=None, ldv=None, sv=None, info=None, lead=0):
    """the batch Rs (upper factors), Vs through the fixed-size entry -> (list of upper triangles, info as NumPy or None, Rf, Vf)"""
    n, k = Vs[0].shape
    ldr, ldv = ldr or max(n, 1), ldv or max(n, 1)
    Rf = Flat(Rs, ldr, sr or ldr * n, True, lead)
    Vf = Flat(Vs, ldv, sv or ldv * k, False, lead)
    inf = None if info is None else torch.tensor(info, dtype=torch.int32, device=DEV)
    assert _batched(sign, Rf, Vf, inf) == OK
    return Rf.all(), (None if inf is None else inf.cpu().numpy()), Rf, Vf


def _single(sign, R, V):
    """cap_dcholupdate (the one-launch driver) on this block alone -> (upper triangle, info)"""
    L = _L()
    n, k = V.shape
    Rf, Vf = Flat([R], n, n * n, True), Flat([V], n, n * k, False)
    work = NanWork(L.cap_dcholupdate_work_size(n, k))                    # all NaN, exactly the stated size, a sentinel behind it
    info = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    assert L.cap_dcholupdate(1, sign, n, k, Rf.ptr(), n, Vf.ptr(), n, info.data_ptr(), work.data_ptr(), _stream()) == OK
    work.check("cap_dcholupdate(n = %d, k = %d)" % (n, k))
    return Rf.get(0), int(info.item())


@functools.lru_cache(maxsize=None)
def _operands(n, k, count):
    """count blocks (A, R = chol(A)^T, V), a seed of its own per block; computed once per shape and never written"""
    out = []
    for i in range(count):
        A, V = cm.spd(n, 1000 * i + n), cm.thin(n, k, 7000 + 1000 * i + n)
        R = np.linalg.cholesky(A).T.copy()
        for x in (A, R, V):
            x.setflags(write=False)
        out.append((A, R, V))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _updated(n, k, count):
    """(batched update of _operands, its info) - computed once, shared by the bit-contract and the accuracy tests"""
    ops = _operands(n, k, count)
    got, info, Rf, Vf = _run(+1, [o[1] for o in ops], [o[2] for o in ops], info=[0] * count)
    for g in got:
        g.setflags(write=False)
    return tuple(got), info


# ---- 1. the exact family ----------------------------------------------------------------------------------------------------------------------
EXACT_N = (1, 7, 8, 9, 16, 17, 33, 64, 65, 128, 129, 192, 193, 255, 256)


def _exact_batch(n):
    np_ = 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64
    return 64 // np_ + 1 if n <= 64 else 3


@pytest.mark.parametrize("n", EXACT_N)
def test_exact_three_four_five_family(n):
    batch = _exact_batch(n)
    e = [np.random.default_rng(300 + 17 * i + n).integers(-2, 3, n).astype(np.float64) for i in range(batch)]
    Rs, Vs = [np.diag(3.0 * 2.0 ** x) for x in e], [np.diag(4.0 * 2.0 ** x) for x in e]
    got, info, Rf, Vf = _run(+1, Rs, Vs, info=[0] * batch)
    assert not info.any()
    for i in range(batch):
        assert _same(got[i], np.diag(5.0 * 2.0 ** e[i])), "block %d of %d: not diag(5 2^e) with +0 off the diagonal" % (i, batch)
    inf = torch.zeros(batch, dtype=torch.int32, device=DEV)
    assert _batched(-1, Rf, Vf, inf) == OK                       # the downdate of the result, in place, with the same V
    assert not inf.cpu().numpy().any()
    for i, g in enumerate(Rf.all()):
        assert _same(g, Rs[i]), "block %d of %d: the downdate did not return diag(3 2^e)" % (i, batch)


@pytest.mark.parametrize("n", (8, 33, 64, 65, 200))
@pytest.mark.parametrize("sign", (+1, -1))
def test_zero_v_keeps_every_bit(n, sign):
    ops = _operands(n, 3, 3)
    Rs = [o[1] for o in ops]
    got, info, _, _ = _run(sign, Rs, [np.zeros((n, 3))] * 3, info=[0] * 3)
    assert not info.any()
    for g, R in zip(got, Rs):
        assert _same(g, np.triu(R))


# ---- 2. the bit contract ----------------------------------------------------------------------------------------------------------------------
# every NK instance (1, 2, 4, 8, 16; 3, 5 and 9 columns are padded ones) and a second and a third pass on both paths
BIT_CASES = [(1, 1, 5), (2, 2, 5), (8, 3, 5), (9, 4, 5), (31, 5, 5), (32, 8, 5), (33, 9, 3), (63, 16, 3), (64, 17, 3), (64, 33, 3),
             (65, 1, 3), (127, 2, 3), (128, 3, 3), (129, 4, 3), (191, 5, 3), (192, 8, 3), (193, 9, 3), (255, 16, 3), (256, 17, 3), (65, 33, 3),
             (256, 33, 2)]


@pytest.mark.parametrize("n,k,batch", BIT_CASES)
def test_bits_are_those_of_the_single_matrix_call(n, k, batch):
    ops = _operands(n, k, batch)
    got, info = _updated(n, k, batch)
    assert not info.any()
    for i, (A, R, V) in enumerate(ops):
        want, winfo = _single(+1, R, V)
        assert winfo == 0
        assert torch.equal(torch.from_numpy(_np_bits(got[i])), torch.from_numpy(_np_bits(want))), "update: block %d differs" % i
    down, dinfo, _, _ = _run(-1, list(got), [o[2] for o in ops], info=[0] * batch)       # the updated factors: the downdate is safe
    assert not dinfo.any()
    for i, (A, R, V) in enumerate(ops):
        want, winfo = _single(-1, got[i], V)
        assert winfo == 0
        assert torch.equal(torch.from_numpy(_np_bits(down[i])), torch.from_numpy(_np_bits(want))), "downdate: block %d differs" % i


# ---- 3. accuracy ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,batch", [(9, 4, 5), (64, 17, 3), (65, 1, 3), (129, 4, 3), (256, 17, 3)])
def test_accuracy_under_the_projects_gates(n, k, batch):
    ops = _operands(n, k, batch)
    got, _ = _updated(n, k, batch)
    for i, (A, R, V) in enumerate(ops):
        A1 = A + V @ V.T
        ref = np.linalg.cholesky(A1).T
        model, minfo = cm.sweep(R, V, +1.0)
        assert minfo == 0
        e_ref, e_model, e_b = cm.element_error(got[i], ref), cm.element_error(got[i], model), cm.backward_error(got[i], A1)
        print("n=%d k=%d block %d update: elementwise %.2e (NumPy cholesky) %.2e (model), backward %.2e" % (n, k, i, e_ref, e_model, e_b))
        assert e_ref <= cm.ELEMENT_GATE and e_model <= cm.ELEMENT_GATE and e_b <= cm.BACKWARD_GATE
    down, dinfo, _, _ = _run(-1, list(got), [o[2] for o in ops], info=[0] * batch)
    assert not dinfo.any()
    for i, (A, R, V) in enumerate(ops):
        d_e, d_b = cm.element_error(down[i], R), cm.backward_error(down[i], A)
        print("n=%d k=%d block %d downdate: elementwise %.2e (the original R), backward %.2e" % (n, k, i, d_e, d_b))
        assert d_e <= cm.ELEMENT_GATE and d_b <= cm.BACKWARD_GATE


# ---- 4. what is not touched -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (8, 64, 65, 200))
@pytest.mark.parametrize("sign", (+1, -1))
def test_only_the_upper_triangles_are_touched(n, sign):
    k, batch = 5, 3
    ops = _operands(n, k, batch)
    Rs = [o[1] for o in ops] if sign > 0 else list(_updated(n, k, batch)[0])
    ldr, ldv = n + 3, n + 5
    got, info, Rf, Vf = _run(sign, Rs, [o[2] for o in ops], ldr, ldr * n + 7, ldv, ldv * k + 9, info=[0] * batch)
    vbits = _np_bits(Flat([o[2] for o in ops], ldv, ldv * k + 9, False).dev.cpu().numpy())
    assert not info.any()
    assert Rf.rest_is_nan(), "strictly lower triangle, padding rows, gaps or the region behind the last block written, or a result is not finite"
    assert np.array_equal(_np_bits(Vf.dev.cpu().numpy()), vbits), "V was written"
    ref, _, _, _ = _run(sign, Rs, [o[2] for o in ops], info=[0] * batch)
    for a, b in zip(got, ref):
        assert _same(a, b)


# ---- 5. failing and skipped blocks ------------------------------------------------------------------------------------------------------------
def _fail_rows(n):
    return sorted({0, min(n - 1, 5), n - 1})           # the first row, inside the first tile, the last row (a later strip for n > 64)


@pytest.mark.parametrize("n", (8, 64, 65, 200))
def test_failing_and_skipped_blocks(n):
    batch = 5
    ops = _operands(n, 1, batch)
    Rs, Vs = [o[1] for o in ops], [o[2] for o in ops]
    Ru = list(_updated(n, 1, batch)[0])                  # safe to downdate with Vs
    others = [0, 1, 3, 4]
    clean, cinfo, _, _ = _run(-1, [Ru[i] for i in others], [Vs[i] for i in others], info=[0] * 4)
    assert not cinfo.any()
    for r0 in _fail_rows(n):
        V = list(Vs)
        V[2] = 1.5 * Ru[2][r0, :].reshape(n, 1)
        got, info, _, _ = _run(-1, Ru, V, info=[0] * batch)
        assert info.tolist() == [0, 0, r0 + 1, 0, 0]
        for r in range(r0):
            assert _same(got[2][r, r:], Ru[2][r, r:]), "row %d above the failing one changed" % r
        assert np.isnan(got[2][r0, r0])
        want, winfo = _single(-1, Ru[2], V[2])
        assert winfo == r0 + 1 and _same(got[2], want)
        for j, i in enumerate(others):
            assert _same(got[i], clean[j]), "block %d changed beside a failing block" % i
    # a block that had failed before the call keeps all its bits and its word
    got, info, _, _ = _run(-1, Ru, Vs, info=[0, 9, 0, 0, 0])
    assert info.tolist() == [0, 9, 0, 0, 0]
    assert _same(got[1], np.triu(Ru[1])) and _same(got[0], clean[0]) and _same(got[3], clean[2]) and _same(got[4], clean[3])
    # info = NULL: every block is swept
    got, info, _, _ = _run(-1, Ru, Vs, info=None)
    assert info is None and all(_same(got[i], clean[j]) for j, i in enumerate(others))


# ---- 6. position and layout -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (9, 64, 129))
def test_bits_do_not_depend_on_position_or_layout(n):
    k, batch = 5, 4
    ops = _operands(n, k, batch)
    Rs, Vs = [o[1] for o in ops], [o[2] for o in ops]
    base, info, _, _ = _run(+1, Rs, Vs, info=[0] * batch)
    perm = [2, 0, 3, 1]
    got, _, Rf, _ = _run(+1, [Rs[i] for i in perm], [Vs[i] for i in perm], n + 2, (n + 2) * n + 11, n + 4, (n + 4) * k + 3, info=[0] * batch, lead=1)
    assert Rf.ptr() % 16 == 8                           # an odd multiple of 8 bytes
    for j, i in enumerate(perm):
        assert _same(got[j], base[i]), "block %d at position %d" % (i, j)
    for i in range(batch):
        one, _, _, _ = _run(+1, [Rs[i]], [Vs[i]], n + 1, 0, n + 1, 0)
        assert _same(one[0], base[i]), "block %d as a batch of one" % i


# ---- 7. variable sizes ------------------------------------------------------------------------------------------------------------------------
def _arr(a):
    return None if a is None else (C.c_int64 * max(len(a), 1))(*[int(x) for x in a])


class Plan:
    def __init__(self, lay):
        self.h = C.c_void_p()
        assert _L().cap_vbatch_plan_create(lay.batch, _arr(lay.sizes), _arr(lay.ld_arg), _arr(lay.off_arg), C.byref(self.h)) == OK

    def __del__(self):
        _L().cap_vbatch_plan_destroy(self.h)


@functools.lru_cache(maxsize=None)
def _var_block(n, k, seed):
    A, V = cm.spd(n, 50 + seed), cm.thin(n, k, 90 + seed)
    return np.linalg.cholesky(A).T.copy(), V


@functools.lru_cache(maxsize=None)
def _var_alone(n, k, seed, sign):
    """cap_dcholupdate_batched on this block alone (batch = 1): the reference of the plan entry, once per block"""
    R, V = _var_block(n, k, seed)
    got, info, _, _ = _run(sign, [R], [V], info=[0])
    assert not info.any()
    return got[0]


def _var_case(sizes, kind, k, sign, seeds):
    lay = VC.Layout(sizes, kind)
    blocks = [_var_block(int(n), k, s) if n else None for n, s in zip(lay.sizes, seeds)]
    buf = lay.buffer([b[0] if b else None for b in blocks])
    ldv = lay.rows + 3
    Vh = np.full((k, ldv), np.nan)
    for i, b in enumerate(blocks):
        if b:
            Vh[:, lay.row_off[i]:lay.row_off[i] + lay.sizes[i]] = b[1].T
    info_h = np.array([0 if n else 77 for n in lay.sizes], dtype=np.int32)
    Rd, Vd, info = torch.from_numpy(buf).to(DEV), torch.from_numpy(Vh).to(DEV), torch.from_numpy(info_h).to(DEV)
    plan = Plan(lay)
    assert _L().cap_dcholupdate_vbatched(plan.h, 1, sign, k, Rd.data_ptr(), Vd.data_ptr(), ldv, info.data_ptr(), _stream()) == OK
    torch.cuda.synchronize()
    out = Rd.cpu().numpy()
    assert np.array_equal(info.cpu().numpy(), info_h), "info of a clean block changed, or an empty block's entry was written"
    assert np.array_equal(_np_bits(Vd.cpu().numpy()), _np_bits(Vh)), "V was written"
    keep = ~lay.written("upper")
    assert np.array_equal(_np_bits(out[keep]), _np_bits(buf[keep])), "something outside the upper triangles was written"
    return lay, [np.triu(lay.block(out, i)) if lay.sizes[i] else None for i in range(lay.batch)]


@pytest.mark.parametrize("name,kind,k,sign", [("EVERY", "gaps", 3, +1), ("EVERY", "ld+3", 17, +1), ("ONE_CLASS", "packed", 5, +1),
                                              ("EDGES", "reverse", 1, +1), ("LONE1", "packed", 2, +1), ("LONE256", "ld+3", 8, +1)])
def test_plan_gives_every_block_the_fixed_size_bits(name, kind, k, sign):
    sizes = VC.LISTS[name]
    seeds = list(range(len(sizes)))
    lay, got = _var_case(sizes, kind, k, sign, seeds)
    if name == "EVERY":
        assert sorted({VC.class_of(int(n)) for n in sizes if n}) == list(range(7)) and 0 in sizes
    for i, n in enumerate(sizes):
        if n:
            assert _same(got[i], _var_alone(int(n), k, seeds[i], sign)), "block %d (n = %d)" % (i, n)


def test_plan_downdate_and_permuted_batch():
    sizes, k = VC.LISTS["EVERY"], 3
    seeds = list(range(len(sizes)))
    lay, up = _var_case(sizes, "gaps", k, +1, seeds)
    perm = np.random.default_rng(5).permutation(len(sizes))
    lay2, up2 = _var_case([sizes[i] for i in perm], "packed", k, +1, [seeds[i] for i in perm])
    for j, i in enumerate(perm):
        assert (up[i] is None and up2[j] is None) or _same(up2[j], up[i]), "block %d at position %d" % (i, j)
    # the downdate of the updated factors through the plan against the fixed-size entry on each block alone
    lay = VC.Layout(sizes, "gaps")
    buf = lay.buffer(up)
    ldv = lay.rows
    Vh = np.zeros((k, ldv))
    for i, n in enumerate(sizes):
        if n:
            Vh[:, lay.row_off[i]:lay.row_off[i] + n] = _var_block(int(n), k, seeds[i])[1].T
    Rd, Vd = torch.from_numpy(buf).to(DEV), torch.from_numpy(Vh).to(DEV)
    info = torch.zeros(lay.batch, dtype=torch.int32, device=DEV)
    plan = Plan(lay)
    assert _L().cap_dcholupdate_vbatched(plan.h, 1, -1, k, Rd.data_ptr(), Vd.data_ptr(), ldv, info.data_ptr(), _stream()) == OK
    torch.cuda.synchronize()
    out = Rd.cpu().numpy()
    assert not info.cpu().numpy().any()
    for i, n in enumerate(sizes):
        if n:
            want, winfo, _, _ = _run(-1, [up[i]], [_var_block(int(n), k, seeds[i])[1]], info=[0])
            assert _same(np.triu(lay.block(out, i)), want[0]), "downdate: block %d (n = %d)" % (i, n)


# ---- 8. chains through the Python layer -----------------------------------------------------------------------------------------------------
def _rel(x, ref):
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("n,k", [(20, 3), (100, 17)])
def test_factor_update_solve_chain(n, k):
    from capital_amd import batched
    batch = 4
    ops = _operands(n, k, batch)
    A = np.stack([o[0] for o in ops])
    V = np.ascontiguousarray(np.stack([o[2].T for o in ops]))       # (batch, k, n): V[i, q] is column q of V_i
    b = np.random.default_rng(n).standard_normal((batch, n))
    Ad, Vd = torch.from_numpy(A).to(DEV), torch.from_numpy(V).to(DEV)
    info = batched.potrf(Ad)
    assert batched.update(Ad, Vd, info) is info
    x = batched.potrs(Ad, torch.from_numpy(b).to(DEV), info).cpu().numpy()
    L1 = torch.tril(Ad).cpu().numpy()
    for i in range(batch):
        A1 = A[i] + V[i].T @ V[i]
        assert _rel(x[i], np.linalg.solve(A1, b[i])) <= 1e-12
        assert _rel(L1[i] @ L1[i].T, A1) <= 1e-13                   # torch's reading: the lower triangle holds L'
    info2 = batched.downdate(Ad, Vd)
    assert info2.dtype == torch.int32 and info2.shape == (batch,) and not info2.cpu().numpy().any() and not info.cpu().numpy().any()
    x = batched.potrs(Ad, torch.from_numpy(b).to(DEV)).cpu().numpy()
    for i in range(batch):
        assert _rel(x[i], np.linalg.solve(A[i], b[i])) <= 1e-12
    x1 = torch.from_numpy(np.stack([o[2][:, 0] for o in ops])).to(DEV)      # (batch, n): one column
    assert not batched.update(Ad, x1).cpu().numpy().any()


def test_varbatch_update_solve_chain():
    from capital_amd import batched
    sizes, k = [5, 0, 70, 33, 130], 3
    vb = batched.VarBatch(sizes)
    mats = [cm.spd(n, 400 + n) if n else np.zeros((0, 0)) for n in sizes]
    Vs = [cm.thin(n, k, 500 + n) for n in sizes]
    A = vb.pack([torch.from_numpy(m) for m in mats])
    Vd = torch.from_numpy(np.concatenate([v.T for v in Vs], axis=1).copy()).to(DEV)        # (k, rows)
    b = np.random.default_rng(3).standard_normal(vb.rows)
    info = vb.potrf(A)
    assert vb.update(A, Vd, info) is info
    x = vb.potrs(A, torch.from_numpy(b).to(DEV), info).cpu().numpy()
    for i, n in enumerate(sizes):
        if n:
            sl = slice(vb.row_offsets[i], vb.row_offsets[i] + n)
            assert _rel(x[sl], np.linalg.solve(mats[i] + Vs[i] @ Vs[i].T, b[sl])) <= 1e-12
    assert not vb.downdate(A, Vd).cpu().numpy().any()
    x = vb.potrs(A, torch.from_numpy(b).to(DEV)).cpu().numpy()
    for i, n in enumerate(sizes):
        if n:
            sl = slice(vb.row_offsets[i], vb.row_offsets[i] + n)
            assert _rel(x[sl], np.linalg.solve(mats[i], b[sl])) <= 1e-12
    assert not vb.update(A, Vd[0]).cpu().numpy().any()              # (rows,): one column


def test_python_refusals():
    from capital_amd import _lib, batched
    n, batch = 12, 3
    R = torch.eye(n, dtype=torch.float64, device=DEV).repeat(batch, 1, 1)
    V = torch.zeros(batch, 2, n, dtype=torch.float64, device=DEV)
    wide = torch.zeros(batch, 2, 2 * n, dtype=torch.float64, device=DEV)
    bad = [lambda f: f(R.cpu(), V), lambda f: f(R, V.cpu()), lambda f: f(R, V.to(torch.float32)), lambda f: f(R.to(torch.float32), V),
           lambda f: f(R, V[:, :, :-1]), lambda f: f(R, V[:2]), lambda f: f(R, torch.zeros(batch, 2, n, 1, dtype=torch.float64, device=DEV)),
           lambda f: f(R, wide[:, :, ::2]),                                       # columns that are not contiguous
           lambda f: f(R, V[:, :1].expand(batch, 2, n)),                          # overlapping columns
           lambda f: f(R, V, torch.zeros(batch, dtype=torch.int32)),              # info on another device
           lambda f: f(R, V, torch.zeros(batch, dtype=torch.int64, device=DEV)), lambda f: f(R, V, torch.zeros(batch - 1, dtype=torch.int32, device=DEV))]
    for f in (batched.update, batched.downdate):
        for call in bad:
            with pytest.raises(_lib.CapitalError):
                call(f)
    vb = batched.VarBatch([3, 5])
    A = torch.zeros(vb.total, dtype=torch.float64, device=DEV)
    for f in (vb.update, vb.downdate):
        for Vb in (torch.zeros(7, dtype=torch.float64, device=DEV), torch.zeros(8, 2, dtype=torch.float64, device=DEV),
                   torch.zeros(8, dtype=torch.float32, device=DEV), torch.zeros(8, dtype=torch.float64),
                   torch.zeros(2, 16, dtype=torch.float64, device=DEV)[:, ::2]):
            with pytest.raises(_lib.CapitalError):
                f(A, Vb)
        with pytest.raises(_lib.CapitalError):
            f(A, torch.zeros(8, dtype=torch.float64, device=DEV), torch.zeros(2, dtype=torch.int32))
    assert bool((R == torch.eye(n, dtype=torch.float64, device=DEV)).all())


# ---- 9. stream order --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    e = SO.Env(2)
    yield e
    e.close()


def _fixed_job(n, k, batch, sign):
    ops = _operands(n, k, batch)
    Rs = [o[1] for o in ops] if sign > 0 else list(_updated(n, k, batch)[0])
    ldr, ldv = n + 1, n + 2
    Rf, Vf = Flat(Rs, ldr, ldr * n + 3, True), Flat([o[2] for o in ops], ldv, ldv * k + 5, False)
    host = {"R": Rf.dev.cpu().numpy(), "V": Vf.dev.cpu().numpy(), "info": np.zeros(batch, dtype=np.int32)}

    def enqueue(ptr, stream):
        assert _L().cap_dcholupdate_batched(1, sign, n, k, ptr["R"], ldr, ldr * n + 3, ptr["V"], ldv, ldv * k + 5, batch, ptr["info"], stream) == OK
    return SO.Job(host, enqueue, label="cap_dcholupdate_batched n=%d k=%d sign=%d" % (n, k, sign))


def _plan_job(plan, lay, k, sign, salt):
    blocks = [_var_block(int(n), k, salt + i) if n else None for i, n in enumerate(lay.sizes)]
    buf = lay.buffer([b[0] if b else None for b in blocks])
    ldv = lay.rows + 1
    Vh = np.full((k, ldv), np.nan)
    for i, b in enumerate(blocks):
        if b:
            Vh[:, lay.row_off[i]:lay.row_off[i] + lay.sizes[i]] = b[1].T
    host = {"R": buf, "V": Vh.ravel(), "info": np.zeros(lay.batch, dtype=np.int32)}

    def enqueue(ptr, stream):
        assert _L().cap_dcholupdate_vbatched(plan.h, 1, sign, k, ptr["R"], ptr["V"], ldv, ptr["info"], stream) == OK
    return SO.Job(host, enqueue, label="cap_dcholupdate_vbatched k=%d salt=%d" % (k, salt))


def _check_ordered(j, ref):
    for name, want in ref.items():
        assert SO.same_bits(j.snap[name], want), "%s: buffer %s differs from the NULL-stream run" % (j.label, name)


@pytest.mark.parametrize("n,k,sign", [(33, 17, +1), (130, 5, -1)])
def test_fixed_size_call_is_ordered_by_its_stream(env, n, k, sign):
    job = _fixed_job(n, k, 37, sign)
    ref, _ = env.plain(job)
    assert not ref["info"].any() and np.isfinite(ref["R"][~np.isnan(job.bufs["R"])]).all()
    with env.ordered(job, label=job.label) as j:
        _check_ordered(j, ref)


def test_plan_calls_are_ordered_on_two_streams_at_once(env):
    lay = VC.Layout(VC.LISTS["EVERY"], "gaps")
    plan = Plan(lay)
    jobs = [_plan_job(plan, lay, 3, +1, 0), _plan_job(plan, lay, 17, +1, 100)]
    refs = [env.plain(j)[0] for j in jobs]
    for r in refs:
        assert not r["info"].any()
    with env.ordered(jobs[0], label=jobs[0].label) as j:
        _check_ordered(j, refs[0])
    with env.ordered(jobs, label="two streams, one plan") as both:
        for j, r in zip(both, refs):
            _check_ordered(j, r)
