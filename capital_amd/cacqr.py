"""qr::cacqr mirror (reference src/alg/qr/cacqr/cacqr.h:18-55, cacqr.hpp:5-248).

    pack = cacqr.info(num_iter, cholinv.info(...))      # num_iter: 1 = CholeskyQR, 2 = CholeskyQR2
    cacqr.factor(A, pack, topo.rect(c))                 # A: local element-cyclic piece: rows over d, columns over c
    Q = cacqr.construct_Q(pack, topo); R = cacqr.construct_R(pack, topo)
    X = cacqr.solve(pack, B)                            # least squares min ||A X - B||: R^-1 (Q^T B); cacqr.apply_Qt(pack, B) = Q^T B

Extension (not in the reference, like lapack.AlapackPotrs): num_iter 3 and 4 are shifted CholeskyQR3 - one / two shifted, equilibrated sweeps
in front of CholeskyQR2 for matrices CholeskyQR2 alone cannot factor (kappa >~ 1e8; include/capital_amd.h states the supported region).  1D path
only.  `info.shift()` is the shift of the last factor call, `factor_robust` escalates num_iter 2 -> 3 -> 4 until the factorization succeeds.

c == 1 (cacqr.hpp:229, the shape of BASELINE config 4): the 1D path - rows cyclic over all ranks, one Gram all-reduce
per sweep.  c > 1: the 3D (c == d) / tunable-grid (d > c) path of cacqr.hpp:75-170 on the c x d x c grid of a
`topo.rect` bundle (csrc/cacqr.hip: sweep_grid)."""
import ctypes as C

import torch

from . import _lib
from ._util import cur_stream
from .matrix import matrix, rect


class info:
    def __init__(self, num_iter, cholesky_inverse_args=None):
        self.num_iter = int(num_iter)
        self.cholesky_inverse_args = cholesky_inverse_args
        self._plan = None
        self._shape = None
        self._grid = False
        self._plan_iter = None            # the num_iter the plan was created with (factor_robust changes num_iter)

    def _ensure(self, m_local, n, comm):
        if self._plan is not None and self._shape == (m_local, n) and not self._grid and self._plan_iter == self.num_iter:
            return
        self._release()
        h = C.c_void_p()
        _lib.check(_lib.lib().cap_cacqr_plan_create(C.byref(h), m_local, n, self.num_iter, comm), "cap_cacqr_plan_create")
        self._plan, self._shape, self._grid, self._plan_iter = h, (m_local, n), False, self.num_iter

    def _ensure_grid(self, A, topo):
        key = (A.num_rows_local(), A.num_columns_local())
        if self._plan is not None and self._shape == key and self._grid and self._plan_iter == self.num_iter:
            return
        self._release()
        h = C.c_void_p()
        _lib.check(_lib.lib().cap_cacqr_plan_create_grid(C.byref(h), A.num_rows_global(), A.num_columns_global(), self.num_iter,
                                                         topo.handle), "cap_cacqr_plan_create_grid")
        self._plan, self._shape, self._grid, self._plan_iter = h, key, True, self.num_iter

    def _release(self):
        if self._plan is not None:
            _lib.lib().cap_cacqr_plan_destroy(self._plan)
            self._plan = None

    def last_info(self):
        v = C.c_int64(0)
        _lib.check_info(_lib.lib().cap_cacqr_info(self._plan, cur_stream(), C.byref(v)), "cap_cacqr_info")
        return v.value

    def shift(self):
        """the shift s = 11 (m n + n (n + 1)) 2^-53 n of the last factor call (m: the global row count); 0.0 for num_iter <= 2"""
        if self._plan is None:
            raise _lib.CapitalError("cacqr: no factor call yet")
        v = C.c_double(0.0)
        _lib.check(_lib.lib().cap_cacqr_shift(self._plan, C.byref(v), cur_stream()), "cap_cacqr_shift")
        return v.value

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


def factor(A, args, CommInfo=None):
    """cacqr::factor (cacqr.hpp:217-248) for the c == 1 grid."""
    c = getattr(CommInfo, "c", 1) if CommInfo is not None else 1
    args._gm, args._gn = A.num_rows_global(), A.num_columns_global()
    if c != 1:
        if getattr(CommInfo, "handle", None) is None:
            raise _lib.CapitalError("the c > 1 CholeskyQR grids need a topo.rect bundle (sub-communicators)")
        args._ensure_grid(A, CommInfo)
        _lib.check(_lib.lib().cap_cacqr_factor(args._plan, A.data_ptr(), A.ld(), cur_stream()), "cacqr::factor")
        return
    comm = getattr(CommInfo, "world", None) if CommInfo is not None else None
    args._ensure(A.num_rows_local(), A.num_columns_local(), comm)
    _lib.check(_lib.lib().cap_cacqr_factor(args._plan, A.data_ptr(), A.ld(), cur_stream()), "cacqr::factor")


def factor_robust(A, args, CommInfo=None, max_iter=4):
    """factor with the cheapest variant that succeeds: `factor` with num_iter 2, then 3, then 4, until last_info() == 0.  Returns the num_iter
    it ended on (args.num_iter is set to it) and leaves `args` usable by solve, apply_Qt, construct_Q and construct_R; raises CapitalError when
    max_iter is exhausted.  Each attempt reads info back (one host synchronisation per attempt).  On several ranks every rank takes the same
    decision without talking to the others: the all-reduced Gram matrix, and with it every pivot and `info`, is bit-identical on every rank.
    1D path only (the grid plans refuse num_iter > 2)."""
    last = None
    for it in range(2, int(max_iter) + 1):
        args.num_iter = it
        factor(A, args, CommInfo)
        last = args.last_info()
        if last == 0:
            return it
    raise _lib.CapitalError("cacqr::factor_robust: no factorization up to num_iter = %d (last info %s)" % (int(max_iter), last))


def construct_Q(args, CommInfo=None):
    """cacqr.hpp construct_Q: fresh rect matrix with this rank's row-cyclic piece of Q."""
    m_local, n = args._shape
    d = getattr(CommInfo, "d", 1) if CommInfo is not None else 1
    c = getattr(CommInfo, "c", 1) if CommInfo is not None else 1
    out = matrix(args._gn, args._gm, c, d, rect)
    ld = C.c_int64(0)
    q = _lib.lib().cap_cacqr_Q_ptr(args._plan, C.byref(ld))
    st = _lib.lib().cap_copy_window(q, 0, ld.value, 0, 0, out.data_ptr(), 0, out.ld(), 0, 0, m_local, n, 0, 0, cur_stream())
    _lib.check(st, "construct_Q")
    return out


def construct_R(args, CommInfo=None):
    """the caller's piece of R: the whole n x n factor on the 1D grid, the c x c element-cyclic piece (rows y mod c, columns
    x mod c) on the 3D / tunable grids - what upstream's args.R holds (cacqr.hpp:214)."""
    if args._grid:
        c = CommInfo.c
        out = matrix(args._gn, args._gn, c, c, rect)
        _lib.check(_lib.lib().cap_cacqr_R_piece(args._plan, out.data_ptr(), out.ld(), cur_stream()), "construct_R")
        return out
    m_local, n = args._shape
    out = matrix(n, n, 1, 1, rect)
    ld = C.c_int64(0)
    r = _lib.lib().cap_cacqr_R_ptr(args._plan, C.byref(ld))
    st = _lib.lib().cap_copy_window(r, 0, ld.value, 0, 0, out.data_ptr(), 0, out.ld(), 0, 0, n, n, 1, 1, cur_stream())
    _lib.check(st, "construct_R")
    return out


def dense_R(args):
    """the replicated dense n x n R (device view) - grid and 1D plans alike."""
    n = args._gn
    ld = C.c_int64(0)
    r = _lib.lib().cap_cacqr_R_ptr(args._plan, C.byref(ld))
    out = matrix(n, n, 1, 1, rect)
    st = _lib.lib().cap_copy_window(r, 0, ld.value, 0, 0, out.data_ptr(), 0, out.ld(), 0, 0, n, n, 1, 1, cur_stream())
    _lib.check(st, "dense_R")
    return out


def _rhs(args, B):
    """(address, leading dimension, nrhs) of the local m_local x nrhs piece of the right-hand sides: a `matrix`, or a device tensor of shape
    (m_local,) / (m_local, nrhs) - used in place when it is column-major, through a column-major copy otherwise"""
    if args._plan is None:
        raise _lib.CapitalError("cacqr: no factor call yet (nothing to apply or solve with)")
    m_local = args._shape[0]
    if isinstance(B, matrix):
        if B.num_rows_local() != m_local:
            raise _lib.CapitalError("right-hand sides have %d local rows, the factored matrix %d" % (B.num_rows_local(), m_local))
        return B.data_ptr(), B.ld(), B.num_columns_local(), B
    if not isinstance(B, torch.Tensor) or B.device.type != "cuda" or B.dtype != torch.float64:
        raise _lib.CapitalError("right-hand sides must be a matrix or an fp64 device tensor; no CPU path")
    t = B.reshape(-1, 1) if B.dim() == 1 else B
    if t.dim() != 2 or t.shape[0] != m_local:
        raise _lib.CapitalError("right-hand sides must be (m_local,) or (m_local, nrhs) with m_local = %d" % m_local)
    if not (t.stride(0) == 1 and (t.shape[1] == 1 or t.stride(1) >= m_local)):
        t = t.t().contiguous().t()                      # column-major copy, ld = m_local
    return t.data_ptr(), (t.stride(1) if t.shape[1] > 1 else max(m_local, 1)), t.shape[1], t


def _apply(entry, what, args, B):
    b, ldb, nrhs, keep = _rhs(args, B)
    n = args._shape[1] if not args._grid else args._gn
    out = matrix(nrhs, n, 1, 1, rect)
    _lib.check(getattr(_lib.lib(), entry)(args._plan, b, ldb, nrhs, out.data_ptr(), out.ld(), cur_stream()), what)
    del keep
    return out


def apply_Qt(args, B, CommInfo=None):
    """Z = Q^T B of the last factor call (cap_cacqr_apply_qt): B is this rank's m_local x nrhs piece of the right-hand sides (rows
    distributed like A's), the result a fresh replicated n x nrhs matrix.  1D plans only."""
    return _apply("cap_cacqr_apply_qt", "cacqr::apply_Qt", args, B)


def solve(args, B, CommInfo=None):
    """X = argmin ||A X - B||_F = R^-1 (Q^T B) of the last factor call (cap_cacqr_solve), a fresh replicated n x nrhs matrix; all NaN
    when the factorization failed (last_info() != 0).  1D plans only."""
    return _apply("cap_cacqr_solve", "cacqr::solve", args, B)
