"""cholesky::cholinv mirror (reference src/alg/cholesky/cholinv/cholinv.h:16-53, cholinv.hpp:6-46).

    pack = cholinv.info(complete_inv, split, bc_mult_dim, 'U')     # plan handle (create once)
    cholinv.factor(A, pack, topo)                                   # A: matrix (read-only)
    R = cholinv.construct_R(pack, topo); Rinv = cholinv.construct_Rinv(pack, topo)
    X = cholinv.solve(B, pack)                                      # A X = B with the factor of the last factor call
    Ainv = cholinv.inverse(pack); ld = cholinv.logdet(pack)         # A^-1 = R^-1 R^-T and log det A = 2 sum log r_ii of that factor
    cholinv.update(V, pack); cholinv.downdate(V, pack)              # the resident factor follows A + V V^T / A - V V^T (V: n x k, k << n)
    f = cholinv.factor_pivoted(A, max_rank, tol)                    # semidefinite / low-rank A: A[piv][:, piv] ~ R^T R, f.rank (no plan)
    rc = cholinv.rcond(A, pack)                                     # LAPACK dpocon: 1 / (||A||_1 est ||A^-1||_1) of that factor (a float)
    ferr, berr = cholinv.error_bounds(A, B, X, pack)                # LAPACK dporfs' bounds per column of a computed solution X
    a1 = cholinv.norm1(A)                                           # ||A||_1 of a symmetric A from its upper triangle (device scalar)

`info` keeps upstream's four user knobs.  complete_inv = -1 is the documented extension:
blocked right-looking Cholesky (real TRSM/SYRK, no explicit inverse) - the headline
"fp64 Cholesky" path; 0 / 1 reproduce upstream's R + R^-1 semantics."""
import ctypes as C

import torch

from . import _lib
from ._util import cur_stream
from .matrix import matrix, rect


class info:
    def __init__(self, complete_inv, split, bc_mult_dim, dir='U'):
        self.complete_inv, self.split, self.bc_mult_dim, self.dir = int(complete_inv), int(split), int(bc_mult_dim), dir
        self._plan = None
        self._n = None
        self._comm = None
        self.options = {}

    def set_option(self, key, value):
        """GPU-schedule knobs: nb (panel width), leaf (<= 64), lookahead (0/1)."""
        self.options[key] = int(value)
        if self._plan:
            _lib.check(_lib.lib().cap_cholinv_set_option(self._plan, key.encode(), int(value)), "set_option")

    def get_option(self, key):
        if not self._plan:
            return self.options.get(key)
        return _lib.lib().cap_cholinv_get_option(self._plan, key.encode())

    def _ensure(self, n, comm=None):
        if self._plan is not None and self._n == n and self._comm == comm:
            return
        self._release()
        L = _lib.lib()
        h = C.c_void_p()
        # args.R/_Rinv._register_: allocated once, later calls are no-ops (cholinv.hpp:11-12)
        _lib.check(L.cap_cholinv_plan_create(C.byref(h), n, self.complete_inv, self.split, self.bc_mult_dim,
                                             self.dir.encode()[0:1], comm), "cap_cholinv_plan_create")
        self._plan, self._n, self._comm = h, n, comm
        order = sorted(self.options.items(), key=lambda kv: kv[0] == "cyclic_c")      # the layout follows the block width: "nb" first
        for k, v in order:
            _lib.check(L.cap_cholinv_set_option(self._plan, k.encode(), v), "set_option")

    def _release(self):
        if self._plan is not None:
            _lib.lib().cap_cholinv_plan_destroy(self._plan)
            self._plan = None

    def last_info(self):
        """0, or the 1-based index of the first non-positive pivot (upstream drops this, lapack/interface.hpp:39)."""
        v = C.c_int64(0)
        _lib.check_info(_lib.lib().cap_cholinv_info(self._plan, cur_stream(), C.byref(v)), "cap_cholinv_info")
        return v.value

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


def factor(A, args, CommInfo=None):
    """cholinv::factor (cholinv.hpp:6-28). Asynchronous on the current stream."""
    if args.dir != 'U':
        raise _lib.CapitalError("dir must be 'U' (upstream asserts the same, cholinv.hpp:9)")
    if args.split <= 0:
        raise _lib.CapitalError("split must be > 0 (cholinv.hpp:9)")
    if CommInfo is not None and getattr(CommInfo, "size", 1) != 1:
        # multi-GPU: the 1 x P schedule of csrc/dist.hip runs behind the same plan handle (complete_inv = 0 / 1 add R^-1).
        #  * A created on the d x d grid of a topo::square bundle (matrix(n, n, d, d), bench/cholesky/cholinv.cpp:34-35): the
        #    REFERENCE's layout - A is this rank's element-cyclic piece, construct_R / construct_Rinv return pieces of the same
        #    shape on every rank (option "cyclic_c": distributed redistribution in front of / behind the plan, csrc/redist.hip);
        #  * A on a 1 x 1 grid: this rank's block columns (all n rows), construct_* return block columns.
        n = A.num_rows_global()
        d = getattr(CommInfo, "d", 1)
        args._cyclic = (d > 1 and A._pgridX == d and A._pgridY == d)
        args.options["cyclic_c"] = int(getattr(CommInfo, "c", 1)) if args._cyclic else 0
        args._grid_d = d
        args._ensure(n, getattr(CommInfo, "world", None))
        args.set_option("cyclic_c", args.options["cyclic_c"])          # (a reused plan follows the layout of THIS call's A)
        _lib.check(_lib.lib().cap_cholinv_factor(args._plan, A.data_ptr(), A.ld(), cur_stream()), "cholinv::factor")
        return
    n = A.num_rows_global()
    if n != A.num_columns_global():
        raise _lib.CapitalError("cholinv needs a square matrix")
    args._ensure(n)
    _lib.check(_lib.lib().cap_cholinv_factor(args._plan, A.data_ptr(), A.ld(), cur_stream()), "cholinv::factor")


def _construct(args, which):
    n = args._n
    if args._comm is not None and _lib.lib().cap_comm_size(args._comm) > 1 and getattr(args, "_cyclic", False):
        out = matrix(n, n, args._grid_d, args._grid_d, rect)      # my element-cyclic piece, like upstream's construct_R
    elif args._comm is not None and _lib.lib().cap_comm_size(args._comm) > 1:
        lc = int(_lib.lib().cap_cholinv_get_option(args._plan, b"local_cols"))
        out = matrix(max(lc, 1), n, 1, 1, rect)      # my block-cyclic columns (n x local_cols)
    else:
        out = matrix(n, n, 1, 1, rect)
    fn = _lib.lib().cap_cholinv_get_R if which == "R" else _lib.lib().cap_cholinv_get_Rinv
    _lib.check(fn(args._plan, out.data_ptr(), out.ld(), cur_stream()), "construct_" + which)
    return out


def construct_R(args, CommInfo=None):
    """cholinv.hpp:30-37: fresh rect matrix holding the upper-triangular factor."""
    return _construct(args, "R")


def construct_Rinv(args, CommInfo=None):
    """cholinv.hpp:39-46."""
    return _construct(args, "Rinv")


def solve(B, args, X=None):
    """A X = B with the factor `cholinv.factor` left in `args` (single-GPU plans; the reference's trsm::diaginvert is a stub).
    B: n x nrhs matrix (not written unless X is B); X: a matrix of the same shape, or None for a new one.  Asynchronous on the
    current stream.  A failing pivot of the last factor call leaves X NaN (args.last_info() reports it)."""
    if args._plan is None:
        raise _lib.CapitalError("cholinv.solve needs a plan that cholinv.factor has filled")
    n, nrhs = B.num_rows_global(), B.num_columns_global()
    if n != args._n:
        raise _lib.CapitalError("B has %d rows, the factor is %d x %d" % (n, args._n, args._n))
    if X is None:
        X = matrix(nrhs, n, 1, 1, rect)
    elif X.num_rows_global() != n or X.num_columns_global() != nrhs:
        raise _lib.CapitalError("X must be %d x %d" % (n, nrhs))
    _lib.check(_lib.lib().cap_cholinv_solve(args._plan, B.data_ptr(), B.ld(), X.data_ptr(), X.ld(), nrhs, cur_stream()),
               "cholinv::solve")
    return X


def inverse(args, out=None, fill=True):
    """A^-1 = R^-1 R^-T of the factor `cholinv.factor` left in `args` (single-GPU plans, any complete_inv; not in the reference, which
    stops at R and R^-1).  out: an n x n matrix, or None for a new one.  fill=True: both triangles; fill=False: only the upper triangle
    of `out` is written.  Asynchronous on the current stream.  complete_inv = 0 / -1 plans keep an n x n inverse of R from the first
    call after a factor call on.  A failing pivot of the last factor call leaves the written window NaN (args.last_info() reports it)."""
    if args._plan is None:
        raise _lib.CapitalError("cholinv.inverse needs a plan that cholinv.factor has filled")
    n = args._n
    if out is None:
        out = matrix(n, n, 1, 1, rect)
    elif out.num_rows_global() != n or out.num_columns_global() != n:
        raise _lib.CapitalError("out must be %d x %d" % (n, n))
    _lib.check(_lib.lib().cap_cholinv_inverse(args._plan, out.data_ptr(), out.ld(), 1 if fill else 0, cur_stream()), "cholinv::inverse")
    return out


def logdet(args):
    """log det A = 2 sum log r_ii of the last factor call as a Python float (NaN when that factor failed).  The sum is formed on the
    device in a fixed order; returning it to the host SYNCHRONISES the current stream."""
    if args._plan is None:
        raise _lib.CapitalError("cholinv.logdet needs a plan that cholinv.factor has filled")
    out = torch.empty(1, dtype=torch.float64, device=torch.device("cuda", torch.cuda.current_device()))
    _lib.check(_lib.lib().cap_cholinv_logdet(args._plan, out.data_ptr(), cur_stream()), "cholinv::logdet")
    return float(out.item())


def norm1(A):
    """||A||_1 = max_j sum_i |a_ij| of the symmetric `matrix` A, read from its upper triangle alone (LAPACK dlansy, cap_dlansy), as a
    1-element fp64 device tensor.  Asynchronous on the current stream.  A NaN in the upper triangle gives NaN."""
    n = A.num_rows_global()
    if n != A.num_columns_global():
        raise _lib.CapitalError("norm1 needs a square matrix")
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    out = torch.empty(1, dtype=torch.float64, device=dev)
    work = torch.empty(max(int(L.cap_dlansy_work_size(n)), 2), dtype=torch.float64, device=dev)
    _lib.check(L.cap_dlansy(ord('1'), 1, n, A.data_ptr(), A.ld(), out.data_ptr(), work.data_ptr(), cur_stream()), "cholinv::norm1")
    return out


def rcond(A_or_anorm, args):
    """Reciprocal condition number 1 / (||A||_1 est ||A^-1||_1) of the matrix whose factor `cholinv.factor` (or `update`) left in `args`,
    by LAPACK's dpocon estimator on the device (cap_cholinv_rcond), as a Python float; returning it to the host SYNCHRONISES the current
    stream.  A_or_anorm: the `matrix` A itself (its upper triangle is read for the norm), or ||A||_1 as a 1-element fp64 device tensor
    (`norm1`) or a float.  The plan does not keep A: passing the matrix or norm that matches the resident factor is the caller's business.
    0.0 when the last factor or downdate failed (args.last_info() reports it), as LAPACK's dposvx."""
    if args._plan is None:
        raise _lib.CapitalError("cholinv.rcond needs a plan that cholinv.factor has filled")
    dev = torch.device("cuda", torch.cuda.current_device())
    out = torch.empty(1, dtype=torch.float64, device=dev)
    L = _lib.lib()
    if isinstance(A_or_anorm, matrix):
        A = A_or_anorm
        if A.num_rows_global() != args._n or A.num_columns_global() != args._n:
            raise _lib.CapitalError("A must be %d x %d" % (args._n, args._n))
        st = L.cap_cholinv_rcond(args._plan, A.data_ptr(), A.ld(), None, out.data_ptr(), cur_stream())
    else:
        if isinstance(A_or_anorm, torch.Tensor):
            an = A_or_anorm.reshape(-1)
            if an.numel() != 1 or an.dtype != torch.float64 or an.device.type != "cuda":
                raise _lib.CapitalError("the norm must be a float or a 1-element fp64 device tensor")
        else:
            an = torch.full((1,), float(A_or_anorm), dtype=torch.float64, device=dev)
        st = L.cap_cholinv_rcond(args._plan, None, 0, an.data_ptr(), out.data_ptr(), cur_stream())
    _lib.check(st, "cholinv::rcond")
    return float(out.item())


def error_bounds(A, B, X, args):
    """(ferr, berr): per column of the computed solution X of A X = B the forward error bound and the componentwise backward error of
    LAPACK's dporfs, without its refinement (cap_cholinv_error_bounds), as fp64 device tensors of nrhs entries.  A: the `matrix` whose
    factor is in `args` (upper triangle read; the plan does not keep A - the match is the caller's business), B, X: n x nrhs matrices.
    Asynchronous on the current stream.  NaN in both when the last factor or downdate failed."""
    if args._plan is None:
        raise _lib.CapitalError("cholinv.error_bounds needs a plan that cholinv.factor has filled")
    n, nrhs = B.num_rows_global(), B.num_columns_global()
    if n != args._n or A.num_rows_global() != n or A.num_columns_global() != n:
        raise _lib.CapitalError("A must be %d x %d and B have %d rows" % (args._n, args._n, args._n))
    if X.num_rows_global() != n or X.num_columns_global() != nrhs:
        raise _lib.CapitalError("X must be %d x %d" % (n, nrhs))
    dev = torch.device("cuda", torch.cuda.current_device())
    ferr = torch.empty(nrhs, dtype=torch.float64, device=dev)
    berr = torch.empty(nrhs, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().cap_cholinv_error_bounds(args._plan, A.data_ptr(), A.ld(), B.data_ptr(), B.ld(), X.data_ptr(), X.ld(), nrhs,
                                                   ferr.data_ptr(), berr.data_ptr(), cur_stream()), "cholinv::error_bounds")
    return ferr, berr


def _thin(args, V):
    """(address, leading dimension, k, keep-alive) of the n x k matrix V: a `matrix`, or an fp64 device tensor of shape (n,) / (n, k) - used
    in place when it is column-major, through a column-major copy otherwise"""
    n = args._n
    if isinstance(V, matrix):
        if V.num_rows_global() != n:
            raise _lib.CapitalError("V has %d rows, the factor is %d x %d" % (V.num_rows_global(), n, n))
        return V.data_ptr(), V.ld(), V.num_columns_global(), V
    if not isinstance(V, torch.Tensor) or V.device.type != "cuda" or V.dtype != torch.float64:
        raise _lib.CapitalError("V must be a matrix or an fp64 device tensor; no CPU path")
    t = V.reshape(-1, 1) if V.dim() == 1 else V
    if t.dim() != 2 or t.shape[0] != n:
        raise _lib.CapitalError("V must be (n,) or (n, k) with n = %d" % n)
    if not (t.stride(0) == 1 and (t.shape[1] == 1 or t.stride(1) >= n)):
        t = t.t().contiguous().t()                      # column-major copy, ld = n
    return t.data_ptr(), (t.stride(1) if t.shape[1] > 1 else max(n, 1)), t.shape[1], t


def update(V, args, sign=+1):
    """The resident factor of the last `cholinv.factor` becomes that of A + sign V V^T (sign = +1 / -1; LINPACK's dchud / dchdd) in
    2 k n^2 flops instead of a new factorization.  V: n x k `matrix` or fp64 device tensor of shape (n,) / (n, k), not written.
    Single-GPU plans with complete_inv = -1.  Asynchronous on the current stream; later solve / inverse / logdet calls use the new
    factor.  A downdate that leaves the matrix indefinite reports its row through args.last_info(); the factor is lost then."""
    if args._plan is None:
        raise _lib.CapitalError("cholinv.update needs a plan that cholinv.factor has filled")
    if sign not in (1, -1):
        raise _lib.CapitalError("sign must be +1 or -1")
    v, ldv, k, keep = _thin(args, V)
    _lib.check(_lib.lib().cap_cholinv_update(args._plan, int(sign), v, ldv, k, cur_stream()), "cholinv::update")
    del keep


def downdate(V, args):
    """`update` with sign = -1: the factor of A - V V^T."""
    update(V, args, sign=-1)


class pivoted_factor:
    """What `factor_pivoted` returns: R (a `matrix` of max_rank rows by n columns, None when max_rank = 0) and piv (int64 device tensor:
    the pivots in order, then the unselected indices in increasing order) with A[piv][:, piv] ~ R^T R.  rank, info (0: stopped at a
    pivot <= tol, 1: max_rank steps done with the remainder above tol, 2: a NaN on the remaining diagonal) and residual_trace
    (trace(A - R^T R)) are read from the device on first use, which synchronises."""

    def __init__(self, R, piv, out):
        self.R, self.piv, self._out, self._host = R, piv, out, None

    def _read(self):
        if self._host is None:
            rank, resid, info = self._out
            self._host = (int(rank.item()), int(info.item()), float(resid.item()))
        return self._host

    rank = property(lambda self: self._read()[0])
    info = property(lambda self: self._read()[1])
    residual_trace = property(lambda self: self._read()[2])


def factor_pivoted(A, max_rank=None, tol=-1.0):
    """Pivoted Cholesky (LAPACK's dpstrf with a rank cap, cap_dpstrf) of the symmetric positive semidefinite `matrix` A, whose upper
    triangle is read and which is not written: at most max_rank (None: n) left-looking steps, stopping at the first pivot <= tol
    (tol < 0: n eps max_i a_ii; otherwise absolute).  O(n rank^2) work, no plan.  Asynchronous on the current stream until rank, info
    or residual_trace of the returned `pivoted_factor` is read."""
    n = A.num_rows_global()
    if n != A.num_columns_global():
        raise _lib.CapitalError("factor_pivoted needs a square matrix")
    max_rank = n if max_rank is None else int(max_rank)
    if not 0 <= max_rank <= n:
        raise _lib.CapitalError("max_rank must be in [0, n]")
    L = _lib.lib()
    R = matrix(n, max_rank, 1, 1, rect, device=A.device) if max_rank > 0 else None
    piv = torch.empty(n, dtype=torch.int64, device=A.device)
    rank = torch.zeros(1, dtype=torch.int64, device=A.device)
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    resid = torch.zeros(1, dtype=torch.float64, device=A.device)
    work = torch.empty(max(int(L.cap_dpstrf_work_size(n, max_rank)), 2), dtype=torch.float64, device=A.device)
    _lib.check(L.cap_dpstrf(1, n, max_rank, float(tol), A.data_ptr(), A.ld(), R.data_ptr() if R is not None else None,
                            R.ld() if R is not None else 1, piv.data_ptr(), rank.data_ptr(), resid.data_ptr(), info.data_ptr(),
                            work.data_ptr(), cur_stream()), "cholinv::factor_pivoted")
    out = pivoted_factor(R, piv, (rank, resid, info))
    out._work = work            # stays alive until the stream has used it (the caching allocator is stream-ordered; this is the belt)
    return out
