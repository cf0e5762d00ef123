"""CPU-only: the shifted CholeskyQR entries (cap_cacqr_shift; num_iter 1 ... 4 of cap_cacqr_plan_create; cacqr.factor_robust, info.shift) are
declared, bound, exported, documented and check their arguments before the library touches a device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "capital_amd.h")
SO = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")
OK, ARG, UNSUPPORTED = 0, 1, 4


def test_header_declares_and_ctypes_table_binds_the_shift_query():
    from capital_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+cap_cacqr_shift\s*\(([^)]*)\)\s*;", src)
    assert m, "cap_cacqr_shift is not declared in include/capital_amd.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 3 and args[0].startswith("cap_cacqr_plan*") and args[1].startswith("double*") and args[2].startswith("void*")
    res, argtypes = _lib.SIGNATURES["cap_cacqr_shift"]
    assert res is C.c_int and len(argtypes) == 3
    assert argtypes[0] is C.c_void_p and argtypes[1] is C.POINTER(C.c_double) and argtypes[2] is C.c_void_p


def test_header_comment_states_the_range_the_refusal_and_the_failure_mode():
    src = open(HEADER).read()
    plan = src[src.index("qr::cacqr<...>::info + factor, 1D path"):src.index("int cap_cacqr_plan_create(")]
    assert "1 ... 4" in plan and "CAP_ERR_ARG" in plan
    assert "info != 0" in plan and "never" in plan and "silently wrong Q" in plan
    assert "kappa" in plan and "2^13" in plan and "2^16" in plan and "2^21" in plan and "profiles/r10_scqr.txt" in plan
    assert "@" not in plan                                            # the measured examples are filled in
    grid = src[src.index("The 3D / tunable-grid path"):src.index("int cap_cacqr_plan_create_grid(")]
    assert "CAP_ERR_UNSUPPORTED" in grid and "num_iter 3 or 4" in grid
    shift = src[src.index("int cap_cacqr_info("):src.index("int cap_cacqr_shift(")]
    assert "0.0" in shift and "ynchronises" in shift


def test_python_mirror_has_factor_robust_and_shift():
    from capital_amd import cacqr
    sig = inspect.signature(cacqr.factor_robust)
    assert list(sig.parameters) == ["A", "args", "CommInfo", "max_iter"]
    assert sig.parameters["CommInfo"].default is None and sig.parameters["max_iter"].default == 4
    assert "bit-identical on every rank" in cacqr.factor_robust.__doc__
    assert list(inspect.signature(cacqr.info.shift).parameters) == ["self"]
    assert "AlapackPotrs" in cacqr.__doc__                             # documented as an extension, the way the solve is


def test_shift_before_any_factor_raises_in_python():
    from capital_amd import _lib, cacqr, cholinv
    for it in (2, 3, 4):
        pack = cacqr.info(it, cholinv.info(1, 1, 0, 'U'))
        assert pack.num_iter == it
        with pytest.raises(_lib.CapitalError):
            pack.shift()


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


def test_release_library_exports_the_entry(L):
    syms = subprocess.run(["nm", "-D", "--defined-only", SO], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert "cap_cacqr_shift" in set(line.split()[-1] for line in syms.splitlines() if line.strip())


def test_arguments_are_checked_first(L):
    """every call below returns before any device work"""
    h = C.c_void_p()
    for it in (0, 5, -1):
        assert L.cap_cacqr_plan_create(C.byref(h), 4096, 64, it, None) == ARG
        assert L.cap_cacqr_plan_create_grid(C.byref(h), 4096, 64, it, C.c_void_p(1 << 20)) == ARG
    for it in (3, 4):
        assert L.cap_cacqr_plan_create_grid(C.byref(h), 4096, 64, it, C.c_void_p(1 << 20)) == UNSUPPORTED
    v = C.c_double(0.0)
    assert L.cap_cacqr_shift(None, C.byref(v), None) == ARG
    assert L.cap_cacqr_shift(C.c_void_p(1 << 20), None, None) == ARG
