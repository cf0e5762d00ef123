"""CPU-only: argument handling of the fp64 solve entry points (cap_cholinv_solve, cap_dpotrs, the recovery hook) - every case here
is decided before the library touches a device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


def test_work_sizes(L):
    assert L.cap_dpotrs_work_size(0, 4) == 0 and L.cap_dpotrs_work_size(100, 0) == 0
    # one-launch path (nrhs <= 16): the 128-wide block inverses + Y and the partial sums; blocked path: the inverses at cap_dtrsm's width
    assert L.cap_dpotrs_work_size(1000, 16) >= 8 * 128 * 128 + 2 * 1024 * 16
    assert L.cap_dpotrs_work_size(65536, 64) >= 128 * 512 * 512 + 512 * 64
    assert L.cap_dpotrs_work_size(4096, 8) < L.cap_dpotrs_work_size(4096, 16)


def test_arguments_are_checked_first(L):
    fake = C.c_void_p(4096)          # never dereferenced: every call below returns before any device work
    assert L.cap_cholinv_solve(None, fake, 10, fake, 10, 1, None) == 1
    assert L.cap_dpotrs(0, 10, 1, fake, 10, fake, 10, fake, None) == 4          # uplo = LOWER, as cap_dpotrf
    assert L.cap_dpotrs(1, -1, 1, fake, 10, fake, 10, fake, None) == 1
    assert L.cap_dpotrs(1, 10, 1, fake, 9, fake, 10, fake, None) == 1
    assert L.cap_dpotrs(1, 10, 1, None, 10, fake, 10, fake, None) == 1
    assert L.cap_dpotrs(1, 0, 3, fake, 1, fake, 1, fake, None) == 0
    assert L.cap_dpotrs(1, 10, 0, fake, 10, fake, 10, fake, None) == 0
    assert L.cap_solve_inject_timeouts(-1) == 1
