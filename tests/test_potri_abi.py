"""CPU-only: argument handling of the SPD inverse / log-determinant entry points (cap_dlauum, cap_dpotri, cap_cholinv_inverse,
cap_cholinv_logdet) - every case here is decided before the library touches a device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")
LOWER, UPPER = 0, 1
OK, ARG, UNSUPPORTED = 0, 1, 4


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


def test_work_size(L):
    assert L.cap_dpotri_work_size(0) == 0
    for n in (1000, 65536):
        assert L.cap_dpotri_work_size(n) >= n * n          # an n x n inverse + TRTRI's own scratch
    sizes = [L.cap_dpotri_work_size(n) for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 1001, 4096, 16384, 65536)]
    assert sizes == sorted(sizes) and sizes[1] > 0


def test_arguments_are_checked_first(L):
    fake = C.c_void_p(1 << 20)           # never dereferenced: every call below returns before any device work
    far = C.c_void_p(1 << 30)            # a second window that does not overlap the first for n = 10
    n = 10
    # cap_dlauum
    assert L.cap_dlauum(UPPER, -1, fake, n, far, n, None) == ARG
    assert L.cap_dlauum(UPPER, n, fake, n - 1, far, n, None) == ARG
    assert L.cap_dlauum(UPPER, n, fake, n, far, n - 1, None) == ARG
    assert L.cap_dlauum(UPPER, n, None, n, far, n, None) == ARG
    assert L.cap_dlauum(UPPER, n, fake, n, None, n, None) == ARG
    assert L.cap_dlauum(UPPER, n, fake, n, fake, n, None) == ARG                               # in place
    assert L.cap_dlauum(UPPER, n, fake, n, C.c_void_p((1 << 20) + 8 * (9 * n + 9)), n, None) == ARG   # C starts on W's last element
    assert L.cap_dlauum(UPPER, n, C.c_void_p((1 << 20) + 8 * (9 * n + 9)), n, fake, n, None) == ARG   # ... and the other way round
    assert L.cap_dlauum(LOWER, n, fake, n, fake, n, None) == ARG                               # ARG before UNSUPPORTED
    assert L.cap_dlauum(LOWER, n, fake, n, far, n, None) == UNSUPPORTED
    assert L.cap_dlauum(UPPER, 0, fake, 1, fake, 1, None) == OK
    # cap_dpotri
    assert L.cap_dpotri(UPPER, -1, fake, n, far, None) == ARG
    assert L.cap_dpotri(UPPER, n, fake, n - 1, far, None) == ARG
    assert L.cap_dpotri(UPPER, n, None, n, far, None) == ARG
    assert L.cap_dpotri(UPPER, n, fake, n, None, None) == ARG
    assert L.cap_dpotri(LOWER, n, fake, n, far, None) == UNSUPPORTED
    assert L.cap_dpotri(UPPER, 0, fake, 1, far, None) == OK
    # the plan calls
    for fill in (0, 1, 2, -1):
        assert L.cap_cholinv_inverse(None, fake, n, fill, None) == ARG
    assert L.cap_cholinv_logdet(None, fake, None) == ARG
