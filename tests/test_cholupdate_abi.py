"""CPU-only: argument handling of the Cholesky update / downdate entry points (cap_dcholupdate, cap_dcholupdate_work_size,
cap_cholinv_update) - every case here is decided before the library touches a device."""
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
    for n, k in ((0, 0), (0, 5), (5, 0), (0, 16)):
        assert L.cap_dcholupdate_work_size(n, k) == 0
    ns = (1, 2, 63, 64, 65, 127, 128, 129, 1000, 1001, 4096, 16384, 65536)
    ks = (1, 2, 5, 15, 16, 17, 40, 64, 1000)
    for k in ks:
        sizes = [L.cap_dcholupdate_work_size(n, k) for n in ns]
        assert sizes == sorted(sizes) and sizes[0] > 0, "not monotone in n at k = %d" % k
    for n in ns:
        sizes = [L.cap_dcholupdate_work_size(n, k) for k in ks]
        assert sizes == sorted(sizes) and sizes[0] > 0, "not monotone in k at n = %d" % n
        for k in (16, 17, 64):
            assert L.cap_dcholupdate_work_size(n, k) >= 16 * n          # the working copy of 16 columns of V


def test_arguments_are_checked_first(L):
    fake = C.c_void_p(1 << 20)           # never dereferenced: every call below returns before any device work
    far = C.c_void_p(1 << 30)
    wrk = C.c_void_p(1 << 32)
    n, k = 10, 3
    assert L.cap_dcholupdate(UPPER, 1, -1, k, fake, n, far, n, None, wrk, None) == ARG
    assert L.cap_dcholupdate(UPPER, 1, n, -1, fake, n, far, n, None, wrk, None) == ARG
    assert L.cap_dcholupdate(UPPER, 1, n, k, None, n, far, n, None, wrk, None) == ARG
    assert L.cap_dcholupdate(UPPER, 1, n, k, fake, n, None, n, None, wrk, None) == ARG
    assert L.cap_dcholupdate(UPPER, 1, n, k, fake, n, far, n, None, None, None) == ARG
    assert L.cap_dcholupdate(UPPER, 1, n, k, fake, n - 1, far, n, None, wrk, None) == ARG
    assert L.cap_dcholupdate(UPPER, 1, n, k, fake, n, far, n - 1, None, wrk, None) == ARG
    for sign in (0, 2, -2, 3):
        assert L.cap_dcholupdate(UPPER, sign, n, k, fake, n, far, n, None, wrk, None) == ARG
        assert L.cap_dcholupdate(UPPER, sign, 0, 0, fake, n, far, n, None, wrk, None) == ARG
    for sign in (1, -1):
        assert L.cap_dcholupdate(LOWER, sign, n, k, fake, n, far, n, None, wrk, None) == UNSUPPORTED
        assert L.cap_dcholupdate(LOWER, sign, n, k, fake, n - 1, far, n, None, wrk, None) == ARG       # ARG before UNSUPPORTED
        assert L.cap_dcholupdate(LOWER, sign, n, k, None, n, far, n, None, wrk, None) == ARG
        assert L.cap_dcholupdate(LOWER, 0, n, k, fake, n, far, n, None, wrk, None) == ARG
        assert L.cap_dcholupdate(LOWER, sign, 0, k, None, 0, None, 0, None, None, None) == UNSUPPORTED   # ... and UNSUPPORTED before the empty case
        assert L.cap_dcholupdate(UPPER, sign, 0, k, None, 0, None, 0, None, None, None) == OK
        assert L.cap_dcholupdate(UPPER, sign, n, 0, None, 0, None, 0, None, None, None) == OK
        assert L.cap_dcholupdate(UPPER, sign, 0, 0, fake, 1, far, 1, fake, wrk, None) == OK
    # the plan call
    for sign in (1, -1, 0, 2):
        assert L.cap_cholinv_update(None, sign, far, n, k, None) == ARG
    assert L.cap_cholinv_update(None, 1, None, n, 0, None) == ARG
    # the diagnostics' argument
    assert L.cap_update_inject_timeouts(-1) == ARG
