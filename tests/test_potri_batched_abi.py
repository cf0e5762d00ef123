"""CPU-only: argument handling of the batched triangular inverse and SPD inverse (cap_dtrtri_batched, cap_dpotri_batched) - the table of
tests/test_potrf_batched_blocked_abi.py for the two new symbols, plus the `fill` argument.  Every case of the table is decided before the
library touches a device.  The last test drives both entries through the recording stand-in of tests/hipshim in a process of its own (this
file run as a script): one launch per call, every launch annotated, no finding."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")
LOWER, UPPER = 0, 1
OK, ARG, UNSUPPORTED = 0, 1, 4
TRACE_N = (8, 64, 65, 256)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


A = C.c_void_p(1 << 20)                  # never dereferenced: every call below returns before any device work
INFO = C.c_void_p(1 << 31)


def entries(L):
    def trtri(uplo=UPPER, n=10, A=A, ld=10, stride=100, batch=5, info=INFO, fill=0):
        return L.cap_dtrtri_batched(uplo, n, A, ld, stride, batch, info, None)

    def potri(uplo=UPPER, n=10, A=A, ld=10, stride=100, batch=5, info=INFO, fill=0):
        return L.cap_dpotri_batched(uplo, n, A, ld, stride, batch, info, fill, None)
    return (trtri, potri)


@pytest.mark.parametrize("which", (0, 1))
def test_arguments_are_checked_first(L, which):
    call = entries(L)[which]
    n = 10
    assert call(n=-1) == ARG
    assert call(batch=-1) == ARG
    assert call(A=None) == ARG
    assert call(ld=n - 1) == ARG
    assert call(stride=n * n - 1) == ARG
    assert call(ld=n + 2, stride=(n + 2) * n - 1) == ARG
    assert call(stride=-1) == ARG
    assert call(n=257, ld=257, stride=257 * 257) == UNSUPPORTED
    assert call(n=257, ld=256, stride=257 * 257) == ARG             # the argument rules come first
    assert call(n=1 << 20, ld=1 << 20, stride=1 << 40) == UNSUPPORTED
    assert call(uplo=LOWER) == UNSUPPORTED
    assert call(uplo=LOWER, n=0, ld=0, stride=0) == UNSUPPORTED     # LOWER is refused before the empty case
    assert call(uplo=LOWER, ld=n - 1) == ARG
    assert call(uplo=LOWER, A=None) == ARG
    assert call(uplo=LOWER, n=257, ld=257, stride=257 * 257) == UNSUPPORTED
    # a batch beyond one grid dimension: refused on the workgroup-per-block path, after LOWER and n > 256, before the empty case matters
    assert call(n=65, ld=65, stride=65 * 65, batch=1 << 31) == UNSUPPORTED
    assert call(n=65, ld=64, stride=65 * 65, batch=1 << 31) == ARG
    assert call(n=257, ld=257, stride=257 * 257, batch=1 << 31) == UNSUPPORTED
    # degenerate sizes: nothing is launched, whatever the pointers
    assert call(n=0, A=None, ld=0, stride=0, info=None) == OK
    assert call(n=0) == OK
    assert call(batch=0, A=None, info=None) == OK
    assert call(batch=0, stride=0) == OK
    assert call(n=0, batch=0, A=None, ld=0, stride=0) == OK
    assert call(n=257, ld=257, stride=0, batch=0) == UNSUPPORTED    # n > 256 is refused for an empty batch too
    assert call(batch=0, A=None, stride=-5) == OK
    for big in (64, 65, 256):
        assert call(n=big, ld=big, stride=big * big, batch=0) == OK
        assert call(n=big, ld=big, stride=big * big, batch=0, A=None) == OK
        assert call(n=big, ld=big - 1, stride=big * big) == ARG
        assert call(n=big, ld=big, stride=big * big - 1) == ARG
        assert call(n=big, ld=big, stride=big * big, A=None) == ARG
        assert call(n=big, ld=big, stride=big * big, uplo=LOWER) == UNSUPPORTED


def test_fill_is_an_argument_rule(L):
    _, potri = entries(L)
    for fill in (2, -1, 255):
        assert potri(fill=fill) == ARG
        assert potri(fill=fill, uplo=LOWER) == ARG                   # before LOWER ...
        assert potri(fill=fill, n=257, ld=257, stride=257 * 257) == ARG      # ... before the size limit ...
        assert potri(fill=fill, batch=0) == ARG                      # ... and before the empty case
    for fill in (0, 1):
        assert potri(fill=fill, batch=0) == OK
        assert potri(fill=fill, uplo=LOWER) == UNSUPPORTED


def test_single_block_needs_no_stride(L):
    """batch = 1: the stride is not used and not checked; batch = 2 with the same stride is refused"""
    n = 100
    assert L.cap_dtrtri_batched(UPPER, n, A, n, 0, 2, None, None) == ARG
    assert L.cap_dpotri_batched(UPPER, n, A, n, 0, 2, None, 1, None) == ARG
    assert L.cap_dtrtri_batched(LOWER, n, A, n, 0, 1, None, None) == UNSUPPORTED        # passes the argument rules with stride 0 ...
    assert L.cap_dpotri_batched(LOWER, n, A, n, 0, 1, None, 0, None) == UNSUPPORTED
    assert L.cap_dtrtri_batched(LOWER, n, A, n, 0, 2, None, None) == ARG                # ... which two blocks do not
    assert L.cap_dpotri_batched(LOWER, n, A, n, 0, 2, None, 0, None) == ARG


def test_the_stride_rule_does_not_wrap(L):
    """ld * columns beyond int64 (2^60 * 16 = 2^64 wraps to 0): the stride rule compares with the clipped product, so two blocks at stride 0
    are refused like any other overlap - decided before any device work"""
    big = 1 << 60
    assert L.cap_dtrtri_batched(UPPER, 16, A, big, 0, 2, None, None) == ARG
    assert L.cap_dpotri_batched(UPPER, 16, A, big, 0, 2, None, 0, None) == ARG


def test_python_layer_names():
    from capital_amd import _lib, batched, lapack
    pt = lapack.ArgPack_trtri_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    pi = lapack.ArgPack_potri_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    assert pt.method == lapack.Method.AlapackTrtriBatched and pi.method == lapack.Method.AlapackPotriBatched
    assert callable(lapack.engine._trtri_batched) and callable(lapack.engine._potri_batched)
    assert callable(batched.trtri) and callable(batched.potri)
    for doc in (batched.trtri.__doc__, batched.potri.__doc__, lapack.engine._trtri_batched.__doc__, lapack.engine._potri_batched.__doc__):
        assert "256" in doc
    assert "LOWER triangle" in batched.potri.__doc__ and "torch.cholesky_inverse" in batched.potri.__doc__
    assert "symmetric=True" in batched.potri.__doc__ and "L^-1" in batched.trtri.__doc__
    for fn in (lapack.engine._trtri_batched, lapack.engine._potri_batched):
        with pytest.raises(_lib.CapitalError, match="256"):
            fn(None, 257, 257, 257 * 257, 1, None, pi)
    with open(os.path.join(ROOT, "include", "capital_amd.h")) as f:
        header = f.read()
    assert "cap_dtrtri_batched(" in header and "cap_dpotri_batched(" in header


def test_cpu_tensors_wrong_types_and_overlaps_are_refused():
    import torch
    from capital_amd import _lib, batched
    a = torch.eye(100, dtype=torch.float64).repeat(3, 1, 1)
    for fn in (batched.trtri, batched.potri):
        with pytest.raises(_lib.CapitalError):
            fn(a)
        with pytest.raises(_lib.CapitalError):
            fn(a.to(torch.float32))
        with pytest.raises(_lib.CapitalError):
            fn(torch.eye(4, dtype=torch.float64))


def test_one_annotated_launch_per_call_on_the_recording_stand_in(tmp_path):
    """both entries at n = 8, 64, 65, 256 with the caller on the NULL stream and on a stream of its own"""
    from capital_amd import build
    build.build(verbose=False)
    out = tmp_path / "trace.json"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    res = json.load(open(out))
    assert len(res) == 2 * len(TRACE_N)
    for x in res:
        assert not x["findings"], (x["name"], x["findings"][:4])
        assert x["stats"]["kernels"] == x["calls"] == 5 and not x["stats"].get("unannotated"), (x["name"], x["stats"])
        assert x["stats"]["oob"] == 0 and x["stats"].get("races", 0) == 0
        assert sorted(x["entries"]) == ["cap_dpotri_batched", "cap_dtrtri_batched"]
        assert all(k.startswith("K ") and ("potri_batched" in k) for k in x["launches"]), x["launches"]


def _trace_main(out_path):
    """runs in a process of its own (no torch: the stand-in takes the place of the HIP runtime)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipshim"))
    import run_scenarios as S
    results = []
    for user_stream in (0, 1):
        for n in TRACE_N:
            r = S.Run("potri batched n=%d%s" % (n, " [user stream]" if user_stream else " [NULL stream]"), user_stream)
            batch, ld = 37, n + 1
            T = S.dmalloc(8 * (ld * n * batch + 3 * (batch - 1)))
            info = S.dmalloc(4 * batch)
            calls = 0
            for fill, inf, stride in ((0, info, ld * n), (1, None, ld * n + 3)):
                S.ok(r.call("dtrtri_batched", S.L.cap_dtrtri_batched, 1, n, T, ld, stride, batch, inf, r.stream), "cap_dtrtri_batched")
                S.ok(r.call("dpotri_batched fill=%d" % fill, S.L.cap_dpotri_batched, 1, n, T, ld, stride, batch, inf, fill, r.stream), "cap_dpotri_batched")
                calls += 2
            S.ok(r.call("dpotri_batched one block", S.L.cap_dpotri_batched, 1, n, T, ld, 0, 1, None, 1, r.stream), "cap_dpotri_batched")
            calls += 1
            out = r.finish()
            out["calls"] = calls
            out["launches"] = [l for l in r.lines if l.startswith("K ")]
            for q in (T, info):
                S.shim.hipFree(q)
            results.append(out)
    json.dump(results, open(out_path, "w"))


if __name__ == "__main__":
    _trace_main(sys.argv[1])
