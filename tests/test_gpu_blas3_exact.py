"""-m gpu: every fp64 GEMM / SYRK / TRMM kernel path of csrc/gemm.hip against EXACT results.

The rows of tests/blas3_cases.py (tests/test_blas3_paths.py shows, without a GPU, which kernel instance each of them launches) through
blas.engine._gemm / _syrk / _trmm.  Operands are small nonzero integers, so a float64 NumPy product is the exact result whatever the
summation order and the device must reproduce it bit for bit - "one 16 x 16 block skipped one K step it should not have" changes an
integer, it cannot hide in rounding.  Everything the call must not write holds NaNs (pad rows, the other triangle of a SYRK C, the
unreferenced triangle of a TRMM operand, all of C for beta == 0) and whole buffers are compared as int64, so a NaN that moved or leaked
fails like a wrong element.  There is no tolerance in this file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import blas3_cases as T  # noqa: E402
from tests.gpu_util import DEV  # noqa: E402


def _blas():
    from capital_amd import blas
    return blas


def _call(blas, c, alpha, beta, ptr, ld):
    order = blas.Order.AblasColumnMajor
    tr = {"N": blas.Transpose.AblasNoTrans, "T": blas.Transpose.AblasTrans}
    if c.op == "gemm":
        blas.engine._gemm(ptr["A"], ptr["B"], ptr["C"], c.m, c.n, c.k, ld["A"], ld["B"], ld["C"], blas.ArgPack_gemm(order, tr[c.form[0]], tr[c.form[1]], alpha, beta))
    elif c.op == "syrk":
        uplo = blas.UpLo.AblasUpper if c.form[0] == "U" else blas.UpLo.AblasLower
        blas.engine._syrk(ptr["A"], ptr["C"], c.n, c.k, ld["A"], ld["C"], blas.ArgPack_syrk(order, uplo, tr[c.form[1]], alpha, beta))
    else:
        side = blas.Side.AblasLeft if c.form[0] == "L" else blas.Side.AblasRight
        blas.engine._trmm(ptr["T"], ptr["B"], c.m, c.n, ld["T"], ld["B"], blas.ArgPack_trmm(order, side, blas.UpLo.AblasUpper, tr[c.form[1]], blas.Diag.AblasNonUnit, alpha))


def _run_exact(c, seed):
    blas = _blas()
    ops = T.operands(c, seed)
    ld = T.lds(c)
    offs = dict(zip(("T", "B") if c.op == "trmm" else ("A", "B"), c.offs))
    out_name = "B" if c.op == "trmm" else "C"
    for alpha, beta in c.ab:
        host = {name: T.place(T.initial_output(c, ops, beta) if name == out_name else mat, ld[name], offs.get(name, 0)) for name, mat in ops.items()}
        dev = {name: torch.from_numpy(flat).to(DEV) for name, flat in host.items()}
        _call(blas, c, alpha, beta, {name: buf[offs.get(name, 0):] for name, buf in dev.items()}, ld)
        want = dict(host)
        want[out_name] = T.place(T.exact_reference(c, ops, alpha, beta), ld[out_name], offs.get(out_name, 0))
        for name in host:
            got = dev[name].cpu().numpy()
            assert T.same_bits(got, want[name]), "%s alpha=%s beta=%s, %s: %s" % (c.id, alpha, beta, name, T.describe_mismatch(got, want[name], ld[name], offs.get(name, 0)))


_SEED = {c.id: i for i, c in enumerate(T.CASES)}


@pytest.mark.parametrize("case", T.GEMM_CASES, ids=lambda c: c.id)
def test_gemm_exact(case):
    _run_exact(case, _SEED[case.id])


@pytest.mark.parametrize("case", T.SYRK_CASES, ids=lambda c: c.id)
def test_syrk_exact(case):
    _run_exact(case, _SEED[case.id])


@pytest.mark.parametrize("case", T.TRMM_CASES, ids=lambda c: c.id)
def test_trmm_exact(case):
    _run_exact(case, _SEED[case.id])


@pytest.mark.parametrize("case", T.BIG_CASES, ids=lambda c: c.id)
def test_large_pitch_exact(case):
    """a leading dimension at the limit of the buffer-addressed LDS-DMA (the last legal 32-bit offset) and just beyond it (64-bit addresses):
    the operand spans 4.3 GB of address space, of which only the k leading rows of its 128 columns are written and read"""
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip("less than 12 GiB of device memory free (%.1f GiB): the large-pitch operand needs 4.3 GB of address space" % (free / 2 ** 30))
    blas = _blas()
    c = case
    rng = np.random.default_rng(1000 + T.BIG_CASES.index(c))
    ops = {"A": T.ints(rng, (c.k, c.m)), "C": T.ints(rng, (c.m, c.n))}
    if c.op == "gemm":
        ops["B"] = T.ints(rng, (c.k, c.n))
    ld = {"A": c.k, "B": c.k, "C": c.m}
    ld[c.which] = c.ld
    dev = {}
    for name in ("A", "B") if c.op == "gemm" else ("A",):
        cols = ops[name].shape[1]
        dev[name] = torch.empty(cols * ld[name], dtype=torch.float64, device=DEV)
        dev[name].view(cols, ld[name])[:, :c.k] = torch.from_numpy(np.ascontiguousarray(ops[name].T)).to(DEV)
    for alpha, beta in c.ab:
        c0 = T.initial_output(c, ops, beta)
        dev["C"] = torch.from_numpy(T.place(c0, ld["C"])).to(DEV)
        _call(blas, c, alpha, beta, dev, ld)
        got = dev["C"].cpu().numpy()
        want = T.place(T.exact_reference(c, ops, alpha, beta), ld["C"])
        assert T.same_bits(got, want), "%s alpha=%s beta=%s: %s" % (c.id, alpha, beta, T.describe_mismatch(got, want, ld["C"]))
    for name in dev:
        if name != "C":
            cols = ops[name].shape[1]
            assert T.same_bits(dev[name].view(cols, ld[name])[:, :c.k].cpu().numpy(), np.ascontiguousarray(ops[name].T)), name
    del dev
    torch.cuda.empty_cache()
