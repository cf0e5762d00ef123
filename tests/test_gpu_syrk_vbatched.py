"""-m gpu: cap_dsyrk_vbatched (csrc/syrk_batched.hip) on an MI355X.
1. exact results on mixed size lists (0, 1, 64, 65, 256 among them, in two batch orders, every layout kind of tests/vbatched_cases.py: per-block
leading dimensions and offsets, gaps, reverse order), both layouts of V, fill 0 / 1, with and without beta and shift; everything outside the
blocks keeps its bits, the words of empty blocks included, 2. CONTRACT 1 (PLAN = FIXED) on random real data: every block against the
fixed-size entry on it alone with batch = 1, 3. VarBatch.syrk followed by VarBatch.potrf, 4. the fixed-size entry in stream order."""
import numpy as np
import pytest
import torch

from tests import stream_order as SO
from tests import syrk_batched_cases as SC
from tests import syrk_batched_gpu as G
from tests import trsm_batched_gpu as TG
from tests import vbatched_cases as VC

pytestmark = pytest.mark.gpu

TRANS, NOTRANS = G.TRANS, G.NOTRANS
MIXED = (0, 1, 64, 65, 256, 7, 8, 9, 16, 17, 33, 0, 130, 192, 193, 5, 6, 7, 8, 3, 2, 1, 8, 8, 8, 12)
PERMUTED = tuple(MIXED[i] for i in np.random.default_rng(7).permutation(len(MIXED)))
LISTS = {"MIXED": MIXED, "PERMUTED": PERMUTED, "WAVES": VC.WAVES, "LONE256": (256,), "LONE1": (1,)}
CASES = (("MIXED", "packed", NOTRANS, 0, (1.0, 0.0), 0, 5), ("MIXED", "gaps", TRANS, 1, (-1.0, 1.0), 1, 17),
         ("PERMUTED", "ld+3", TRANS, 0, (2.0, -1.0), 1, 4), ("PERMUTED", "reverse", NOTRANS, 1, (1.0, 0.0), 1, 3),
         ("WAVES", "gaps", NOTRANS, 0, (0.5, 0.5), 0, 16), ("WAVES", "ld+3", TRANS, 1, (1.0, 0.0), 0, 1),
         ("LONE256", "ld+3", NOTRANS, 1, (0.0, 1.0), 1, 40), ("LONE1", "gaps", TRANS, 0, (1.0, 0.0), 1, 0),
         ("MIXED", "reverse", TRANS, 0, (1.0, 0.0), 0, 0))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%s-fill%d-a%g-b%g-shift%d-k%d" % (c[0], c[1], "T" if c[2] else "N", c[3], c[4][0], c[4][1], c[5], c[6]))
def test_exact_results_on_mixed_plans(case):
    name, kind, trans, fill, (alpha, beta), shift, k = case
    sizes = LISTS[name]
    p = G.Plan(sizes, kind)
    try:
        ops = [SC.operands(n, k, i) if n else None for i, n in enumerate(sizes)]
        out = p.run(trans, [None if o is None else o[0] for o in ops], None if beta == 0.0 else [None if o is None else o[1] for o in ops], k, alpha,
                    beta, [0.0 if o is None else o[2] for o in ops] if shift else None, fill)
        for i, o in enumerate(ops):
            if o is None:
                assert out[i] is None
                continue
            E = SC.expected(o[0], o[1], o[2], alpha, beta, shift)
            assert G.same(np.triu(out[i]), np.triu(E)), "block %d (n = %d)" % (i, sizes[i])
            if fill:
                assert G.same(out[i], E), "block %d (n = %d): mirror" % (i, sizes[i])
    finally:
        p.close()


@pytest.mark.parametrize("trans", (NOTRANS, TRANS))
@pytest.mark.parametrize("name,kind", (("MIXED", "gaps"), ("PERMUTED", "ld+3")))
def test_every_block_gets_the_bits_of_the_fixed_size_entry(name, kind, trans):
    sizes, k, alpha, beta = LISTS[name], 19, 1.375, -0.625
    p = G.Plan(sizes, kind)
    try:
        bl = [G.real(n, k, i) if n else None for i, n in enumerate(sizes)]
        out = p.run(trans, [None if b is None else b[0] for b in bl], [None if b is None else b[1] for b in bl], k, alpha, beta,
                    [0.0 if b is None else b[2] for b in bl], 1)
        for i, b in enumerate(bl):
            if b is None:
                continue
            alone = G.run(NOTRANS, [b[0]], [b[1]], alpha, beta, [b[2]], 1)[0]
            assert G.same(out[i], alone), "block %d (n = %d)" % (i, sizes[i])
    finally:
        p.close()


def test_varbatch_syrk_then_potrf():
    from capital_amd import batched
    sizes, k = (5, 0, 70, 1, 64, 130), 33
    vb = batched.VarBatch(sizes, ld=[n + 1 for n in sizes])
    rng = np.random.default_rng(91)
    X = torch.from_numpy(rng.standard_normal((k, vb.rows))).to(G.DEV)
    lam = torch.from_numpy(1.0 + rng.random(len(sizes))).to(G.DEV)
    A = vb.syrk(X, shift=lam)
    assert A.shape == (vb.total,)
    A2 = vb.syrk(X.t().contiguous(), trans=True, shift=lam)
    assert torch.equal(A, A2)
    formed = [vb.block(A, i).clone() for i in range(len(sizes))]
    info = vb.potrf(A)
    assert not info.cpu().numpy().any()
    Xh = X.cpu().numpy()
    for i, n in enumerate(sizes):
        if not n:
            continue
        Xi = Xh[:, vb.row_offsets[i]:vb.row_offsets[i] + n].astype(np.longdouble)
        want = Xi.T @ Xi + np.longdouble(float(lam[i])) * np.eye(n)
        got = np.tril(formed[i].cpu().numpy())
        bound = G.gamma(k + 2) * (np.abs(Xi).T @ np.abs(Xi) + float(lam[i]) * np.eye(n))
        assert np.all(np.abs(got - np.tril(want)) <= bound), i
        assert np.array_equal(np.triu(formed[i].cpu().numpy(), 1), np.zeros((n, n))), "the other triangle of a fresh C was written"
        l = np.tril(vb.block(A, i).cpu().numpy()).astype(np.longdouble)
        assert np.all(np.abs(want - l @ l.T) <= G.gamma(n + 2) * (np.abs(l) @ np.abs(l).T) + bound), i


# ---- stream order -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    e = SO.Env(nstreams=1)
    yield e
    e.close()


@pytest.mark.parametrize("n", (33, 130))
def test_fixed_size_entry_in_stream_order(env, n):
    L = G.lib()
    batch, k = 5, 17
    ldc, sc, ldv, sv = G.shapes(n, k, TRANS, (1, 3), (1, 3))
    bl = [G.real(n, k, 20 + i) for i in range(batch)]
    Cf = TG.Flat([G.lower_nan(b[1]) for b in bl], ldc, sc, True)
    Vf = TG.Flat([b[0].T for b in bl], ldv, sv, False)
    bufs = {"V": Vf.host0, "C": Cf.host0, "shift": np.array([b[2] for b in bl])}

    def enqueue(p, s):
        return L.cap_dsyrk_batched(1, TRANS, n, k, -1.0, p["V"], ldv, sv, 1.0, p["C"], ldc, sc, p["shift"], 0, batch, s)
    job = SO.Job(bufs, enqueue, label="syrk_batched")
    want, ret = env.plain(job)
    assert ret == 0 and np.isfinite(want["C"][Cf.touched]).all() and np.isnan(want["C"][~Cf.touched]).all()
    with env.ordered(job, label="cap_dsyrk_batched n %d k 17" % n) as j:
        assert j.ret == 0
        for name in bufs:
            assert SO.same_bits(j.snap[name], want[name]), name
        assert SO.same_bits(j.snap["V"], Vf.host0) and not SO.same_bits(j.snap["C"], Cf.host0)
