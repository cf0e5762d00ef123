"""The rounding model of the mixed-precision factor (tests/mixed_model.py) checked on its own, without a GPU: it is plain blocked
Cholesky when its roundings are off, its bf16 conversion is torch's bit for bit, its factor sits in the bf16 error band, and a
single planted defect moves its factor far outside the tolerances the GPU tests (tests/test_gpu_mixed.py) hold the library to."""
import numpy as np
import pytest
import torch

from tests import mixed_model as mm


def _spd(n, kind, seed=0):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((n, n))
    return b @ b.T / n + (0.5 if kind == "gram" else 0.02) * np.eye(n)      # kappa ~ 10 / ~ 200


def _rel(x, ref):
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("n", [128, 640, 896, 2048, 2176])
def test_without_rounding_the_model_is_fp64_cholesky(n):
    """panel widths 128 ... 1024, one panel, a ragged last panel (896 = 512 + 384, 2176 = 2 x 1024 + 128)"""
    a = _spd(n, "spd", seed=n)
    r = mm.factor(a, rounding=False)
    assert _rel(r, np.linalg.cholesky(a).T) < 1e-12
    assert mm.panel_width(n) == {128: 128, 640: 512, 896: 512, 2048: 1024, 2176: 1024}[n]


def test_bf16_conversion_is_torchs_bit_for_bit():
    """round to nearest even incl. ties both ways, subnormals, the largest finite values (one of them rounds to inf), +-inf, NaN;
    and the truncating converter of the teeth below really truncates"""
    rng = np.random.default_rng(0)
    bits = [0x3F808000, 0x3F818000, 0x3F80FFFF, 0x3F817FFF, 0xBF808000, 0xBF818000,       # ties to even (down, up), just off them
            0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807F8000, 0x00800000,       # subnormals, the smallest normal
            0x7F7FFFFF, 0x7F7F7FFF, 0xFF7F8000, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,
            0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FBFFFFF]                                # NaNs (quiet, signalling, negative)
    u = np.concatenate([np.array(bits, dtype=np.uint32), rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32),
                        (rng.integers(0, 2 ** 16, 20000, dtype=np.uint64).astype(np.uint32) << 16) | 0x8000])     # random ties
    x = u.view(np.float32)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = mm.bf16_bits(x)
    nan = np.isnan(x)
    assert nan.sum() >= 4
    assert np.array_equal(got[~nan], want[~nan]), np.flatnonzero(got[~nan] != want[~nan])[:10]
    # NaN stays NaN (which NaN pattern is the converter's choice: torch's vectorised CPU path answers 0xffff, the model 0x7fc0)
    as_f32 = lambda h: (h.astype(np.uint32) << 16).view(np.float32)
    assert np.isnan(as_f32(got[nan])).all() and np.isnan(as_f32(want[nan])).all()
    assert np.array_equal(mm.bf16_bits(np.float32([1.0 + 2 ** -8 + 2 ** -9]), trunc=True), np.uint16([0x3F80]))


@pytest.mark.parametrize("kind,lo,hi", [("gram", 5e-5, 2e-3), ("spd", 2e-4, 1e-2)])
def test_the_model_factor_is_in_the_bf16_band(kind, lo, hi):
    """bf16 panels (relative 2^-9) in every update: the factor is ~ 1e-4 .. 1e-3 off the fp64 one, more with kappa; and not closer than
    the fp32 storage would be on its own (the roundings are really on)"""
    a = _spd(2048, kind, seed=1)
    ref = np.linalg.cholesky(a).T
    e = _rel(mm.factor(a), ref)
    assert lo < e < hi, e
    assert _rel(mm.factor(a, solve3=False), ref) < hi


@pytest.fixture(scope="module")
def teeth_case():
    a = _spd(3072, "gram", seed=3)                            # three panels: two updates, a tile to skip, a previous panel
    return a, mm.factor(a)


@pytest.mark.parametrize("perturb", [("trunc",), ("no_lohi",), ("skip_tile", 0, 5, 9), ("skip_tile", 1, 8, 8), ("stale_panel", 1)])
def test_one_planted_defect_is_ten_times_outside_the_gpu_tolerance(teeth_case, perturb):
    """The GPU test compares a factor with the model replayed on that factor's own bf16 panels (mixed_model.factor(panels_of=)).
    A factor with ONE defect - truncating bf16 conversions, the row solve without its lo * hi term, one 256 x 256 tile of one update
    not applied, one update with the previous panel's operand - fails that comparison by at least 10 x the normwise or the per-tile
    bound; the unperturbed model passes it exactly."""
    a, r = teeth_case
    tn, tt = mm.tolerances(a.shape[0])
    assert _rel(mm.factor(a, panels_of=r), r) == 0.0
    bad = mm.factor(a, perturb=perturb)
    replay = mm.factor(a, panels_of=bad)
    norm, tile = _rel(bad, replay), float(mm.tile_errors(bad, replay).max())
    assert norm > 10 * tn or tile > 10 * tt, (perturb, norm, tile, tn, tt)
    if perturb[0] == "skip_tile":
        assert tile > 10 * tt, (norm, tile)
    else:
        assert norm > 10 * tn, (norm, tile)
    # against the unperturbed model, too
    assert _rel(bad, r) > 10 * tn
