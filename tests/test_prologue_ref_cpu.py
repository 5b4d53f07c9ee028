"""The derived references of tests/prologue_ref.py, checked on the CPU: each must accept the oracle and a model of the kernel's own order, and
must REJECT what it is there to catch (a truncated constant, an element moved by one fp16 step) — a window that accepts everything pins
nothing. The caps are the issue's; the figures in the comments are what this file measured."""
import numpy as np
import pytest

from oracle import fq_oracle as O
from tests import edge_tokens as E
from tests import prologue_ref as R
from tests.conftest import hadk_matrix

F16, F32 = np.float16, np.float32


# ---------------------------------------------------------------------------------------------------------------- A. SiLU.mul

def test_silu_sets_hold_at_most_two_values_and_rarely_two():
    g = R.all_gates()
    fin = np.isfinite(g.astype(F32))
    assert fin.sum() == 63488
    cnt = R.n_admissible(*R.silu_admissible(g))[fin]
    assert cnt.min() == 1 and (cnt >= 3).sum() == 0
    assert (cnt == 2).sum() <= 317, (cnt == 2).sum()                                     # 0.5 % of the finite gates


def test_silu_oracle_and_emulated_kernel_are_admissible_for_every_gate():
    g = R.all_gates()
    lo, hi = R.silu_admissible(g)
    for name, got in (("oracle", O.silu_mul(g, np.ones_like(g))), ("emulation", R.silu8_emulated(g))):
        bad = ~R.in_set(got, [lo, hi])
        assert bad.sum() == 0, (name, int(bad.sum()), g[bad][:8])
    # the classes the issue states
    inf, ninf, nan = F16(np.inf), F16(-np.inf), F16(np.nan)
    lo3, hi3 = R.silu_admissible(np.array([inf, ninf, nan, 0.0, -0.0], F16))
    assert lo3[0] == inf and np.isnan(lo3[1]) and np.isnan(lo3[2])
    assert lo3.view(np.uint16)[3] == 0 and hi3.view(np.uint16)[3] == 0 and lo3.view(np.uint16)[4] == 0x8000 and hi3.view(np.uint16)[4] == 0x8000


def test_silu_sets_reject_a_truncated_constant():
    """fq_silu8 with 1.4427 for log2(e): today's 0.5 % bar passes it, the admissible sets do not"""
    g = R.all_gates()
    g = g[np.isfinite(g.astype(F32))]
    out = ~R.in_set(R.silu8_emulated(g, c=F32(1.4427)), list(R.silu_admissible(g)))
    assert out.sum() >= 50, int(out.sum())


def test_sweep_tokens_hold_every_gate_twice():
    want = np.sort(R.sweep_gates().view(np.uint16))
    for width in (512, 6144, 11008, 14336):
        gate, up = R.sweep_tokens(width)
        half = gate.shape[0] // 2
        for part in (gate[:half], gate[half:]):
            assert np.array_equal(np.unique(part.view(np.uint16)), want)
        assert set(np.unique(np.abs(up.astype(F32)))) == {0.25, 0.5, 1.0, 2.0}
    for M, N in ((112, 128), (128, 224), (86, 128)):
        R.edge_up(E.batch(M, N))                                                         # (asserts that 4 |product| stays finite)


# ---------------------------------------------------------------------------------------------------------------- B. RMSNorm

RMS_DIMS = [(32, 64), (64, 64), (64, 128)]                                               # d = 2048, 4096, 8192


@pytest.mark.parametrize("M,N", RMS_DIMS)
def test_rmsnorm_search_accepts_the_oracle_and_the_kernels_order(M, N):
    b = E.batch(M, N)
    d = M * N
    for eps in (1e-5, 0.0):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            outs = {"oracle": O.rmsnorm(b, eps), "wave model": R.rmsnorm_wave_model(b, eps)}
        for name, y in outs.items():
            for i in range(b.shape[0]):
                r, cands, ok = R.rms_search(b[i], y[i], eps, d)
                assert ok.any(), (name, eps, i)
                if np.isfinite(r):
                    assert 20 <= len(cands) <= 200                              # (the doubled window: 4 w fp32 values at most)
                else:
                    assert eps == 0 and not b[i].any() and np.isnan(y[i]).all()      # the all-zero row at eps = 0: NaN by class


@pytest.mark.parametrize("M,N", RMS_DIMS)
def test_rmsnorm_search_has_power(M, N):
    """every Gaussian row rejects part of its window, and a single element moved by one fp16 step is found at >= 95 % of seeded positions"""
    b = E.batch(M, N)
    d = M * N
    y = O.rmsnorm(b, 1e-5)
    rng = np.random.default_rng([M, N, 77])
    tried = found = whole = 0
    for i in range(0, E.N_BATCH, 2):                                                     # the Gaussian rows
        r, cands, ok = R.rms_search(b[i], y[i], 1e-5, d)
        assert ok.any(), i
        whole += bool(ok.all())
        for p in rng.choice(d, 8, replace=False):
            moved = y[i].copy()
            moved.view(np.int16)[p] += 1 if rng.integers(2) else -1                       # (one step up or down in magnitude)
            tried += 1
            found += not R.rms_search(b[i], moved, 1e-5, d)[2].any()
    # d = 2048: the doubled window holds 26 fp32 values only and ONE of the thirteen Gaussian rows may accept all of them (row 20 does: there the
    # window itself bounds r'); from 4096 on every row must reject part of its window.
    assert whole <= (1 if d < 4096 else 0), whole
    assert found >= 0.95 * tried, (found, tried)


# ---------------------------------------------------------------------------------------------------------------- C. Hadamard

HAD_SHAPES = [(6144, 12), (14336, 28), (12288, 12), (28672, 28), (5120, 40), (8960, 140), (11008, 172), (1536, 12), (5120, 20),
              (64, 1), (512, 1), (8192, 1), (32768, 1)]


@pytest.mark.parametrize("n,K", HAD_SHAPES)
def test_hadamard_tokens_are_exact_and_the_oracle_returns_their_bits(n, K):
    x, single = R.had_tokens(n, K)
    assert 35 <= x.shape[0] <= 70
    xa = np.abs(x.astype(np.float64))
    assert (xa[~single].sum(axis=1) <= R.SUM_CAP).all() and np.array_equal(xa[~single], np.rint(xa[~single]))
    assert ((xa[single] != 0).sum(axis=1) == 1).all() and not x[len(single) - single.sum() - 1].any()
    hadK = hadk_matrix(K) if K > 1 else None
    for scale in R.HAD_SCALES:
        keep = R.had_keep(x, single, scale)
        assert keep[~single].all() and keep.sum() >= 30
        y = R.had_exact(x[keep], K, hadK, scale)                                         # (asserts representability itself)
        nz = np.abs(y[y != 0].astype(F32))
        assert nz.min() >= 2.0 ** -14 and nz.max() <= 65504
        assert np.array_equal(O.hadamard(x[keep], K, hadK, scale).view(np.uint16), y.view(np.uint16))
    s32 = F32(1.0) / np.sqrt(F32(n))
    keep = R.had_keep(x, single, float(s32)) & single
    assert keep.sum() >= 15
    y = R.had_single_default(x[keep], K, hadK, s32)
    assert np.array_equal(O.hadamard(x[keep], K, hadK).view(np.uint16), y.view(np.uint16))
