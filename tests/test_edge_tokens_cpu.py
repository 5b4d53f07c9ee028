"""The reference side of tests/test_gpu_edge_tokens.py checked on its own: with the signed-permutation factors of tests/edge_tokens.py
the oracle's transform of the edge batch is EXACT (equal to the fp64 product, finite, representable in the activation dtype) for every pair
the GPU file runs, the tie / zero rows quantise as the reference's round-half-even says, and every clip pair of SIGS reaches the quantiser
routes it is listed for. These are conditions on the INPUTS: if one fails for a pair the inputs change, never the check."""
import numpy as np
import pytest

from oracle import fq_oracle as O
from tests import edge_tokens as E


@pytest.mark.parametrize("lowp", ["f16", "bf16"])
@pytest.mark.parametrize("M,N", E.ALL_PAIRS)
def test_exact_factors_make_the_oracle_transform_exact(M, N, lowp):
    b = E.batch(M, N, lowp)
    L, R = E.exact_factors(M, N, lowp)
    assert b.shape == (E.N_BATCH, M * N) and b.dtype == (np.float32 if lowp == "bf16" else np.float16)
    for m in (L, R):                                                   # permutations with entries in {-1, -2} (why both negative: exact_factors)
        assert np.array_equal((m != 0).sum(axis=0), np.ones(len(m))) and np.array_equal((m != 0).sum(axis=1), np.ones(len(m)))
        assert set(np.unique(m[m != 0]).astype(np.float64)) <= {-1.0, -2.0}
    y = O.kron_transform(b, L, R, lowp=lowp)
    X = b.astype(np.float64).reshape(-1, M, N)
    want = L.astype(np.float64).T @ X @ R.astype(np.float64)
    assert np.isfinite(y).all()
    assert np.array_equal(y.astype(np.float64), want)
    assert np.array_equal(O._rnd(y, lowp), y)                          # representable: FQ_ROUND_Y_F16 changes nothing
    assert not y[1].any() and y[0].any()


@pytest.mark.parametrize("lowp", ["f16", "bf16"])
@pytest.mark.parametrize("M,N", [(64, 64), (86, 128), (3, 6)])
@pytest.mark.parametrize("round_y", [False, True])
@pytest.mark.parametrize("clamp0", [False, True])
@pytest.mark.parametrize("quant_f16", [False, True])
def test_tie_and_zero_rows_through_the_reference_quantiser(M, N, lowp, round_y, clamp0, quant_f16):
    e = E.edge_rows(M, N, lowp)
    eye = lambda n: np.eye(n, dtype=e.dtype)
    ref = O.kron_quant(e, eye(M), eye(N), 1.0, 1.0, round_y_f16=round_y, clamp0=clamp0, quant_f16=quant_f16, lowp=lowp)
    assert ref["q"][7, :8].tolist() == [7, 0, 2, 2, 0, -2, 4, -4] and not ref["q"][7, 8:].any()       # .5 ties go to even
    assert ref["scale"][7] == 1.0
    fq = ref["fq"][7, 4]                                                                              # fake-quant of -0.5: +0.0, never -0.0
    bits = O.bf16_bits(fq) if lowp == "bf16" else np.asarray(fq).view(np.uint16)
    assert int(np.asarray(bits).reshape(-1)[0]) == 0x0000
    assert ref["scale"][0] == 1.0 and not ref["q"][0].any()                                           # m == 0 -> scale 1
    assert not np.asarray(ref["fq"][0], np.float32).view(np.uint32).any()
    if quant_f16 and lowp == "f16":   # the one-hot subnormal: m / 7 underflows the fp16 scale; the reference divides by the 0 it stores
        hot = M * N // 2
        assert ref["scale16"][8] == 0 and ref["q"][8, hot] == 7 and np.abs(ref["q"][8]).sum() == 7 and not np.asarray(ref["fq"][8]).any()


@pytest.mark.parametrize("lowp", ["f16", "bf16"])
@pytest.mark.parametrize("M,N", E.ALL_PAIRS)
def test_every_clip_pair_reaches_the_routes_it_is_listed_for(M, N, lowp):
    """(no single pair can reach all three routes on one batch — sig = (1, 1) puts every quotient at +-7 — so the list says which routes
    each entry is there for, and together they must cover the three)"""
    b = E.batch(M, N, lowp)
    y = O.kron_transform(b, *E.exact_factors(M, N, lowp), lowp=lowp).reshape(E.N_BATCH, -1)
    assert len(E.SIGS) == len(E.SIG_ROUTES) == 9
    seen = set()
    for sig, want in zip(E.SIGS, E.SIG_ROUTES):
        for clamp0 in (True, False):
            got = set(E.routes(y, sig, clamp0).tolist())
            assert want <= got, (sig, clamp0, got)
            seen |= got
    assert seen == {"plain", "clamp", "div"}
    # (0.9346, 0.9346) sits ON the clamp guard: its largest quotient lies between 7.48 and fq_needs_clamp's 7.49
    s = O.token_scale(y, 0.9346, 0.9346)
    quot = (np.abs(y).max(axis=1) / s)[np.abs(y).max(axis=1) > 0]
    assert ((quot > 7.48) & (quot < 7.49)).any()
    # (0.33, 0.9) without the clamp to zero: the single-signed rows (batch rows 3, 5 and 19) keep both extremes on one side of zero
    assert y[3].min() > 0 and y[5].max() < 0 and y[19].min() in (7, 14, 28)
    assert E.routes(y, (0.33, 0.9), clamp0=False)[3] == "clamp"
    assert O.token_scale(y[19:20], 3e-6, 1.0, clamp0=False)[0] == y[19].min() / np.float32(7)              # from the MINIMUM of the constant row


@pytest.mark.parametrize("lowp", ["f16", "bf16"])
@pytest.mark.parametrize("M,N", E.ALL_PAIRS)
def test_random_factors_keep_the_batch_finite(M, N, lowp):
    """a condition on the inputs of the GPU file's parts (b) and (c): neither the rounded intermediate nor the result overflows"""
    y = O.kron_transform(E.batch(M, N, lowp), *E.random_factors(M, N, lowp), lowp=lowp)
    assert np.isfinite(O._rnd(y, lowp)).all()


def test_nonfinite_rows():
    b = E.batch(64, 64)
    bad = E.nonfinite(b)
    rest = [i for i in range(E.N_BATCH) if i not in E.NONFINITE_ROWS]
    assert np.array_equal(bad[rest], b[rest]) and np.isfinite(b).all()
    assert np.isnan(bad[1]).all() and np.isinf(bad[3]).sum() == 1 and (bad[9] == 65504).all()
