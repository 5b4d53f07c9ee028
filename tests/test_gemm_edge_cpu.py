"""The reference side of tests/test_gpu_gemm_edge.py checked on its own (builders: tests/gemm_edge.py): the operands multiply to the prescribed
accumulators, and at every K the GPU file runs the ORACLE ALONE reaches each branch of sym_dequant the file is there for — the clamp on both
sides, the bound without the clamp, integers fp16 cannot hold with round-to-even ties in every binade, -9 .. -1 -> +0.0, and -0.0 / subnormal /
Inf / NaN outputs under the format-end scales (NaN capped, so no GPU failure can hide in the NaN class). These are conditions on the INPUTS: if
one fails the inputs change, never the check."""
import numpy as np
import pytest

from oracle import fq_oracle as O
from tests import gemm_edge as G

KS = (128, 10112, 10176, 10208, 10240, 11744, 11776)      # every K of the GPU file's edge cases (the fused decode launch: test below)


@pytest.fixture(scope="module")
def built():
    return {K: G.operands(K) for K in KS}


def count(c):
    return {k: int(v.sum()) for k, v in c.items() if v.dtype == bool}


@pytest.mark.parametrize("K", KS)
def test_the_operands_multiply_to_the_prescribed_accumulators(built, K):
    xq, wq, q = built[K]
    lv = G.levels(K)
    assert xq.shape == (len(lv) + 2, K) and wq.shape == (G.N_FEATURES, K) and q.shape == (len(lv) + 2, G.N_FEATURES)
    assert xq.min() == -8 and xq.max() == 7 and wq.min() == -8 and wq.max() == 7
    assert np.array_equal(O.int4_matmul(O.pack_i4(xq), O.pack_i4(wq)), q.astype(np.int32))
    c, r = G.feature_terms()
    assert np.array_equal(r, np.arange(-128, 112)) and set(c[0::2]) == {64} and set(c[1::2]) == {-56}
    assert np.array_equal(q[:len(lv)], c[None, :] * lv[:, None] + r[None, :])
    assert lv[0] == 0 and lv[-1] == K - G.T and lv[-2] == K - G.T - 1 and np.all(np.diff(lv) > 0)
    # the full-scale rows, on both operands
    assert (xq[-2] == -8).all() and (xq[-1] == 7).all() and (wq[0] == -8).all()
    assert q[-2, 0] == 64 * K and q[-1, 0] == -56 * K
    fw = G.full_scale_w(4, K)
    assert (fw[0] == -8).all() and (fw[1] == 7).all() and (fw[2] == -8).all() and fw.shape == (4, K)
    # fewer features, and rows repeated up to a row count: the same accumulators
    x2, w2, q2 = G.operands(K, n=232)
    assert np.array_equal(w2, wq[:232]) and np.array_equal(q2, q[:, :232])
    xr, qr = G.repeat_rows(xq, q, 65)
    assert xr.shape[0] == 65 and np.array_equal(xr[len(xq):2 * len(xq)], xq[:65 - len(xq)]) and np.array_equal(qr[len(xq)], q[0])


@pytest.mark.parametrize("K", KS)
def test_every_branch_of_the_integer_part_is_reached(built, K):
    xq, wq, q = built[K]
    lv = len(G.levels(K))
    c, n = G.classify(q), count(G.classify(q))
    assert n["minus9_to_minus1"] == 23                      # (row 0: q = r, and -56 + r, 64 + r of row 1; trunc(-0.x) = -0.0 where the reference's int is +0)
    assert np.array_equal(c["iv"], np.trunc(q.astype(np.float32) / np.float32(10)).astype(np.int64))      # the classifier's iv IS the oracle's
    if K == 128:                                            # a one-stage K loop: the signs and zeros only (|q| / 10 < 2048)
        assert np.abs(c["iv"]).max() < 2048 and n["inexact"] == 0
        return
    # integers fp16 cannot hold, with round-to-even ties in every binade from 2048 up
    assert n["inexact"] >= 2000
    for e in range(11, 16):
        t = c["tie"] & (c["binade"] == e)
        assert t.sum() >= 10, e
        iv = np.abs(np.clip(c["iv"][t], -G.CLAMP, G.CLAMP))
        lo = (iv - (1 << (e - 11))) >> (e - 10)             # the two neighbours, in units of the binade's spacing: both parities are met,
        assert set((lo % 2).tolist()) == {0, 1}, e          # i.e. ties that round DOWN to even and ties that round UP to even
    # multiples of ten where q * 0.1f is inexact in fp32, on both signs (the all-7 token row carries the negative ones)
    big10 = (q % 10 == 0) & (np.abs(q) > (1 << 16))
    assert (big10 & (q > 0)).sum() >= 20 and (big10 & (q < 0)).sum() >= 20
    m = count(G.classify(q[:lv]))                          # the level rows alone: the figures the helper was designed to
    if K > 11640 + G.T:
        assert (m["clamped_high"], m["clamped_low"], m["on_bound"], m["inexact"], m["inf_without_clamp"]) == (777, 453, 30, 3632, 840)
        assert n["clamped_high"] > m["clamped_high"] and n["clamped_low"] > m["clamped_low"]          # the full-scale rows clamp as well
        on = c["iv"][c["on_bound"]]
        assert (on == G.CLAMP).sum() >= 10 and (on == -G.CLAMP).sum() >= 10
    elif K > 10176:
        assert m["clamped_high"] == 417 and n["clamped_low"] == 0 and m["on_bound"] >= 10
        assert (c["iv"][c["on_bound"]] == G.CLAMP).all()
        assert (n["inf_without_clamp"] > 0) == (64 * K // 10 >= 65520)        # K = 10240: 65536 is Inf in fp16 without the clamp
    else:                                                   # the kernels' gate: the clamp cannot bind — and the top level sits just under it
        assert n["clamped_high"] == n["clamped_low"] == n["on_bound"] == n["inf_without_clamp"] == 0
        assert c["iv"].max() == 64 * K // 10 and G.CLAMP - c["iv"].max() <= 64 * (10176 - 10112) // 10 + 51


@pytest.mark.parametrize("K", KS)
def test_the_scale_cases_reach_the_ends_of_fp16_and_nan_stays_rare(built, K):
    xq, wq, q = built[K]
    xp, wp = O.pack_i4(xq), O.pack_i4(wq)
    M, N = q.shape
    b = G.bias(N)
    assert np.isinf(b).sum() == 1 and (b == 65504).sum() == 1 and (b == -65504).sum() == 1
    with np.errstate(invalid="ignore"):
        sx, sw = G.scales("ordinary", M, N)
        assert np.isfinite(sx).all() and np.isfinite(sw).all() and sx.min() > 0 and sw.min() > 0
        for bb in (None, b):
            assert not np.isnan(O.linear4bit(xp, sx, wp, sw, bb)).any()          # NaN occurs in no ordinary case
        sx, sw = G.scales("ends", M, N)
        for ends, s in ((G.X_ENDS, sx), (G.W_ENDS, sw)):
            for v in ends:
                assert (np.isnan(s).sum() == 1) if np.isnan(v) else ((s == np.float16(v)).sum() == 1), v
        y = O.linear4bit(xp, sx, wp, sw)
        sub = (y != 0) & (np.abs(y.astype(np.float32)) < 2.0 ** -14)
        assert ((y == 0) & np.signbit(y)).sum() >= 10 and ((y == 0) & ~np.signbit(y)).sum() >= 10
        assert sub.sum() >= 2 and (y == np.inf).sum() >= 10 and (y == -np.inf).sum() >= 10
        yb = O.linear4bit(xp, sx, wp, sw, b)
        assert 0 < np.isnan(y).mean() <= 0.01 and 0 < np.isnan(yb).mean() <= 0.01
        assert (np.isnan(yb) & ~np.isnan(y)).any()           # Inf + (-Inf) in the bias add


def test_the_rows_of_the_fused_decode_case():
    """K = 4096 against digits +-7 (tests/test_gpu_gemm_edge.py builds them through the kernel's own quantiser): |q| / 10 reaches the
    twenty-thousands, fp16-inexact with ties, and -9 .. -1 occurs"""
    K = 4096
    _, wq, _ = G.operands(K, full_scale=False)
    A = G.decode_levels(K)
    assert len(A) == 16
    xq = np.where(np.arange(K)[None, :] < A[:, None], -7, 7).astype(np.int32)
    q = xq.astype(np.int64) @ wq.astype(np.int64).T
    n, c = count(G.classify(q)), G.classify(q)
    assert 20000 <= np.abs(c["iv"]).max() < 30000 and n["inexact"] >= 500 and n["minus9_to_minus1"] >= 1
    assert {11, 12, 13, 14} <= set(c["binade"][c["tie"]].tolist())


def test_sym_dequant_values():
    v = G.dequant_values()
    assert v.dtype == np.int32 and len(set(v.tolist())) == len(v)
    for a in (0, 9, 10, 11, 20479, 20491, 651759, 651760, 651769, 651770, (1 << 24) - 1, 1 << 24, (1 << 24) + 1):
        assert a in v and -a in v
    assert np.iinfo(np.int32).max in v and np.iinfo(np.int32).min in v
    g = G.dequant_grid()
    assert g.shape == (16, 4 * len(v)) and all((g[i] == a).any() for i in range(16) for a in (v[0], v[-1]))
    iv = np.trunc(g.astype(np.float32) / np.float32(10))
    assert (iv > G.CLAMP).any() and (iv < -G.CLAMP).any() and (iv == G.CLAMP).any() and (iv == -G.CLAMP).any()
    with np.errstate(invalid="ignore"):
        assert not np.isnan(O.sym_dequant(g, *G.scales("ordinary", *g.shape))).any()
        y = O.sym_dequant(g, *G.scales("ends", *g.shape))
        assert 0 < np.isnan(y).mean() <= 0.01 and np.isinf(y).any() and ((y == 0) & np.signbit(y)).any()


def test_constant_rows_by_slices():
    assert G.const_product(-8, -8, 14336) == 64 * 14336 and G.const_product(-8, 7, 1 << 18) == -56 << 18
    K = 70000 - 70000 % 32
    direct = O.int4_matmul(O.pack_i4(np.full((1, K), -8, dtype=np.int32)), O.pack_i4(np.full((1, K), 7, dtype=np.int32)))
    assert G.const_product(-8, 7, K) == int(direct[0, 0])
    assert G.const_product(-8, -8, 131072) == 1 << 23 and 256 * G.const_product(-8, -8, 131072) == 1 << 31      # what the int8 path would carry
    assert G.const_product(-8, -8, G.GENERAL_K_CAP) < 1 << 31 <= 64 * (G.GENERAL_K_CAP + 32)
    assert G.const_product(-8, -8, 1 << 18) == 1 << 24
