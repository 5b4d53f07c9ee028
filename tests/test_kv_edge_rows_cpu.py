"""The reference side of tests/test_gpu_kv_edge_rows.py checked on its own (builders: tests/kv_edge_rows.py): the oracle's value BEFORE its clip is
classified per row, every branch of the quantiser (csrc/fq_kv_common.hpp: kv_params, kv_q8) is reached by at least one row, and the digits no
reference defines (that value is NaN: 0 / 0, Inf / Inf) — which the GPU file masks — are capped HERE, so no GPU failure can hide behind the mask.
These are conditions on the INPUTS: if one fails the inputs change, never the check."""
import numpy as np
import pytest

from oracle import fq_oracle as O
from tests import kv_edge_rows as K

HDS = (64, 128)
TINY = {f"tiny_{k}" for k in K.TINY_UNITS}


def edge_name(i):
    """name of batch row i (None: an ordinary row)"""
    return K.EDGE_NAMES[(i - 1) // 2] if i % 2 else None


def inputs(hd, trans):
    b = K.batch(hd)
    return O.kv_transform(b, K.exact_trans(hd)) if trans else b


def by_name(hd, trans, clip, lac):
    r = K.routes(inputs(hd, trans), clip, lac)
    return {edge_name(i): r[i] for i in range(1, K.N_BATCH, 2)}, r


@pytest.mark.parametrize("hd", HDS)
def test_the_builders_build_what_they_say(hd):
    e, b = K.edge_rows(hd), K.batch(hd)
    assert e.shape == (K.N_EDGE, hd) and b.shape == (K.N_BATCH, hd) and e.dtype == b.dtype == np.float16
    assert np.array_equal(b[1::2].view(np.uint16), e.view(np.uint16)) and np.isfinite(b).all()
    u = K.UNIT
    assert not e[K.ROW["zero"]].any() and (e[K.ROW["positive"]] > 0).all() and (e[K.ROW["negative"]] < 0).all()
    assert e[K.ROW["onehot_first"], 0] == 1 and np.count_nonzero(e[K.ROW["onehot_first"]]) == 1
    assert e[K.ROW["onehot_last"], hd - 1] == -3 and np.count_nonzero(e[K.ROW["onehot_last"]]) == 1
    assert e[K.ROW["outlier_15000"]].max() == 15000
    sub = lambda r: (r != 0) & (np.abs(r) < np.float16(2.0 ** -14))
    assert sub(e[K.ROW["gauss_1e-3"]]).any() and (~sub(e[K.ROW["gauss_1e-3"]])).any()
    g6 = e[K.ROW["gauss_1e-6"]].astype(np.float64)
    assert 0 < g6.max() - g6.min() < 1e-5
    lone = e[K.ROW["lone_subnormal"]]
    assert lone[hd // 2].view(np.uint16) == 1 and np.count_nonzero(lone) == 1
    assert (e[K.ROW["const_7"]] == 7).all() and sorted(set(e[K.ROW["const_-8_one_7"]].tolist())) == [-8.0, 7.0]
    ties = e[K.ROW["ties"]].astype(np.float64)
    assert ties.min() == 0 and ties.max() == 15
    for k in range(15):
        for dlt in (0.0, 2.0 ** -6, -2.0 ** -6):
            assert (ties == k + 0.5 + dlt).any()
    places = set()
    for i, k in enumerate(K.TINY_UNITS):
        r = e[K.ROW[f"tiny_{k}"]].astype(np.float64)
        (c,) = np.nonzero(r)[0]
        assert r[c] == k * u and c == K.tiny_col(i, hd)
        places.add((c // 32, (c // 16) % 2, c % 16))
    assert len(places) == 6 and len({(q, h) for q, h, _ in places}) == min(6, hd // 16)
    m172 = e[K.ROW["tiny_-172"]].astype(np.float64)
    assert sorted(set(m172.tolist())) == [-172 * u, 0.0] and np.count_nonzero(m172 == 0) == 1
    assert sorted(set(e[K.ROW["const_1000_one_ulp"]].tolist())) == [1000.0, 1000.5]
    top = e[K.ROW["top_65504"]].astype(np.float64)
    assert top.max() == 65504 and top.min() >= 0 and np.isfinite(np.float16(top.max() - top.min()))
    ov = e[K.ROW["overflow_40000"]].astype(np.float64)
    assert ov.max() == 40000 and ov.min() == -40000


@pytest.mark.parametrize("hd", HDS)
def test_extrema_rows_cover_every_pair_of_places(hd):
    e = K.extrema_rows(hd)
    n = hd // 16
    assert e.shape == (n * n, hd)
    seen = set()
    for r in e.astype(np.float64):
        assert r.max() == 3 and r.min() == -5 and np.abs(np.delete(r, [r.argmax(), r.argmin()])).max() < 0.1
        seen.add((r.argmax() // 16, r.argmin() // 16))
    assert len(seen) == n * n                                  # (quarter, half) of the maximum x (quarter, half) of the minimum
    for lac, clip in ((False, (1.0, 1.0)), (True, (0.9, 0.8))):
        assert not K.unpinned(e, clip, lac).any()


@pytest.mark.parametrize("hd", HDS)
def test_exact_trans_makes_the_oracle_transform_exact(hd):
    T = K.exact_trans(hd)
    assert np.array_equal((T != 0).sum(axis=0), np.ones(hd)) and np.array_equal((T != 0).sum(axis=1), np.ones(hd))
    vals = set(np.unique(T[T != 0]).astype(np.float64))
    assert vals == {-2.0, -1.0, 1.0, 2.0}
    assert not np.array_equal(np.argmax(T != 0, axis=1), np.arange(hd))
    for x in (K.batch(hd), K.extrema_rows(hd)):
        y = O.kv_transform(x, T)
        assert np.array_equal(y.view(np.uint16), K.exact_product(x, T).view(np.uint16))
        with np.errstate(over="ignore"):
            want = (x.astype(np.float64) @ T.astype(np.float64)).astype(np.float16)
        assert np.array_equal(y, want) and np.isfinite(y).all()
        assert not (y.view(np.uint16) == 0x8000).any()        # no -0.0: the kernels' fp32 sums start from +0


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("lac,clip", [(False, (1.0, 1.0))] + [(True, c) for c in K.CLIPS])
def test_preclip_restates_the_oracle(hd, trans, lac, clip):
    """clip(pre, 0, 15) IS the oracle's digit and the parameters are the oracle's, bit for bit: `pre` is the oracle's own value before the clip"""
    for x in (inputs(hd, trans), K.extrema_rows(hd)) + ((K.sweep_rows(hd),) if hd == 128 and not trans and clip in ((1.0, 1.0), (0.9, 0.8)) else ()):
        p = K.preclip(x, clip, lac)
        packed, scale, zero, q = O.kv_asym_quant(x, clip[0], clip[1], lac)
        with np.errstate(invalid="ignore"):
            mine = np.nan_to_num(np.clip(p["pre"], np.float16(0), np.float16(15)).astype(np.float32), nan=0.0).astype(np.uint8)
        assert np.array_equal(mine, q)
        assert np.array_equal(p["scale"].view(np.uint16), scale.view(np.uint16))
        nz = ~np.isnan(zero)
        assert np.array_equal(p["zero"].view(np.uint16)[nz], zero.view(np.uint16)[nz]) and np.array_equal(np.isnan(p["zero"]), ~nz)
        assert np.array_equal(packed, (q[:, 0::2] | (q[:, 1::2] << 4)))


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("trans", [False, True])
def test_every_route_without_lac_is_reached(hd, trans):
    names, allr = by_name(hd, trans, (1.0, 1.0), False)
    for n in ("zero", "gauss_1e-6", "lone_subnormal"):
        assert "floor" in names[n]                             # the 1e-5 floor binds
    for k in K.TINY_UNITS:                                     # the row's maximum has the rounded quotient 15.5 .. 15.63: rint gives 16
        assert "rint16" in names[f"tiny_{k}"] and "subnormal_scale" in names[f"tiny_{k}"]
        x = inputs(hd, trans)[2 * K.ROW[f"tiny_{k}"] + 1]
        p = K.preclip(x[None], (1.0, 1.0), False)
        top = x.argmax() if x.max() > 0 else x.argmin()        # (exact_trans may have negated the value: then it is the minimum, digit 0)
        if x.max() > 0:
            assert 15.5 <= float(p["quot"][0, top]) < 15.64 and p["pre"][0, top] == 16
    if not trans:
        assert "rint16" in names["tiny_-172"]                  # the same range below zero (zero = 172 units)
        assert {"tie_even", "tie_odd"} <= names["ties"]
        q = O.kv_asym_quant(K.edge_rows(hd)[K.ROW["ties"]][None])[3][0]
        assert q[2:17].tolist() == [0, 2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 12, 12, 14, 14]                 # .5 ties go to even
        assert q[17:32].tolist() == list(range(1, 16)) and q[32:47].tolist() == list(range(15))      # their neighbours do not
    assert "inf_scale" in names["overflow_40000"]
    every = set().union(*allr)
    assert {"floor", "rint16", "tie_even", "tie_odd", "inf_scale", "subnormal_scale"} <= every


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("trans", [False, True])
def test_every_route_with_lac_is_reached(hd, trans):
    per_clip = {c: by_name(hd, trans, c, True) for c in K.CLIPS}
    for c in K.CLIPS:
        names, allr = per_clip[c]
        assert "subst" in names["zero"]                        # lac's (-1, 1) substitution
        assert "inf_scale" in names["overflow_40000"] or c == (0.02, 0.5)
        assert {"tie_even", "tie_odd"} <= set().union(*allr)
    for c in K.CLIPS[1:]:
        every = set().union(*per_clip[c][1])
        assert {"clamp_above", "clamp_below"} <= every         # the clamp binds on both sides
    assert "zero_scale" in per_clip[(1.0, 1.0)][0]["lone_subnormal"]
    names, allr = per_clip[(0.02, 0.5)]
    assert "beyond_512" in set().union(*allr)                  # quotients outside the exact range of the magic-number rint
    assert "subst" in names["lone_subnormal"]                  # (0.02 of one unit rounds to 0: the row counts as all-zero)
    assert any("zero_scale" in names[t] for t in TINY)


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("trans", [False, True])
def test_unpinned_digits_are_capped(hd, trans):
    """what the GPU file may mask. lac off: at most 2 digits, both in the +-40000 row (whose range is Inf) — through exact_trans one more, in the
    65504 row (its other values change sign there: that range overflows too). lac: only rows whose scale underflows to 0 (zero = 0 / 0): the lone
    subnormal, and under the 0.02 clip the tiny-range rows; every digit of such a row is unpinned, no digit of any other row is."""
    x = inputs(hd, trans)
    m = K.unpinned(x, (1.0, 1.0), False)
    rows = {edge_name(i) for i in np.nonzero(m.any(axis=1))[0]}
    assert rows <= ({"overflow_40000", "top_65504"} if trans else {"overflow_40000"})
    assert m[2 * K.ROW["overflow_40000"] + 1].sum() <= 2 and m[2 * K.ROW["top_65504"] + 1].sum() <= 1
    assert m.sum() <= (3 if trans else 2)
    for c in K.CLIPS + [K.APPEND_CLIP[2:]]:
        m = K.unpinned(x, c, True)
        r = K.routes(x, c, True)
        rows = {edge_name(i) for i in np.nonzero(m.any(axis=1))[0]}
        assert rows <= ({"lone_subnormal"} | (TINY if c == (0.02, 0.5) else set()))
        for i in np.nonzero(m.any(axis=1))[0]:
            assert "zero_scale" in r[i]
        _, scale, zero, _ = O.kv_asym_quant(x, c[0], c[1], True)
        assert not np.isnan(scale).any()
        assert np.array_equal(m.any(axis=1), m.all(axis=1))             # such a row is unpinned as a whole (its zero point is NaN, or Inf - Inf)
        assert not (np.isnan(zero[:, 0]) & ~m.all(axis=1)).any()        # the ONLY parameters no comparison sees: NaN zero points, of those rows


def test_sweeps_cover_their_cases_and_have_no_unpinned_digit():
    s = K.sweep_rows(128)
    assert s.shape[1] == 128 and 1000 < s.shape[0] < 10000
    assert not K.unpinned(s, (1.0, 1.0), False).any() and not K.unpinned(s, (0.9, 0.8), True).any()
    fam = {}
    for name, pairs in K.SWEEPS.items():
        fam[name] = [K.preclip(K.sweep(lo, hi), (1.0, 1.0), False) for lo, hi in pairs]
        for (lo, hi), p in zip(pairs, fam[name]):
            sw = K.sweep(lo, hi)
            assert (sw.min(axis=1) == np.float16(lo)).all() and (sw.max(axis=1) == np.float16(hi)).all()
            assert len(np.unique(p["scale"].view(np.uint16))) == 1 and len(np.unique(p["zero"].view(np.uint16))) == 1
            v = K._bits_between(lo, hi)                          # every representable value in between is in some row
            assert np.isin(v.view(np.uint16), sw.view(np.uint16)).all()
    f16 = np.float16
    assert all(p["scale"][0, 0] == 1 for p in fam["scale_1"])
    assert all(np.frexp(float(p["scale"][0, 0]))[0] != 0.5 for p in fam["scale_not_pow2"]) and any(p["zero"][0, 0] > 0 for p in fam["scale_not_pow2"])
    assert all(p["d"][0, 0] > f16(1e-5) for p in fam["scale_subnormal"]) and sum(p["scale"][0, 0] < f16(2.0 ** -14) for p in fam["scale_subnormal"]) == 2
    assert all(p["d"][0, 0] <= f16(1e-5) for p in fam["floor"])
    assert all(p["d"][0, 0] == 65504 for p in fam["largest"])
    assert all(p["d"][0, 0] <= 2.5 and abs(float(p["zero"][0, 0])) >= 1000 for p in fam["offset_1000"])
    wraps = [int(round(float(hi) / K.UNIT)) for (lo, hi), p in zip(K.SWEEPS["tiny"], fam["tiny"]) if lo == 0 and (p["pre"] == 16).any()]
    assert set(K.TINY_UNITS) <= set(wraps)                       # (the ranges the edge rows were taken from)
    r = set().union(*K.routes(s, (0.9, 0.8), True))
    assert {"clamp_above", "clamp_below", "tie_even", "tie_odd"} <= r
