"""The builders of tests/quant_edge_rows.py checked on their own (no GPU): the rows have the scales, quotients and routes they were built for,
the by-hand digits are what the oracle computes, and the batch tells each of a list of WRONG quantisers from the right one. These are
conditions on the INPUTS of tests/test_gpu_quant_edge_rows.py: if one fails the inputs change, never the check."""
import numpy as np
import pytest

from oracle import fq_oracle as O
from tests import edge_tokens as E
from tests import quant_edge_rows as Q

# (the oracle divides by underflowed scales and overflows fp16 on purpose on these rows)
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")
F32 = np.float32
COLS = [64, 136, 264, 2056, 4104]                 # the construction conditions hold from 64 columns on
SMALL = [8, 16, 24]
ALL_BITS = [4, 2, 3, 5, 6, 7, 8]


def _rows_of(kind, specials):
    return [(i, sp) for i, sp in specials.items() if sp.kind == kind]


@pytest.mark.parametrize("lowp", ["f16", "bf16"])
@pytest.mark.parametrize("cols", SMALL + COLS + [63, 4097])
def test_batch_layout(cols, lowp):
    b, labels, specials = Q.batch(cols, lowp)
    assert b.shape[0] % 2 == 1 and b.shape[0] < 60 and b.shape == (len(labels), cols)
    assert b.dtype == (np.float32 if lowp == "bf16" else np.float16) and np.isfinite(b).all()
    assert np.array_equal(O._rnd(b.astype(F32), lowp), b.astype(F32))
    assert all(l == "ordinary" for l in labels[0::2]) and "ordinary" not in labels[1::2]
    x = b.astype(F32)
    row = lambda name: x[labels.index(name)]
    assert not row("all zero").any() and (row("all positive") > 0).all() and (row("all negative") < 0).all()
    assert row("one-hot -3 last")[-1] == -3 and not row("one-hot -3 last")[:-1].any()
    assert row("outlier 15000").max() == (15000 if lowp == "f16" else O.bf16_round(F32(15000)))
    assert (row("constant 7") == 7).all() and row("constant -8, one +7").min() == -8 and row("constant -8, one +7").max() == 7
    top = F32(65504) if lowp == "f16" else O.bf16_round(F32(65504))
    assert row("+-65504").max() == top and row("+-65504").min() == -top
    if lowp == "f16":
        sub = np.abs(row("gaussians x 1e-3"))
        assert ((sub > 0) & (sub < 2.0 ** -14)).any() or cols < 64            # fp16 subnormals among them
        assert np.count_nonzero(row(Q.UNDERFLOW)) == 1 and row(Q.UNDERFLOW)[cols // 2] == 2.0 ** -24
    else:
        assert Q.UNDERFLOW not in labels and row("lone 2^-120")[cols // 2] == 2.0 ** -120
    assert len([l for l in labels if l.startswith("double rounding")]) == (5 if lowp == "f16" else 0)
    assert len(_rows_of("sym", specials)) == 3 and len(_rows_of("zp0", specials)) == 2 and len(_rows_of("span", specials)) == 2
    for i, sp in specials.items():                                          # the extremum sits in the row's last 16-byte chunk
        assert sp.cols[-1] == cols - 1 and len(set(sp.cols.tolist())) == len(sp.cols)


@pytest.mark.parametrize("lowp", ["f16", "bf16"])
@pytest.mark.parametrize("bits", ALL_BITS)
@pytest.mark.parametrize("cols", COLS)
def test_tie_rows_have_power_of_two_scales_and_the_by_hand_digits(cols, lowp, bits):
    b, labels, specials = Q.batch(cols, lowp, bits)
    qmax = 2 ** (bits - 1) - 1
    sym = _rows_of("sym", specials)
    assert len(sym) == 3
    for i, sp in sym:
        assert sp.qmax == qmax and (sp.nbr == 0).sum() >= 3 and (sp.nbr != 0).sum() >= 2, (labels[i], "special elements left")
        ties = sp.u[sp.nbr == 0] % 1 == 0.5
        assert ties.sum() >= min(2 * qmax, 6)
    for sigma in (1.0, 0.5):
        for quant_f16 in (False, True):
            ref = O.rowquant(b, sigma, sigma, quant_f16=quant_f16, lowp=lowp, bits=bits)
            for i, sp in sym:
                assert ref["scale"][i] == 2.0 ** sp.e * sigma, (labels[i], sigma)
                hand = Q.hand_sym_digits(sp, sigma)
                assert np.array_equal(ref["q"][i, sp.cols], hand), (labels[i], sigma, quant_f16)
                if sigma == 0.5 and qmax > 1:                                # ties beyond the clamp on both sides
                    t = (sp.u / sigma)[sp.nbr == 0]
                    assert (t == qmax + 0.5).any() and (t == -qmax - 0.5).any()
                    assert (t == -qmax - 1.5).any() or (lowp == "bf16" and qmax > 63)   # (bf16 has no 64.25)


@pytest.mark.parametrize("lowp", ["f16", "bf16"])
@pytest.mark.parametrize("bits", ALL_BITS)
@pytest.mark.parametrize("cols", COLS)
def test_asymmetric_rows_have_the_by_hand_values(cols, lowp, bits):
    b, labels, specials = Q.batch(cols, lowp, bits)
    x = b.astype(F32)
    qmax = 2 ** bits - 1
    for quant_f16 in (False, True):
        ref = O.rowquant_asym(b, 1.0, 1.0, quant_f16=quant_f16, lowp=lowp, bits=bits).astype(np.float64)
        for i, sp in specials.items():
            if sp.kind == "sym":
                continue
            assert sp.qmax == qmax and (sp.nbr == 0).sum() >= 3
            lo, hi = (0, qmax) if sp.kind == "zp0" else (-(qmax + 1) // 2, (qmax + 1) // 2 - 1)
            assert x[i].min() == lo * 2.0 ** sp.e if lo else x[i].min() >= 0
            assert x[i].max() == hi * 2.0 ** sp.e                         # scale 2^e, zero point 0 / (qmax + 1) / 2
            assert np.array_equal(ref[i, sp.cols], Q.hand_asym_values(sp)), (labels[i], quant_f16)


def test_by_hand_digits_are_round_half_even_then_clamp():
    """hand_digit itself, on values anyone can check"""
    h = lambda u, n, s=1.0: Q.hand_digit(u, n, s, -8, 7)
    assert [h(u, 0) for u in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 6.5, -6.5)] == [0, 2, 2, 0, -2, -2, 6, -6]
    assert [h(0.5, 1), h(0.5, -1), h(-2.5, 1), h(-2.5, -1), h(7.0, 0)] == [1, 0, -2, -3, 7]
    assert [h(3.75, 0, 0.5), h(-3.75, 0, 0.5), h(4.25, 0, 0.5), h(-4.25, 0, 0.5), h(-3.75, -1, 0.5), h(-3.75, 1, 0.5)] == [7, -8, 7, -8, -8, -7]
    assert [h(2.5, 0, 0.5), h(2.5, 1, 0.5), h(-6.5, 0, 0.5)] == [5, 5, -8]


@pytest.mark.parametrize("cols", COLS)
def test_double_rounding_rows_split_the_two_contracts(cols):
    b, labels, _ = Q.batch(cols)
    x = b.astype(F32)
    rows = [i for i, l in enumerate(labels) if l.startswith("double rounding")]
    assert len(rows) == len(Q.DR_SCALES) == 5
    s16 = O.token_scale(x, quant_f16=True)
    for i, sc in zip(rows, Q.DR_SCALES):
        s, m, xs = Q.double_rounding_elements(sc)
        assert np.log2(float(s)) % 1 != 0 and 6 <= len(xs) <= 8
        assert s16[i] == F32(s) and x[i].max() == F32(m) and x[i].min() > -F32(m)          # the row's scale IS s
        for v in np.r_[xs, -xs].astype(F32):
            assert v in x[i]
        t32 = np.abs(xs.astype(F32)) / F32(s)
        assert (np.abs(t32 % 1 - 0.5) > 0).all() and (t32.astype(np.float16).astype(F32) % 1 == 0.5).all()
        q16 = O.quantize(x[i:i + 1], s16[i:i + 1], quant_f16=True)
        q32 = O.quantize(x[i:i + 1], s16[i:i + 1], quant_f16=False)
        assert 1 <= (q16 != q32).sum(), labels[i]
        assert np.array_equal(q16, O.rowquant(b, quant_f16=True)["q"][i:i + 1])


def h16_needs_clamp(x, sig):
    """fq_h16_needs_clamp of csrc/fq_common.hpp restated on the fp16 contract's scale (an underflowed scale: FQ_SCALE_UNDERFLOW)"""
    s = O.token_scale(x, sig[0], sig[1], quant_f16=True)
    s = np.where(s == 0, F32(2.0 ** -100), s).astype(F32)
    with np.errstate(over="ignore"):
        inv = (F32(1) / s).astype(F32)
        return ~((x.max(axis=1) * inv < F32(7.49)) & (x.min(axis=1) * inv > F32(-8.49)))


@pytest.mark.parametrize("lowp", ["f16", "bf16"])
@pytest.mark.parametrize("cols", SMALL + COLS)
def test_every_clip_pair_reaches_the_routes_it_is_listed_for(cols, lowp):
    b, labels, _ = Q.batch(cols, lowp)
    x = b.astype(F32)
    seen = set()
    for sig, want in zip(E.SIGS, E.SIG_ROUTES):
        got = set(E.routes(x, sig).tolist())
        assert want <= got, (sig, got)
        seen |= got
    assert seen == {"plain", "clamp", "div"}
    if lowp == "f16":
        gate = h16_needs_clamp(x, (1.0, 1.0))
        assert gate.any() and not gate.all() and gate[labels.index(Q.UNDERFLOW)]
        assert h16_needs_clamp(x, (0.5, 0.6)).sum() > gate.sum()
        i = labels.index(Q.UNDERFLOW)
        ref = O.rowquant(b, quant_f16=True)
        assert ref["scale16"][i] == 0 and ref["q"][i, cols // 2] == 7 and np.abs(ref["q"][i]).sum() == 7
    # (0.9346, 0.9346) sits ON the clamp guard
    s = O.token_scale(x, 0.9346, 0.9346)
    quot = np.abs(x).max(axis=1) / s
    assert ((quot > 7.48) & (quot < 7.49)).any()


# ------------------------------------------------------------------------------------------------ sensitivity

def model_digits(x, sig, quant_f16, half_away=False, swap_quotient=False, clamp=True, skip_last_chunk=False, with_neighbour=False,
                 underflow_one=False):
    """the symmetric 4-bit quantiser in plain numpy, with switches that each make it WRONG in one way a kernel can be wrong"""
    ext = x[:, :-8] if skip_last_chunk else x
    xmax, xmin = np.maximum(ext.max(axis=1), 0), np.minimum(ext.min(axis=1), 0)
    if with_neighbour:
        xmax, xmin = np.maximum(xmax, np.roll(xmax, -1)), np.minimum(xmin, np.roll(xmin, -1))
    m = np.maximum(np.abs((xmin * F32(sig[1])).astype(F32)), (xmax * F32(sig[0])).astype(F32))
    s = (m / F32(7)).astype(F32)
    if quant_f16:
        s = s.astype(np.float16).astype(F32)
        if underflow_one:
            s = np.where(s == 0, F32(1), s)
    s = np.where(m == 0, F32(1), s).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = (x / s[:, None]).astype(F32)
        if quant_f16 != swap_quotient:
            t = t.astype(np.float16).astype(F32)
    r = np.sign(t) * np.floor(np.abs(t) + F32(0.5)) if half_away else np.rint(t)
    r = np.where(np.isnan(r), 0, r)
    if clamp:
        return np.clip(r, -8, 7).astype(np.int64)
    return (np.clip(r, -2 ** 20, 2 ** 20).astype(np.int64) + 8) % 16 - 8       # the nibble wraps


WRONG = [("half away from zero", dict(half_away=True), (False, True)),
         ("the other contract's quotient", dict(swap_quotient=True), (False, True)),      # fp32 where fp16 is due, and the reverse
         ("no clamp", dict(clamp=False), (False, True)),
         ("extrema skip the last chunk", dict(skip_last_chunk=True), (False, True)),
         ("extrema over the neighbouring row too", dict(with_neighbour=True), (False, True)),
         ("underflowed scale replaced by 1", dict(underflow_one=True), (True,))]


@pytest.mark.parametrize("cols", [64, 136, 2056])
def test_the_batch_tells_wrong_quantisers_from_the_right_one(cols):
    b, labels, _ = Q.batch(cols)
    x = b.astype(F32)
    for quant_f16 in (False, True):
        for sig in Q.SIGS:
            assert np.array_equal(model_digits(x, sig, quant_f16), O.rowquant(b, sig[0], sig[1], quant_f16=quant_f16)["q"]), (sig, quant_f16)
    for name, kw, modes in WRONG:
        for quant_f16 in modes:
            diff = {sig: int((model_digits(x, sig, quant_f16, **kw) != model_digits(x, sig, quant_f16)).sum()) for sig in Q.SIGS}
            assert max(diff.values()) >= 1, (name, quant_f16, diff)
            if name in ("half away from zero", "the other contract's quotient"):          # (1, 1) alone already shows them
                assert diff[(1.0, 1.0)] >= 1, (name, quant_f16, diff)


# ------------------------------------------------------------------------------------------------ NaN cap of the asymmetric 16-bit route

ASYM_SIGS = [s for s in Q.SIGS if s != (1e-7, 1e-7)]      # (1e-7, 1e-7) underflows ordinary rows' fp16 scales too: left out of the route's sweep
OVERFLOW = ("+-65504", "double rounding s=9360.0")        # xmax - xmin leaves fp16: the 16-bit scale is Inf, the row Inf x 0 = NaN


@pytest.mark.parametrize("cols", SMALL + COLS + [520, 4096])
def test_asymmetric_f16_route_nan_rows_are_whole_underflow_rows(cols):
    """the GPU file compares NaN as a class on this route: that is sound only if NaN covers whole rows, few of them, and only rows whose
    16-bit scale is known to be no number: underflowed to 0 (at most 2 rows, labelled so) or — the two rows that span more than 65504, for
    the reason asserted here — overflowed to Inf"""
    assert (1e-7, 1e-7) in Q.SIGS and len(ASYM_SIGS) == len(Q.SIGS) - 1
    b, labels, _ = Q.batch(cols)
    x = b.astype(F32)
    for sig in ASYM_SIGS:
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            ref = O.rowquant_asym(b, sig[0], sig[1], quant_f16=True)
            assert not np.isnan(O.rowquant_asym(b, sig[0], sig[1], quant_f16=False).astype(F32)).any()
            r16 = lambda a: a.astype(np.float16).astype(F32)
            span = r16(r16(np.maximum(x.max(axis=1), 0) * F32(sig[0])) - r16(np.minimum(x.min(axis=1), 0) * F32(sig[1])))
        nan = np.isnan(ref.astype(F32))
        rows = np.flatnonzero(nan.any(axis=1))
        assert nan[rows].all(), (sig, "partly NaN rows")
        under = [i for i in rows if labels[i] == Q.UNDERFLOW]
        over = [i for i in rows if labels[i] in OVERFLOW]
        assert len(under) + len(over) == len(rows), (sig, [labels[i] for i in rows])
        assert len(under) <= 2 and all(np.isinf(span[i]) for i in over) and all(r16(span[i:i + 1] / F32(15))[0] == 0 for i in under)
    bb, _, _ = Q.batch(cols, "bf16")
    for sig in ASYM_SIGS:
        for quant_f16 in (False, True):
            assert not np.isnan(O.rowquant_asym(bb, sig[0], sig[1], quant_f16=quant_f16, lowp="bf16")).any(), sig
