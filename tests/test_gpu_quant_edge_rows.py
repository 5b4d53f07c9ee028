"""Edge rows through every standalone quantiser launch of csrc/fq_quant.hip, bit for bit (builders: tests/quant_edge_rows.py; their own
checks: tests/test_quant_edge_rows_cpu.py).

The batch is under 60 rows: zero / single-signed / one-hot / outlier / subnormal / constant / +-65504 rows, tie rows whose scale is a power of
two (digits prescribed BY HAND as well as by the oracle), double-rounding rows on which the fp16 and the fp32 contract legitimately differ,
and closed-form asymmetric rows — each between two ordinary Gaussian rows. The row lengths reach every build fq_launch_rowquant can select:
lane groups of 1 .. 32 lanes, a wave per row with 4 / 8 / 16 / 24 chunks per lane, a workgroup per row with 8 / 16, and the asymmetric
kernel with 1 / 4 / 8 register vectors or the row read twice — each with a partly filled last chunk, lane or lane group. Every launch
carries several clip pairs (at most FQ_MAX_CLIPS). Every assertion is BIT EQUALITY; on the asymmetric 16-bit route NaN is compared as a
class at the oracle's positions (whole rows whose 16-bit scale is 0 or Inf: the CPU file bounds them)."""
import numpy as np
import pytest
import torch

from oracle import fq_oracle as O
from tests import quant_edge_rows as Q

# (the oracle divides by underflowed scales and overflows fp16 on purpose on these rows)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
P, F, NC0, Q16, S16, ASYM, RPOST = 0x01, 0x02, 0x10, 0x20, 0x400, 0x800, 0x10000
MAX_CLIPS = 4
F32 = np.float32
LANE_GROUP = [8, 16, 24, 64, 128, 136, 256]                 # 1 .. 32 lanes per row, several rows per wave
WAVE = [264, 2048, 2056, 4104, 8200, 12288]                 # a wave per row: 4, 8, 16, 24 chunks per lane
WORKGROUP = [12296, 16392, 32768]                           # a workgroup per row: 8 and 16 chunks per thread
SYM_COLS = LANE_GROUP + WAVE + WORKGROUP
ASYM_COLS = SYM_COLS + [520, 4096]                          # (4 and 8 register vectors at a full wave per row)
ASYM_SIGS_16 = [s for s in Q.SIGS if s != (1e-7, 1e-7)]     # (ordinary rows' fp16 scales underflow under it: tests/test_quant_edge_rows_cpu.py)
ARITH = [("fp32", 0, {}), ("Q16", Q16, dict(quant_f16=True)), ("Q16|S16", Q16 | S16, dict(quant_f16=True, sig_f16=True))]
LOWP = ["f16", "bf16"]


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import _lib, ops as _ops
    assert (_lib.FQ_OUT_PACKED, _lib.FQ_OUT_FAKEQUANT, _lib.FQ_NO_CLAMP0, _lib.FQ_QUANT_F16, _lib.FQ_SIG_F16, _lib.FQ_ASYM, _lib.FQ_RATIO_POST,
            _lib.FQ_MAX_CLIPS) == (P, F, NC0, Q16, S16, ASYM, RPOST, MAX_CLIPS)
    return _ops


def dev(a, lowp="f16"):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(torch.bfloat16) if lowp == "bf16" else t).cuda()


def bits16(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def ref_bits(a, lowp):
    return O.bf16_bits(a) if lowp == "bf16" else np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def values(bits, lowp):
    return O.bf16_from_bits(bits) if lowp == "bf16" else bits.view(np.float16).astype(F32)


def sigs_for(lowp, aflag):
    """FQ_SIG_F16 on bf16 data multiplies with the bf16-rounded factor (the caller passes it so): clip pairs bf16 represents exactly"""
    if lowp == "bf16" and aflag & S16:
        return [(float(O.bf16_round(F32(a))), float(O.bf16_round(F32(b)))) for a, b in Q.SIGS]
    return Q.SIGS


def chunks(sigs):
    return [sigs[k:k + MAX_CLIPS] for k in range(0, len(sigs), MAX_CLIPS)]


def differ(ctx, labels, x, scale, got, want):
    """'' when got == want, else the failure message: dtype / cols / flags / clip pair (ctx), the first differing row's label, its first
    differing elements with their quotients"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    bad = got != want
    if not bad.any():
        return ""
    r = int(np.flatnonzero(bad.reshape(len(bad), -1).any(axis=1))[0])
    if bad.ndim == 1:
        return f"{ctx}: {int(bad.sum())} rows differ, first row {r} ({labels[r]}): got {got[r]!r}, want {want[r]!r}"
    cs = np.flatnonzero(bad[r])[:6]
    with np.errstate(all="ignore"):
        quot = x[r, cs].astype(F32) / F32(scale[r]) if scale is not None else None
    return (f"{ctx}: {int(bad.sum())} elements differ in {int(bad.any(axis=1).sum())} rows; first row {r} ({labels[r]}), cols {cs.tolist()}: "
            f"x = {x[r, cs].tolist()}, scale = {None if scale is None else float(scale[r])!r}, x / scale = {None if quot is None else quot.tolist()}, "
            f"got {got[r, cs].tolist()}, want {want[r, cs].tolist()}")


def check_sym(o, ci, ref, outs, lowp, ctx, b, labels, specials, sig):
    rows, cols = b.shape
    x = b.astype(F32)
    if outs & P:
        got = O.unpack_i4(o.q[ci].reshape(rows, -1).cpu().numpy())
        assert not (m := differ(ctx + " digits", labels, x, ref["scale"], got, ref["q"].astype(np.int32))), m
        assert not (m := differ(ctx + " scale bits", labels, x, None, bits16(o.scale[ci]).reshape(-1), ref_bits(ref["scale16"], lowp).reshape(-1))), m
        if sig in Q.TIE_SIGS:                                  # the by-hand table, no oracle involved
            for i, sp in specials.items():
                if sp.kind == "sym":
                    hand = Q.hand_sym_digits(sp, sig[0])
                    assert np.array_equal(got[i, sp.cols], hand), (ctx, labels[i], "by hand", sp.cols.tolist(), got[i, sp.cols].tolist(), hand.tolist())
    if outs & F:
        got = bits16(o.fq[ci]).reshape(rows, cols)
        assert not (m := differ(ctx + " fake-quant bits", labels, x, ref["scale"], got, ref_bits(ref["fq"], lowp))), m


def asym_scale(x, sig, qmax):
    """(for failure messages only) the fp32 route's scale"""
    return (np.maximum(x.max(axis=1), 0) * F32(sig[0]) - np.minimum(x.min(axis=1), 0) * F32(sig[1])) / F32(qmax)


def check_asym(got_t, ref, lowp, ctx, b, labels, specials, sig, qmax):
    """bit for bit; NaN as a class, at the oracle's positions"""
    x = b.astype(F32)
    got = bits16(got_t).reshape(b.shape)
    want = ref_bits(np.where(np.isnan(ref), 0, ref), lowp)
    gv = values(got, lowp)
    nan_g, nan_w = np.isnan(gv), np.isnan(np.asarray(ref, F32))
    sc = asym_scale(x, sig, qmax)
    assert not (m := differ(ctx + " NaN positions", labels, x, sc, nan_g, nan_w)), m
    assert not (m := differ(ctx + " fake-quant bits", labels, x, sc, np.where(nan_w, 0, got), np.where(nan_w, 0, want))), m
    if sig == (1.0, 1.0):
        for i, sp in specials.items():
            if sp.kind != "sym":
                hand = Q.hand_asym_values(sp)
                assert np.array_equal(gv[i, sp.cols].astype(np.float64), hand), (ctx, labels[i], "by hand", gv[i, sp.cols].tolist(), hand.tolist())


# ------------------------------------------------------------------------------------------------ fq_rowquant_*: symmetric

SYM_CASES = [(name, aflag, kw, (P, F, P | F)) for name, aflag, kw in ARITH] + [("fp32 NC0", NC0, dict(clamp0=False), (P,))]


@pytest.mark.parametrize("lowp", LOWP)
@pytest.mark.parametrize("name,aflag,kw,out_sets", SYM_CASES, ids=[c[0].replace("|", "+").replace(" ", "+") for c in SYM_CASES])
@pytest.mark.parametrize("cols", SYM_COLS)
def test_symmetric_rowquant_every_output_set_and_arithmetic(ops, cols, name, aflag, kw, out_sets, lowp):
    b, labels, specials = Q.batch(cols, lowp)
    x = dev(b, lowp)
    sigs = sigs_for(lowp, aflag)
    refs = [O.rowquant(b, s[0], s[1], lowp=lowp, **kw) for s in sigs]               # once per arithmetic, shared by the output sets
    for outs in out_sets:
        k = 0
        for group in chunks(sigs):
            o = ops.rowquant(x, group, outs | aflag)
            for ci, sig in enumerate(group):
                ctx = f"rowquant {lowp} cols={cols} flags={hex(outs | aflag)} ({name}) clip={sig}"
                check_sym(o, ci, refs[k + ci], outs, lowp, ctx, b, labels, specials, sig)
            k += len(group)


@pytest.mark.parametrize("cols", SYM_COLS)
def test_ratio_post_against_the_plain_quantizer(ops, cols):
    """deploy.nn.Quantizer(input_clip_ratio): scale = fp16(max|x| / 7) * ratio with no zero guard, then sym_quant"""
    b, labels, _ = Q.batch(cols)
    ratios = [1.0, 0.9, 0.83]
    o = ops.rowquant(dev(b), [(r, 1.0) for r in ratios], P | Q16 | RPOST)
    x = b.astype(F32)
    for ci, r in enumerate(ratios):
        packed, s = O.quantizer_plain(b, r)
        ctx = f"rowquant f16 cols={cols} flags={hex(P | Q16 | RPOST)} ratio={r}"
        assert s[labels.index("all zero")] == 0
        assert not (m := differ(ctx + " scale bits", labels, x, None, bits16(o.scale[ci]).reshape(-1), s.view(np.uint16))), m
        got = O.unpack_i4(o.q[ci].cpu().numpy())
        assert not (m := differ(ctx + " digits", labels, x, s.astype(F32), got, O.unpack_i4(packed))), m


# ------------------------------------------------------------------------------------------------ fq_rowquant_*: FQ_ASYM

@pytest.mark.parametrize("lowp", LOWP)
@pytest.mark.parametrize("cols", ASYM_COLS)
def test_asymmetric_rowquant_both_arithmetics(ops, cols, lowp):
    b, labels, specials = Q.batch(cols, lowp)
    x = dev(b, lowp)
    for f16a in (False, True):
        flags = F | ASYM | (Q16 if f16a else 0)
        for group in chunks(ASYM_SIGS_16 if f16a else Q.SIGS):
            o = ops.rowquant(x, group, flags)
            for ci, sig in enumerate(group):
                with np.errstate(all="ignore"):
                    ref = O.rowquant_asym(b, sig[0], sig[1], quant_f16=f16a, lowp=lowp)
                check_asym(o.fq[ci], ref, lowp, f"rowquant {lowp} cols={cols} flags={hex(flags)} clip={sig}", b, labels, specials, sig, 15)


# ------------------------------------------------------------------------------------------------ fq_sym_quant_f16

@pytest.mark.parametrize("cols", [8, 64, 136, 2056, 4104, 12296, 63, 4097])
def test_sym_quant_with_the_batchs_own_halved_and_zero_scales(ops, cols):
    """both kernels: 16-byte chunks (cols % 8 == 0) and the element kernel with the odd tail"""
    b, labels, _ = Q.batch(cols)
    x = b.astype(F32)
    s = O.token_scale(x, quant_f16=True).astype(np.float16)                  # (the lone-subnormal row's is 0 already)
    s[labels.index("all zero")] = 0                                          # 0 / 0: digit 0
    assert s[labels.index(Q.UNDERFLOW)] == 0
    for name, sc in (("own", s), ("halved", (s.astype(F32) * F32(0.5)).astype(np.float16))):
        got = ops.sym_quant(dev(b), dev(sc)).cpu().numpy()
        want = O.sym_quant(b, sc)
        pad = lambda p: O.unpack_i4(p)[:, :cols + (cols & 1)]
        xp = np.concatenate([x, np.zeros((len(x), cols & 1), F32)], axis=1)
        assert not (m := differ(f"sym_quant f16 cols={cols} scales={name}", labels, xp, sc.astype(F32), pad(got), pad(want))), m


# ------------------------------------------------------------------------------------------------ fq_fakequant_bits_*

@pytest.mark.parametrize("lowp", LOWP)
@pytest.mark.parametrize("bits", [2, 3, 4, 5, 6, 7, 8])
def test_fakequant_bits_symmetric_and_asymmetric(ops, bits, lowp):
    for cols in (64, 520, 4104):
        b, labels, specials = Q.batch(cols, lowp, bits)
        x, x32 = dev(b, lowp), b.astype(F32)
        rows = len(b)
        for name, aflag, kw in ARITH:
            for sig in sigs_for(lowp, aflag):
                ref = O.rowquant(b, sig[0], sig[1], lowp=lowp, bits=bits, **kw)
                ctx = f"fakequant_bits {lowp} bits={bits} cols={cols} flags={hex(aflag)} ({name}) clip={sig}"
                got = bits16(ops.fakequant_bits(x, sig, bits, aflag)).reshape(rows, cols)
                assert not (m := differ(ctx, labels, x32, ref["scale"], got, ref_bits(ref["fq"], lowp))), m
                if sig in Q.TIE_SIGS:                          # by hand: the value is digit x scale, scale = 2^e x sigma
                    gv = values(got, lowp).astype(np.float64)
                    for i, sp in specials.items():
                        if sp.kind == "sym":
                            hand = Q.hand_sym_digits(sp, sig[0]) * 2.0 ** sp.e * sig[0]
                            assert np.array_equal(gv[i, sp.cols], hand), (ctx, labels[i], "by hand", gv[i, sp.cols].tolist(), hand.tolist())
        for f16a in (False, True):
            flags = ASYM | (Q16 if f16a else 0)
            for sig in (ASYM_SIGS_16 if f16a else Q.SIGS):
                with np.errstate(all="ignore"):
                    ref = O.rowquant_asym(b, sig[0], sig[1], quant_f16=f16a, lowp=lowp, bits=bits)
                ctx = f"fakequant_bits {lowp} bits={bits} cols={cols} flags={hex(flags)} clip={sig}"
                check_asym(ops.fakequant_bits(x, sig, bits, flags), ref, lowp, ctx, b, labels, specials, sig, 2 ** bits - 1)


# ------------------------------------------------------------------------------------------------ neighbour independence

INDEP_SIGS = [(1.0, 1.0), (3e-6, 1.0), (0.5, 0.6)]            # magic-number rounding, true division, the clamp


def raw(o):
    return [t if t.dtype == torch.uint8 else t.view(torch.int16) for t in list(o.q) + list(o.scale) + list(o.fq) if t is not None]


@pytest.mark.parametrize("lowp", LOWP)
@pytest.mark.parametrize("cols", [16, 128, 2056, 12296])
def test_an_edge_row_alone_gives_the_bytes_it_gave_inside_the_batch(ops, cols, lowp):
    """no reference needed: in the lane-group builds the row shared its wave (extrema butterflies, the exact-division vote) with ordinary rows"""
    b, labels, _ = Q.batch(cols, lowp)
    x = dev(b, lowp)
    n = len(b)
    for flags in (P | F, P | F | Q16, F | ASYM, F | ASYM | Q16):
        base = raw(ops.rowquant(x, INDEP_SIGS, flags))
        assert base
        for i in range(1, n, 2):
            alone = raw(ops.rowquant(x[i:i + 1].contiguous(), INDEP_SIGS, flags))
            for k, (a, g) in enumerate(zip(base, alone)):
                assert torch.equal(g.reshape(1, -1), a.reshape(n, -1)[i:i + 1]), (lowp, cols, hex(flags), labels[i], "output tensor", k)


# ------------------------------------------------------------------------------------------------ the modules

def test_modules_equal_the_flag_combinations_they_stand_for(ops):
    from flatquant_amd import deploy
    from flatquant_amd.flatquant.quant_utils import ActivationQuantizer
    cols = 4096
    b, labels, specials = Q.batch(cols)
    x, x32, rows = dev(b), b.astype(F32), len(b)
    same = lambda t, u: torch.equal(t.reshape(rows, -1).view(torch.int16) if t.dtype != torch.uint8 else t.reshape(rows, -1),
                                    u.reshape(rows, -1).view(torch.int16) if u.dtype != torch.uint8 else u.reshape(rows, -1))

    sig = ops.sigmoid_pair_f16(4.0, 4.0)
    p = deploy.nn.Quantizer(lac=True).cuda()(x)
    o = ops.rowquant(x, [sig], P | Q16 | S16)
    assert same(p.quantized_x, o.q[0]) and same(p.scales_x, o.scale[0]), "Quantizer(lac=True)"
    check_sym(o, 0, O.rowquant(b, sig[0], sig[1], quant_f16=True, sig_f16=True), P, "f16", f"Quantizer(lac=True) cols={cols}", b, labels, specials, sig)

    p = deploy.nn.Quantizer(input_clip_ratio=0.9).cuda()(x)
    o = ops.rowquant(x, [(0.9, 1.0)], P | Q16 | RPOST)
    assert same(p.quantized_x, o.q[0]) and same(p.scales_x, o.scale[0]) and p.scales_x.shape == (rows, 1), "Quantizer(input_clip_ratio=0.9)"
    packed, s = O.quantizer_plain(b, 0.9)
    assert not (m := differ("Quantizer(input_clip_ratio=0.9) scale bits", labels, x32, None, bits16(p.scales_x).reshape(-1), s.view(np.uint16))), m
    assert not (m := differ("Quantizer(input_clip_ratio=0.9) digits", labels, x32, s.astype(F32), O.unpack_i4(p.quantized_x.cpu().numpy()),
                            O.unpack_i4(packed))), m

    sig32 = ops.sigmoid_pair(4.0, 4.0)
    for lac, flags, sg, kw in ((True, F, sig32, {}), (False, F | Q16, (1.0, 1.0), dict(quant_f16=True))):
        with torch.no_grad():
            y = ActivationQuantizer(bits=4, sym=True, lac=lac).cuda()(x)
        o = ops.rowquant(x, [sg], flags)
        assert same(y, o.fq[0]), ("ActivationQuantizer(sym=True)", lac)
        check_sym(o, 0, O.rowquant(b, sg[0], sg[1], **kw), F, "f16", f"ActivationQuantizer(4, sym=True, lac={lac}) cols={cols}", b, labels, specials, sg)
    for lac, flags, sg in ((True, F | ASYM, sig32), (False, F | ASYM | Q16, (1.0, 1.0))):
        with torch.no_grad():
            y = ActivationQuantizer(bits=4, sym=False, lac=lac).cuda()(x)
        o = ops.rowquant(x, [sg], flags)
        assert same(y, o.fq[0]), ("ActivationQuantizer(sym=False)", lac)
        with np.errstate(all="ignore"):
            ref = O.rowquant_asym(b, sg[0], sg[1], quant_f16=not lac)
        check_asym(y, ref, "f16", f"ActivationQuantizer(4, sym=False, lac={lac}) cols={cols}", b, labels, specials, tuple(sg), 15)
