"""Derived references for the launches whose prologue is NOT exact — SiLU.mul, RMSNorm, the Hadamard rotations (numpy and the oracle only; no
GPU, no torch.cuda). tests/test_prologue_ref_cpu.py checks the references themselves, tests/test_gpu_prologue_ref.py holds every launch to them;
DESIGN.md 7.6 has the derivations.

  SiLU.mul  every fp16 gate has a SET of admissible fp16 values: the fp16 roundings of s(g) (1 +- 2 delta(g)), s in float64, delta the
            first-order bound of fq_silu8's five roundings. At most two values, for 0.1 % of the gates.
  RMSNorm   a row is explained by ONE fp32 reciprocal root r' inside [r (1 - 2w), r (1 + 2w)], r in float64: every element equals
            fp16(fp32(x r')). The search enumerates the fp32 values of the window.
  Hadamard  tokens of small integers (sum |x| <= 2047) and single-nonzero tokens under a power-of-two scale: every partial sum in every
            order is exact, so hadK (x) H_P in int64 IS the answer and every route must return its bits.

U_RSQ / U_EXP / U_RCP are max(1, measured) fp32 ulps of v_rsq_f32 / v_exp_f32 / v_rcp_f32 (profiles/prologue_ref.txt; the GPU file measures
them again and asserts that they do not exceed these)."""
import numpy as np

from oracle import fq_oracle as O

F16, F32, F64 = np.float16, np.float32, np.float64
U_RSQ, U_EXP, U_RCP = 1.0, 1.0, 1.0
U_CAP = 2.0                                        # above this the first-order terms of the derivations no longer hold
LOG2E32 = F32(1.44269504088896340736)

# ---------------------------------------------------------------------------------------------------------------- special functions

SFU_RANGES = {"rsq": (1e-20, 1e10), "exp2": (-150.0, 150.0), "rcp": (1.0, 3.4e38)}   # what the kernels feed them (rsq from 1e-20: one 6e-8 in 16384, eps = 0)


def sfu_inputs(op, n=1 << 20, seed=0):
    """about 2^20 fp32 inputs over the range the kernels feed `op`: log-uniform (rsq, rcp) / uniform (exp2), the end points, powers of two"""
    rng = np.random.default_rng([seed, len(op)])
    lo, hi = SFU_RANGES[op]
    if op == "exp2":
        x = rng.uniform(lo, hi, n)
        extra = np.arange(-150, 151, dtype=F64)
    else:
        x = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
        extra = 2.0 ** np.arange(np.ceil(np.log2(lo)), np.floor(np.log2(hi)) + 1)
    x = np.concatenate([x, extra, [lo, hi]]).astype(F32)
    if op == "rcp":
        x = np.concatenate([x, np.array([np.inf, np.finfo(F32).max], F32)])
    return x


def sfu_exact(op, x32):
    x = np.asarray(x32, F64)
    with np.errstate(divide="ignore", over="ignore"):
        return {"rsq": lambda: 1.0 / np.sqrt(x), "exp2": lambda: np.exp2(x), "rcp": lambda: 1.0 / x}[op]()


def ulp_error(got32, exact64):
    """largest |got - exact| in units of the fp32 ulp of `exact` (normal results only: below 2^-126 the hardware may flush, and no kernel's
    result depends on it — see DESIGN 7.6); an exact 0 / Inf must be returned as such"""
    got, ex = np.asarray(got32, F64), np.asarray(exact64, F64)
    special = (ex == 0) | ~np.isfinite(ex)
    assert np.array_equal(got[special], ex[special])
    m = ~special & (np.abs(ex) >= 2.0 ** -126) & (np.abs(ex) <= float(np.finfo(F32).max))
    ulp = 2.0 ** (np.floor(np.log2(np.abs(ex[m]))) - 23)
    return float(np.max(np.abs(got[m] - ex[m]) / ulp))


# ---------------------------------------------------------------------------------------------------------------- A. SiLU.mul

def all_gates():
    """the 65536 fp16 bit patterns, in pattern order"""
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(F16)


def silu_exact(g16):
    g = np.asarray(g16, F16).astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        return g / (1.0 + np.exp(-g))


def silu_delta(g16, u_exp=U_EXP, u_rcp=U_RCP):
    """first-order bound of the relative error of fq_silu8's fp32 result: t = fl(g c) with c itself rounded (1.5 |g| 2^-24 on the exponent,
    i.e. relative on e), exp2 (u_exp ulp) — both reach the result through e / (1 + e) = sigma(-g) —, 1 + e (2^-24, bounded by the term
    below), rcp (u_rcp ulp), the product (2^-24 -> with the sum's: 2^-23)"""
    g = np.asarray(g16, F16).astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        sig_neg = 1.0 / (1.0 + np.exp(g))
        return sig_neg * (1.5 * np.abs(g) * 2.0 ** -24 + u_exp * 2.0 ** -23) + u_rcp * 2.0 ** -23 + 2.0 ** -23


def silu_admissible(g16, u_exp=U_EXP, u_rcp=U_RCP):
    """-> (lo16, hi16): the admissible fp16 values of silu(g) are the fp16 values from lo16 to hi16 (the roundings of s (1 -+ 2 delta); rounding
    is monotone). Signed zero: that of g. +Inf -> +Inf, -Inf and NaN -> NaN."""
    g = np.asarray(g16, F16)
    s, d = silu_exact(g), silu_delta(g, u_exp, u_rcp)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = (s * (1.0 - 2.0 * d)).astype(F16), (s * (1.0 + 2.0 * d)).astype(F16)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
    inf = np.isposinf(g.astype(F32))
    lo, hi = np.where(inf, F16(np.inf), lo), np.where(inf, F16(np.inf), hi)
    bad = np.isnan(g.astype(F32)) | np.isneginf(g.astype(F32))
    return np.where(bad, F16(np.nan), lo).astype(F16), np.where(bad, F16(np.nan), hi).astype(F16)


def n_admissible(lo16, hi16):
    """how many fp16 values lie in [lo, hi] (same sign or zero: counted on the bit patterns)"""
    lo, hi = lo16.view(np.uint16).astype(np.int64), hi16.view(np.uint16).astype(np.int64)
    key = lambda b: np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)    # monotone in the value; +-0 coincide
    return key(hi) - key(lo) + 1


def in_set(got16, cands16):
    """got [..] fp16 equals, BIT FOR BIT (NaN as a class), one of the candidates cands [k, ..] -> bool array"""
    got = np.asarray(got16, F16)
    ok = np.zeros(got.shape, bool)
    for c in cands16:
        c = np.asarray(c, F16)
        ok |= (got.view(np.uint16) == c.view(np.uint16)) | (np.isnan(got) & np.isnan(c))
    return ok


def silu8_emulated(g16, c=LOG2E32):
    """fq_silu8 in numpy: fp32 throughout, numpy's exp2 and division for v_exp_f32 / v_rcp_f32"""
    g = np.asarray(g16, F16).astype(F32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp2((g * -F32(c)).astype(F32), dtype=F32)
        return (g * (F32(1.0) / (F32(1.0) + e)).astype(F32)).astype(F32).astype(F16)


def mul16(a16, up16):
    """the fp16 product: exact in fp32 (22 significant bits), rounded once"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a16, F16).astype(F32) * np.asarray(up16, F16).astype(F32)).astype(F16)


UPS = np.array([1, -1, 0.5, 3, 2.0 ** -14, 6e-8, 65504, 0, -0.0, np.inf], F16)
SWEEP_MAX = 24.0


def sweep_gates():
    """every fp16 gate with |g| <= 24, in pattern order (39938 of them)"""
    g = all_gates()
    return g[np.abs(g.astype(F32)) <= SWEEP_MAX]


def sweep_tokens(width, seed=0):
    """-> (gate, up) fp16 [rows, width]: the sweep gates in pattern order, then in a seeded shuffle, each cut into tokens of `width` (the last
    token of each filled up from the front); up drawn from +-{0.25, 0.5, 1, 2}"""
    g = sweep_gates()
    rng = np.random.default_rng([width, seed, 5])
    rows = -(-g.size // width)
    parts = [np.resize(o, rows * width).reshape(rows, width) for o in (g, g[rng.permutation(g.size)])]
    gate = np.concatenate(parts)
    up = (rng.choice(np.array([.25, .5, 1, 2], F32), gate.shape) * rng.choice(np.array([-1, 1], F32), gate.shape)).astype(F16)
    return np.ascontiguousarray(gate), up


def edge_up(batch16):
    """`up` for E.batch as the gate under factors over {-1, -2}: 1 everywhere, 0.5 for the token holding 15000 — 4 |product| stays finite"""
    up = np.ones(batch16.shape, F16)
    up[np.abs(batch16.astype(F32)).max(axis=1) > 8192] = F16(0.5)
    lo, hi = silu_admissible(batch16)
    for a in (lo, hi):
        assert np.isfinite(4.0 * mul16(a, up).astype(F32)).all()
    return up


# ---------------------------------------------------------------------------------------------------------------- B. RMSNorm

def rms_width(d_pad, u_rsq=U_RSQ):
    """relative bound of the kernels' fp32 reciprocal root, in units of 2^-24 BEFORE the doubling: the sum is four fma chains per lane of
    d_pad / 256 non-negative terms, two adds, six reduction stages (half a rounding each on the root), the division and the add (one each,
    halved by the root, taken whole), the rsq (u_rsq ulp = 2 u_rsq 2^-24)"""
    return (d_pad / 256 + 10) / 2 + 2 + 2 * u_rsq


def rms_root(x16, eps):
    x = np.asarray(x16, F16).astype(F64)
    with np.errstate(divide="ignore"):
        return 1.0 / np.sqrt((x * x).mean(axis=-1) + float(F32(eps)))


def _f32_between(lo, hi):
    """every positive fp32 value in [lo, hi]"""
    a = np.array([lo, hi], F64).astype(F32)
    a[0] = a[0] if float(a[0]) >= lo else np.nextafter(a[0], F32(np.inf))
    a[1] = a[1] if float(a[1]) <= hi else np.nextafter(a[1], F32(0))
    b = a.view(np.uint32).astype(np.int64)
    return np.arange(b[0], b[1] + 1).astype(np.uint32).view(F32)


def rms_candidates(x16_row, eps, d_pad, u_rsq=U_RSQ):
    """-> (r float64, the fp32 candidates of the doubled window); a zero row at eps = 0: (inf, [inf])"""
    r = float(rms_root(x16_row, eps))
    if not np.isfinite(r):
        return r, np.array([np.inf], F32)
    w = 2.0 * rms_width(d_pad, u_rsq) * 2.0 ** -24
    return r, _f32_between(r * (1 - w), r * (1 + w))


def rms_apply(x16_row, cands32):
    """fp16(fp32(x r')) for every candidate -> [n_cand, d]: round to fp32, then to fp16, as fq_mul_to does"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(x16_row, F16).astype(F32)[None, :] * np.asarray(cands32, F32)[:, None]).astype(F32).astype(F16)


def rms_search(x16_row, y16_row, eps, d_pad, u_rsq=U_RSQ):
    """-> (r, candidates, accepted mask): the candidates that explain EVERY element of the row, bit for bit (NaN as a class)"""
    r, cands = rms_candidates(x16_row, eps, d_pad, u_rsq)
    ok = in_set(np.broadcast_to(np.asarray(y16_row, F16), (len(cands), len(y16_row))), [rms_apply(x16_row, cands)]).all(axis=1)
    return r, cands, ok


def rms_deviation(r, cands, ok):
    """|centre of the accepted candidates / r - 1| in units of 2^-24 (0 for the non-finite root)"""
    if not np.isfinite(r):
        return 0.0
    acc = cands[ok].astype(F64)
    return abs((acc.min() + acc.max()) / 2 / r - 1) * 2.0 ** 24


def rmsnorm_wave_model(x16, eps):
    """the standalone kernel's order in numpy: lane l holds the 16-byte chunks l, l + 64, ...; four fma chains per lane (element e of a chunk
    feeds chain e & 3, here: fp32 product and add — the double rounding of the unfused form stays inside the window), (s0 + s1) + (s2 + s3),
    six butterfly stages, / cols + eps, 1 / sqrt, fp16(fp32(x r))"""
    x = np.asarray(x16, F16).astype(F32)
    rows, d = x.shape
    nch = -(-(d // 8) // 64)
    xp = np.zeros((rows, nch * 64 * 8), F32)
    xp[:, :d] = x
    v = xp.reshape(rows, nch, 64, 2, 4)                                    # [row, k, lane, half, chain]
    ss = np.zeros((rows, 64, 4), F32)
    for k in range(nch):
        for h in range(2):
            ss = (ss + (v[:, k, :, h, :] * v[:, k, :, h, :]).astype(F32)).astype(F32)
    t = ((ss[..., 0] + ss[..., 1]).astype(F32) + (ss[..., 2] + ss[..., 3]).astype(F32)).astype(F32)
    for s in (1, 2, 4, 8, 16, 32):
        t = (t + t[:, np.arange(64) ^ s]).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (F32(1) / np.sqrt((t[:, :1] / F32(d)).astype(F32) + F32(eps), dtype=F32)).astype(F32)
        return (x * r).astype(F32).astype(F16)


def rms_rows(cols):
    """E.batch at width `cols` (its 25 rows first, so a tiled launch can index them), plus rows of constant 65504, one-hot 65504 and a
    single 6e-8"""
    from tests import edge_tokens as E
    b = E.batch(1, cols)
    extra = np.zeros((3, cols), F16)
    extra[0] = 65504
    extra[1, cols // 3] = 65504
    extra[2, cols - 1] = 6e-8
    return np.ascontiguousarray(np.concatenate([b, extra]).astype(F16))


# ---------------------------------------------------------------------------------------------------------------- C. Hadamard

HAD_SCALES = (1.0, 2.0 ** -7)
SINGLE_VALUES = (1.0, -3.0, 15000.0, 65504.0, 2.0 ** -4)
SUM_CAP = 2047


def sylvester(n):
    h = np.ones((1, 1), np.int64)
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


def had_tokens(n, K, seed=0):
    """-> (x fp16 [rows, n], single [rows] bool): sparse integer tokens with sum |x| <= 2047, the zero token, single-nonzero tokens"""
    P = n // K
    rng = np.random.default_rng([n, K, seed])
    rows = []

    def sparse(count, top, lo=0, hi=n):
        t = np.zeros(n, F32)
        pos = lo + rng.choice(hi - lo, min(count, hi - lo), replace=False)
        t[pos] = rng.integers(1, top + 1, pos.size) * rng.choice([-1, 1], pos.size)
        return t

    rows += [sparse(SUM_CAP, 1), sparse(SUM_CAP, 1), sparse(SUM_CAP // 7, 7), sparse(SUM_CAP // 7, 7)]
    blk = int(rng.integers(0, K))
    rows += [sparse(min(P, SUM_CAP // 7), 7, blk * P, (blk + 1) * P), sparse(min(P, SUM_CAP // 7), 7, n - P, n), np.zeros(n, F32)]
    n_multi = len(rows)
    fixed = sorted({0, 1, P - 1, P % n, n - P, n - 1})
    positions = fixed + list(rng.choice(n, 16, replace=False))
    for i, p in enumerate(positions):
        for c in (SINGLE_VALUES if i < len(fixed) else (SINGLE_VALUES[i % len(SINGLE_VALUES)],)):
            t = np.zeros(n, F32)
            t[p] = c
            rows.append(t)
    x = np.stack(rows).astype(F16)
    single = np.arange(len(rows)) >= n_multi
    return x, single


def had_keep(x16, single, scale):
    """the rows a scale admits: sparse tokens under power-of-two scales only; single-nonzero tokens with |c| scale / 32 >= 2^-14 (no fp16
    subnormal in any route's intermediate: whether the matrix pipe keeps them is unmeasured)"""
    amax = np.abs(x16.astype(F64)).max(axis=1)
    pow2 = float(np.log2(scale)).is_integer()
    return np.where(single, amax * scale / 32 >= 2.0 ** -14, pow2)


def had_int(x16, K, hadK):
    """hadK (x) H_P in int64 on integer-valued tokens [rows, n] -> int64 [rows, n]"""
    x = np.asarray(x16, F64)
    xi = x.astype(np.int64)
    assert np.array_equal(xi, x)
    rows, n = xi.shape
    v = xi.reshape(rows, K, n // K).copy()
    h = 1
    while h < n // K:                                                       # H_P as log2(P) butterfly stages (Sylvester order), exact integers
        w = v.reshape(rows, K, -1, 2, h)
        a, b = w[..., 0, :].copy(), w[..., 1, :].copy()
        w[..., 0, :], w[..., 1, :] = a + b, a - b
        h *= 2
    if K > 1:
        v = np.einsum("jk,rkp->rjp", np.asarray(hadK, F64).astype(np.int64), v)
    return v.reshape(rows, n)


def had_exact(x16, K, hadK, scale):
    """the rotation's fp16 bits on tokens that are integers times ONE power of two per row (2^-4: brought to integers first): exact in float64,
    asserted representable -> fp16 [rows, n]"""
    x = np.asarray(x16, F16).astype(F64)
    unit = np.where((x != np.rint(x)).any(axis=1), 2.0 ** -4, 1.0)[:, None]
    y = had_int(x / unit, K, hadK).astype(F64) * unit * float(scale)
    y16 = y.astype(F16)
    assert np.array_equal(y16.astype(F64), y), "not representable in fp16"
    return y16


def had_single_default(x16, K, hadK, s32):
    """single-nonzero tokens at an arbitrary fp32 scale: fp16(fp32(+-c s))"""
    sign = had_int(np.sign(x16.astype(F32)).astype(F16), K, hadK).astype(F32)          # the column of signs the token reads
    c = np.abs(x16.astype(F32)).max(axis=1, keepdims=True)
    with np.errstate(over="ignore"):
        return (sign * (c * F32(s32)).astype(F32)).astype(F32).astype(F16)
