"""Edge rows for the standalone quantisers of csrc/fq_quant.hip: shared builders (numpy only; no GPU, no torch.cuda).

The input of fq_rowquant_* / fq_sym_quant_f16 / fq_fakequant_bits_* IS the quantiser's operand, so a row can prescribe its own scale and
quotients: `batch(cols, lowp, bits)` puts ordinary Gaussian rows at the even positions and edge rows at the odd ones (an odd row count:
in the lane-group builds every edge row shares its wave with ordinary rows and the last lane group of the last wave is partly idle).
Three kinds of edge row carry SPECIAL elements whose digits are written down here by hand (round half to even, then clamp — hand_digit
never calls the oracle), each a `Special` in the returned dict:
  "sym"   extremum qmax 2^e, so the scale under the clip pair (1, 1) is exactly 2^e, under (0.5, 0.5) 2^(e-1); elements (k + 0.5) 2^e with
          their 16-bit neighbours below and above, and +-(qmax + 0.5) / 2, +-(qmax + 1.5) / 2 (x 2^e): ties beyond the clamp under (0.5, 0.5)
  "zp0"   asymmetric, non-negative, maximum qmax 2^e: scale 2^e, zero point 0
  "span"  asymmetric, from -h 2^e to (h - 1) 2^e with h = (qmax + 1) / 2: scale 2^e, zero point h
The double-rounding rows (fp16, bits = 4) hold every fp16 x below the extremum whose fp16 quotient by the row's fp16 scale s rounds ONTO a
tie k + 0.5 without x / s being one: the fp16 and the fp32 contract legitimately give different digits there.

For cols < 64 a row keeps its extremum and as many special elements as fit; tests/test_quant_edge_rows_cpu.py asserts the construction
conditions for cols >= 64. bf16 arrays follow the oracle's convention: float32 arrays of bf16-representable values."""
import math
from dataclasses import dataclass

import numpy as np

from oracle import fq_oracle as O
from tests import edge_tokens as E

TIE_EXPONENTS = (0, -10, 9)              # sym rows; bits > 4 replace 9 by 8 (the fake-quant value 2^9 x -128 would leave fp16)
ASYM_EXPONENTS = (0, -6)                 # (255 x 2^e has to fit fp16; at 2^-10 the pair (3e-6, 1.0) would underflow the 16-bit scale)
TIE_SIGS = [(1.0, 1.0), (0.5, 0.5)]      # the clip pairs under which the special elements' digits are prescribed by hand
SIGS = E.SIGS + [(0.5, 0.5)]
DR_SCALES = (1.0009765625, 0.1428, 1.337, 3.1416e-3, 9360.0)     # double-rounding rows: fp16 scales that are no powers of two
UNDERFLOW = "lone subnormal"             # the one label whose fp16 scale underflows to 0 under every clip pair


@dataclass(frozen=True)
class Special:
    kind: str            # "sym" | "zp0" | "span"
    e: int               # the scale under (1, 1) is 2^e
    qmax: int            # of the grid the row was built for (sym: 2^(bits-1) - 1, asymmetric: 2^bits - 1)
    cols: np.ndarray     # where the special elements sit
    u: np.ndarray        # their quotients under (1, 1), before the nudge: exact multiples of 1/4
    nbr: np.ndarray      # -1 / 0 / +1: the 16-bit neighbour below, the value itself, the neighbour above


def _round(a, lowp):
    return E._round(a, lowp)


def _gauss(cols, tag, rows=1):
    return np.random.default_rng([cols, tag]).standard_normal((rows, cols)).astype(np.float32)


def _neighbour(v, lowp, up):
    """the next 16-bit value above / below v (v: float32 array of representable non-zero values)"""
    if lowp == "bf16":
        b = O.bf16_bits(v).astype(np.int32)
        step = np.where((v > 0) == up, 1, -1)
        return O.bf16_from_bits((b + step).astype(np.uint16))
    h = v.astype(np.float16)
    return np.nextafter(h, np.float16(np.inf if up else -np.inf)).astype(np.float32)


def hand_digit(u, nbr, sigma, lo, hi):
    """BY HAND: the digit of an element whose quotient under (1, 1) is u (nudged by nbr), under the clip pair (sigma, sigma) with sigma a
    power of two: t = u / sigma exactly; a nudged integer keeps its integer, a nudged tie leaves the tie on the side of the nudge, an exact
    tie goes to the even neighbour; then the clamp to [lo, hi]."""
    t = u / sigma
    f = math.floor(t)
    frac = t - f
    if frac == 0.5:
        r = (f if f % 2 == 0 else f + 1) if nbr == 0 else (f + 1 if nbr > 0 else f)
    elif frac == 0.0:
        r = f
    else:
        r = f if frac < 0.5 else f + 1
    return int(min(max(r, lo), hi))


def _positions(cols, n):
    """n distinct columns from 0 to cols - 1, the last one cols - 1 (the last lane's last chunk); cols < n: the first cols - 1 and the last"""
    if cols >= n:
        return np.array([(i * (cols - 1)) // max(n - 1, 1) for i in range(n)])
    return np.arange(cols)


def _special_row(cols, lowp, kind, e, qmax, tag):
    h = (qmax + 1) // 2
    if kind == "sym":
        ks = range(-qmax, qmax) if qmax <= 7 else [-3, -2, -1, 0, 1, 2, -qmax, -qmax + 1, qmax - 2, qmax - 1]
        us = [k + 0.5 for k in ks] + [s * (qmax + d) / 2 for s in (1, -1) for d in (0.5, 1.5)]
        bound, ext = qmax, [float(qmax)]
    elif kind == "zp0":
        ks = range(0, qmax) if qmax <= 15 else [0, 1, 2, qmax - 3, qmax - 2, qmax - 1]
        us, bound, ext = [k + 0.5 for k in ks], qmax, [float(qmax)]
    else:
        ks = range(-h, h - 1) if qmax <= 15 else [-h, -h + 1, -2, -1, 0, 1, h - 3, h - 2]
        us, bound, ext = [k + 0.5 for k in ks], h - 1, [float(-h), float(h - 1)]
    s = np.float32(2.0 ** e)
    spec = [(u, nb) for u in us for nb in (-1, 0, 1)]
    u = np.array([p[0] for p in spec], np.float32)
    nbr = np.array([p[1] for p in spec])
    base = u * s
    ok = _round(base, lowp).astype(np.float32) == base              # (bf16 cannot hold every k + 0.5 of the 8-bit grids)
    val = np.where(nbr == 0, base, np.where(nbr > 0, _neighbour(np.where(ok, base, s), lowp, True), _neighbour(np.where(ok, base, s), lowp, False)))
    ok &= np.abs(val / s - u) < 0.125                                # a nudge that stays a nudge (coarse formats at the large grids)
    ok &= np.abs(val) <= bound * s if kind != "span" else (val >= -h * s) & (val <= (h - 1) * s)
    u, nbr, val = u[ok], nbr[ok], val[ok]
    # the extremes last (span: the minimum first): exact elements, digits by hand like the others
    if kind == "span":
        u, nbr, val = np.r_[ext[0], u, ext[1]], np.r_[0, nbr, 0], np.r_[ext[0] * s, val, ext[1] * s]
    else:
        u, nbr, val = np.r_[u, ext[0]], np.r_[nbr, 0], np.r_[val, ext[0] * s]
    if cols < len(u):                                                # keep the extremes and what fits
        keep = np.r_[np.arange(cols - 1), len(u) - 1]
        u, nbr, val = u[keep], nbr[keep], val[keep]
    fill = np.clip(_gauss(cols, tag)[0], -1, 1) * np.float32(0.4 * max(bound, 1)) * s
    row = np.abs(fill) if kind == "zp0" else fill
    pos = _positions(cols, len(u))
    row[pos] = val
    return row, Special(kind, e, qmax, pos, u.astype(np.float64), nbr)


_dr_cache = {}


def double_rounding_elements(scale):
    """(s, m, xs): s = fp16(scale); m an fp16 extremum with fp16(m / 7) == s; xs every fp16 x in (0, m) whose fp16 quotient RN16(x / s) is
    an exact k + 0.5 (k = 0 .. 6) while x / s is not — found by enumerating all finite fp16 values"""
    if scale not in _dr_cache:
        s = np.float16(scale)
        allh = np.arange(1, 0x7C00, dtype=np.uint16).view(np.float16)          # every positive finite fp16
        with np.errstate(over="ignore"):
            cand = allh[(allh.astype(np.float32) / np.float32(7)).astype(np.float16) == s]
        assert len(cand), scale
        m = cand[-1]                                                       # (the largest: the most elements below it)
        x = allh[allh < m].astype(np.float32)
        t32 = x / np.float32(s)
        t16 = t32.astype(np.float16).astype(np.float32)
        # (x / s exact in fp32 <=> it is the true quotient; a true tie would show as t32 == t16)
        hit = (t16 < 7) & (t16 - np.floor(t16) == 0.5) & (t32 != t16)
        _dr_cache[scale] = (s, m, x[hit].astype(np.float16))
    return _dr_cache[scale]


def _dr_row(cols, scale, tag):
    s, m, xs = double_rounding_elements(scale)
    val = np.r_[xs, -xs, m].astype(np.float32)
    if cols < len(val):
        val = np.r_[val[:cols - 1], val[-1]]
    row = np.clip(_gauss(cols, tag)[0], -1, 1) * np.float32(2.8) * np.float32(s)
    row[_positions(cols, len(val))] = val
    return row


def edge_rows(cols, lowp="f16", bits=4):
    """-> (rows [n, cols] in the 16-bit dtype, labels [n], specials {row index: Special})"""
    rows, labels, specials = [], [], {}

    def add(label, row, special=None):
        if special is not None:
            specials[len(rows)] = special
        rows.append(np.asarray(row, np.float32))
        labels.append(label)

    z = lambda: np.zeros(cols, np.float32)
    add("all zero", z())
    add("all positive", np.abs(_gauss(cols, 1)[0]) + np.float32(2.0 ** -10))
    add("all negative", -np.abs(_gauss(cols, 2)[0]) - np.float32(2.0 ** -10))
    r = z(); r[0] = 1.0
    add("one-hot +1 first", r)
    r = z(); r[cols - 1] = -3.0
    add("one-hot -3 last", r)
    r = _gauss(cols, 5)[0]; r[min(5, cols - 1)] = 15000.0
    add("outlier 15000", r)
    add("gaussians x 1e-3", _gauss(cols, 6)[0] * np.float32(1e-3))
    r = z(); r[cols // 2] = 6e-8 if lowp == "f16" else 2.0 ** -120
    add(UNDERFLOW if lowp == "f16" else "lone 2^-120", r)
    add("constant 7", z() + 7)
    r = z() - 8; r[min(3, cols - 1)] = 7.0
    add("constant -8, one +7", r)
    r = _gauss(cols, 10)[0]; r[0] = 65504.0; r[cols - 1] = -65504.0
    add("+-65504", r)
    qs, qa = 2 ** (bits - 1) - 1, 2 ** bits - 1
    for e in TIE_EXPONENTS:
        e = 8 if (e == 9 and bits > 4) else e
        add(f"ties e={e}", *_special_row(cols, lowp, "sym", e, qs, 20 + e))
    if lowp == "f16" and bits == 4:
        for i, sc in enumerate(DR_SCALES):
            add(f"double rounding s={sc}", _dr_row(cols, sc, 40 + i))
    for e in ASYM_EXPONENTS:
        add(f"asym zero point 0 e={e}", *_special_row(cols, lowp, "zp0", e, qa, 60 + e))
        add(f"asym span e={e}", *_special_row(cols, lowp, "span", e, qa, 80 + e))
    return _round(np.stack(rows), lowp), labels, specials


_batches = {}


def batch(cols, lowp="f16", bits=4):
    """-> (rows [2 n + 1, cols], labels, specials keyed by BATCH row): ordinary rows at the even positions, edge rows at the odd ones.
    Built once per key and read-only."""
    key = (cols, lowp, bits)
    if key not in _batches:
        e, labels, specials = edge_rows(cols, lowp, bits)
        n = len(e)
        b = np.empty((2 * n + 1, cols), e.dtype)
        b[0::2] = _round(_gauss(cols, 100, n + 1), lowp)
        b[1::2] = e
        b.setflags(write=False)
        lab = ["ordinary"] * (2 * n + 1)
        lab[1::2] = labels
        _batches[key] = (b, lab, {2 * i + 1: s for i, s in specials.items()})
    return _batches[key]


def hand_sym_digits(sp, sigma):
    """the special elements' digits of a "sym" row under the clip pair (sigma, sigma), sigma in {1, 0.5}"""
    return np.array([hand_digit(float(u), int(n), sigma, -sp.qmax - 1, sp.qmax) for u, n in zip(sp.u, sp.nbr)])


def hand_asym_values(sp):
    """the special elements' fake-quant VALUES (float64, exact) of a "zp0" / "span" row under (1, 1): scale 2^e, zero point 0 or h, so
    scale (q - zero) = 2^e clamp(round(u), -zero, qmax - zero)"""
    zero = 0 if sp.kind == "zp0" else (sp.qmax + 1) // 2
    d = np.array([hand_digit(float(u), int(n), 1.0, -zero, sp.qmax - zero) for u, n in zip(sp.u, sp.nbr)])
    return d * 2.0 ** sp.e
