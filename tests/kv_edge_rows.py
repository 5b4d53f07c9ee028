"""Edge rows for every KV-cache quantiser (fq_kv_quant_f16, fq_kv_quant_append_i4, the prologue of fq_kv_decode_append[_rope]_i4): shared
builders (numpy + the oracle; no GPU, no torch.cuda). The counterpart of tests/edge_tokens.py for the asymmetric INT4 quantiser of
csrc/fq_kv_common.hpp (kv_params / kv_q8), whose reference is oracle.fq_oracle.kv_asym_quant.

`edge_rows` are hand-built rows that reach every branch of that quantiser, `batch` puts each between two ordinary rows, `extrema_rows` put the
maximum and the minimum into every pair of (32-column quarter, 16-column half) — the pieces the kernels reduce separately —, `exact_trans` is a
signed permutation over {+-1, +-2} (x @ T is one product per element: exact whatever the summation order, so the oracle pins the transformed
path bit for bit), `sweep` walks EVERY fp16 value between two extrema at a fixed (scale, zero). `preclip` restates the oracle's arithmetic up
to the value it clips (tests/test_kv_edge_rows_cpu.py asserts that clipping it gives the oracle's digits): a digit is UNPINNED where that value
is NaN (0 / 0, Inf / Inf — no reference output defines those), and `routes` names the branches a row takes."""
import numpy as np

from oracle import fq_oracle as O

F16, F32 = np.float16, np.float32
UNIT = 2.0 ** -24                                   # the smallest fp16 subnormal
TINY_UNITS = (171, 172, 186, 187, 202, 217)         # ranges (in UNITs, just above the 1e-5 floor = 168 UNITs) whose maximum's quotient rints to 16
# lac clip pairs (clip_max, clip_min): no clip, the clamp binds on both sides, the deployed sigmoid(4) pair (edge_tokens.SIGS[1]), and a clip so
# small that quotients pass +-512 (beyond the exact range of the kernel's magic-number rint)
CLIPS = [(1.0, 1.0), (0.9, 0.8), (0.9820137619972229, 0.9820137619972229), (0.02, 0.5)]
APPEND_CLIP = (0.9, 0.8, 0.95, 0.85)                # (K max, K min, V max, V min) of the paged append under lac
EDGE_NAMES = ["zero", "positive", "negative", "onehot_first", "onehot_last", "outlier_15000", "gauss_1e-3", "gauss_1e-6", "lone_subnormal",
              "const_7", "const_-8_one_7", "ties"] + [f"tiny_{k}" for k in TINY_UNITS] + ["tiny_-172", "const_1000_one_ulp", "one_plus_3e-5",
              "top_65504", "overflow_40000", "gauss"]
N_EDGE = len(EDGE_NAMES)                            # 24
N_BATCH = 2 * N_EDGE + 1
ROW = {n: i for i, n in enumerate(EDGE_NAMES)}      # edge row index by name; its place in batch() is 2 i + 1
COL_BIG, COL_P4, COL_M4 = 7, 3, -4                  # columns of the 65504 and of the +-40000


def tiny_col(i, hd):
    """column of the one non-zero value of tiny row i: quarter i % (hd / 32), half (i + i // 4) % 2, a different place in the half each time"""
    return (i % (hd // 32)) * 32 + ((i + i // 4) % 2) * 16 + (3 * i + 1) % 16


def _gauss(hd, tag, rows=1):
    return np.random.default_rng([hd, tag, 4]).standard_normal((rows, hd)).astype(F32)


def edge_rows(hd):
    e = np.zeros((N_EDGE, hd), F32)
    e[ROW["positive"]] = np.abs(_gauss(hd, 1)[0]) + 0.25
    e[ROW["negative"]] = -np.abs(_gauss(hd, 2)[0]) - 0.25
    e[ROW["onehot_first"], 0] = 1.0
    e[ROW["onehot_last"], hd - 1] = -3.0
    e[ROW["outlier_15000"]] = _gauss(hd, 5)[0]
    e[ROW["outlier_15000"], 5] = 15000.0
    e[ROW["gauss_1e-3"]] = _gauss(hd, 6)[0] * 1e-3           # fp16 subnormals among them
    e[ROW["gauss_1e-6"]] = _gauss(hd, 7)[0] * 1e-6           # range under the 1e-5 floor
    e[ROW["lone_subnormal"], hd // 2] = UNIT
    e[ROW["const_7"]] = 7.0
    e[ROW["const_-8_one_7"]] = -8.0
    e[ROW["const_-8_one_7"], 3] = 7.0
    t = e[ROW["ties"]]                                       # minimum 0, maximum 15: scale 1, zero 0; k + .5 and its two neighbours 2^-6 away
    t[1] = 15.0
    t[2:17] = np.arange(15) + 0.5
    t[17:32] = np.arange(15) + 0.5 + 2.0 ** -6
    t[32:47] = np.arange(15) + 0.5 - 2.0 ** -6
    for i, k in enumerate(TINY_UNITS):
        e[ROW[f"tiny_{k}"], tiny_col(i, hd)] = k * UNIT
    e[ROW["tiny_-172"]] = -172 * UNIT                        # the same range below zero: zero = 172 units, not 0
    e[ROW["tiny_-172"], hd // 2 + 9] = 0.0
    e[ROW["const_1000_one_ulp"]] = 1000.0
    e[ROW["const_1000_one_ulp"], hd - 2] = 1000.5
    e[ROW["one_plus_3e-5"]] = 1.0 + _gauss(hd, 21)[0] * 3e-5
    e[ROW["top_65504"]] = np.abs(_gauss(hd, 22)[0]) * 100.0
    e[ROW["top_65504"], COL_BIG] = 65504.0                   # the range stays finite at the top of the format
    e[ROW["overflow_40000"]] = _gauss(hd, 23)[0]
    e[ROW["overflow_40000"], COL_P4] = 40000.0               # the range overflows: scale = Inf
    e[ROW["overflow_40000"], hd + COL_M4] = -40000.0
    e[ROW["gauss"]] = _gauss(hd, 24)[0]
    return e.astype(F16)


def batch(hd):
    """2 N_EDGE + 1 rows: ordinary Gaussian rows at the even positions, the edge rows at the odd ones"""
    b = np.empty((N_BATCH, hd), F16)
    b[0::2] = _gauss(hd, 100, N_EDGE + 1).astype(F16)
    b[1::2] = edge_rows(hd)
    return b


def extrema_rows(hd):
    """one row per ((quarter, half) of the maximum, (quarter, half) of the minimum): (hd / 16)^2 rows of small Gaussian values with a +3 and a -5"""
    n = hd // 16
    r = (_gauss(hd, 200, n * n) * 0.01).astype(F32)
    for a in range(n):
        for b in range(n):
            i = a * n + b
            ca = a * 16 + (5 * i) % 16
            cb = b * 16 + (5 * i + 7) % 16
            r[i, ca], r[i, cb] = 3.0, -5.0
    return r.astype(F16)


def exact_trans(hd):
    """seeded signed permutation T with entries in {+-1, +-2}: (x @ T)[:, perm[i]] = x[:, i] * T[i, perm[i]], one product per element. The input
    columns that hold the 65504 and the +-40000 pass with +1 (doubled or negated they would turn two more rows into Inf-range rows), the tiny
    rows' columns with +-1 (their ranges stay the ranges that rint to 16)."""
    rng = np.random.default_rng([hd, 9])
    T = np.zeros((hd, hd), F32)
    perm = rng.permutation(hd)
    val = rng.choice(np.array([1, 2], F32), hd) * rng.choice(np.array([-1, 1], F32), hd)
    for i in range(len(TINY_UNITS)):
        val[tiny_col(i, hd)] = np.sign(val[tiny_col(i, hd)])
    for c in (COL_BIG, COL_P4, hd + COL_M4):
        val[c] = 1.0
    T[np.arange(hd), perm] = val
    return T.astype(F16)


def exact_product(x16, T16):
    """x @ T for a signed permutation T, element by element (no sum): what O.kv_transform and every kernel must return, bit for bit"""
    T = np.asarray(T16, F32)
    src = np.argmax(T != 0, axis=0)                          # the input column of output column j
    with np.errstate(over="ignore"):
        y = (np.asarray(x16, F16).astype(F32)[:, src] * T[src, np.arange(T.shape[0])]).astype(F16)
    return y + F16(0)                                        # a sum that has a +0 term is never -0


def _bits_between(lo, hi):
    """every fp16 value v with lo <= v <= hi, ascending (one zero)"""
    lo, hi = F16(lo), F16(hi)
    allv = np.arange(0x10000, dtype=np.uint32).astype(np.uint16).view(F16)
    keep = np.isfinite(allv) & (allv >= lo) & (allv <= hi) & (np.arange(0x10000) != 0x8000)
    return np.sort(allv[keep])


def sweep(lo, hi, hd=128):
    """rows whose first two columns are lo and hi and whose other hd - 2 columns walk every fp16 value in [lo, hi] (the last row padded with lo):
    every row has the extrema (lo, hi), so every representable x meets the quantiser at that one (scale, zero)"""
    v = _bits_between(lo, hi)
    per = hd - 2
    rows = (len(v) + per - 1) // per
    out = np.full((rows, hd), F16(lo), F16)
    out[:, 1] = F16(hi)
    body = np.full(rows * per, F16(lo), F16)
    body[:len(v)] = v
    out[:, 2:] = body.reshape(rows, per)
    return out


# (lo, hi) of the sweeps, by the case each is there for
SWEEPS = {
    "scale_1": [(0.0, 15.0), (-8.0, 7.0)],                                        # x + zero exact / rounding (x + 8 above 8 loses bits)
    "scale_not_pow2": [(-1.3, 2.9), (-0.37, 0.11), (0.5, 4.0)],                   # negative lo: x + zero rounds
    "scale_subnormal": [(0.0, 5e-4), (-3e-4, 4e-4), (0.0, 15 * 2.0 ** -14)],      # fp16(d / 15) below 2^-14 (the last: exactly 2^-14)
    "floor": [(0.0, 100 * UNIT), (-50 * UNIT, 60 * UNIT), (0.0, 168 * UNIT)],     # d <= fp16(1e-5) = 168 units
    "tiny": [(0.0, k * UNIT) for k in range(169, 233)] + [(-172 * UNIT, 0.0)],    # every range in units just above the floor
    "largest": [(-32752.0, 32752.0), (0.0, 65504.0)],                             # d = 65504
    "offset_1000": [(1000.0, 1002.5), (-1002.0, -1000.0)],                        # a few ulps (0.5) at a large offset
}
ALL_SWEEPS = [p for fam in SWEEPS.values() for p in fam]
_sweeps = {}


def sweep_rows(hd=128):
    """all sweeps stacked (computed once, never modified): -> rows [n, hd] fp16"""
    if hd not in _sweeps:
        s = np.concatenate([sweep(lo, hi, hd) for lo, hi in ALL_SWEEPS])
        s.setflags(write=False)
        _sweeps[hd] = s
    return _sweeps[hd]


def preclip(x16, clip=(1.0, 1.0), lac=False):
    """oracle.fq_oracle.kv_asym_quant up to the value it clips to [0, 15], every step rounded to fp16 as there -> dict: `pre` (fp16 [rows, hd], the
    digit is clip(pre, 0, 15); without lac pre = rint(quot)), `quot` (the fp16 quotient before rint: (x + zero) / scale, with lac x / scale),
    `scale`, `zero` (fp16 [rows, 1]), `d` (the fp16 range before the 1e-5 floor; with lac after the clip and the substitution),
    `subst` (lac: the all-zero row got (-1, 1))"""
    x = np.asarray(x16, F16)
    xmax, xmin = x.max(axis=-1, keepdims=True), x.min(axis=-1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if lac:
            xmax, xmin = np.maximum(xmax, F16(0)), np.minimum(xmin, F16(0))
            xmax = (xmax.astype(F32) * F32(F16(clip[0]))).astype(F16)
            xmin = (xmin.astype(F32) * F32(F16(clip[1]))).astype(F16)
            subst = (xmin == 0) & (xmax == 0)
            xmin, xmax = np.where(subst, F16(-1), xmin), np.where(subst, F16(1), xmax)
            d = (xmax.astype(F32) - xmin.astype(F32)).astype(F16)
            scale = (d.astype(F32) / F32(15)).astype(F16)
            nx = (F32(-1.0) * xmin.astype(F32)).astype(F16)
            zero = np.rint((nx.astype(F32) / scale.astype(F32)).astype(F16)).astype(F16)
            quot = (x.astype(F32) / scale.astype(F32)).astype(F16)
            pre = (np.rint(quot).astype(F16).astype(F32) + zero.astype(F32)).astype(F16)
        else:
            subst = np.zeros(xmax.shape, bool)
            d = (xmax.astype(F32) - xmin.astype(F32)).astype(F16)
            scale = (np.maximum(d, F16(1e-5)).astype(F32) / F32(15)).astype(F16)
            zero = (-xmin).astype(F16)
            t = (x.astype(F32) + zero.astype(F32)).astype(F16)
            quot = (t.astype(F32) / scale.astype(F32)).astype(F16)
            pre = np.rint(quot).astype(F16)
    return {"pre": pre, "quot": quot, "scale": scale, "zero": zero, "d": d, "subst": subst}


def unpinned(x16, clip=(1.0, 1.0), lac=False):
    """bool [rows, hd]: the digits no reference output defines (the oracle's value before the clip is NaN)"""
    return np.isnan(preclip(x16, clip, lac)["pre"])


def routes(x16, clip=(1.0, 1.0), lac=False):
    """per row, the set of quantiser branches it reaches (names: see tests/test_kv_edge_rows_cpu.py)"""
    p = preclip(x16, clip, lac)
    quot, pre = p["quot"].astype(np.float64), p["pre"].astype(np.float64)
    out = []
    with np.errstate(invalid="ignore"):
        frac_half = np.isfinite(quot) & (quot - np.floor(quot) == 0.5)
        for i in range(quot.shape[0]):
            r = set()
            if not lac and p["d"][i, 0] < F16(1e-5):
                r.add("floor")
            if not lac and (pre[i] == 16).any():
                r.add("rint16")
            if lac and (pre[i] > 15).any():
                r.add("clamp_above")
            if lac and (pre[i] < 0).any():
                r.add("clamp_below")
            if (frac_half[i] & (np.floor(quot[i]) % 2 == 0)).any():
                r.add("tie_even")                            # k + .5 with k even: rounds DOWN to k
            if (frac_half[i] & (np.floor(quot[i]) % 2 == 1)).any():
                r.add("tie_odd")                             # k + .5 with k odd: rounds UP to k + 1
            if (np.isfinite(quot[i]) & (np.abs(quot[i]) > 512)).any():
                r.add("beyond_512")
            if p["subst"][i, 0]:
                r.add("subst")
            if np.isinf(p["scale"][i, 0]):
                r.add("inf_scale")
            if p["scale"][i, 0] == 0:
                r.add("zero_scale")
            s = p["scale"][i, 0]
            if 0 < s < F16(2.0 ** -14):
                r.add("subnormal_scale")
            out.append(r)
    return out


_refs = {}


def reference(hd, trans, clip, lac, which="batch"):
    """the oracle's outputs for batch(hd) / extrema_rows(hd) / sweep_rows(hd) (through exact_trans when `trans`), computed once per case and never
    modified -> dict x (what the kernel is given), y (what it quantises), packed, scale, zero (fp16 [rows]), mask (unpinned digits), deq"""
    key = (hd, bool(trans), tuple(clip), bool(lac), which)
    if key not in _refs:
        x = {"batch": batch, "extrema": extrema_rows, "sweep": sweep_rows}[which](hd)
        y = O.kv_transform(x, exact_trans(hd)) if trans else x
        packed, scale, zero, q8 = O.kv_asym_quant(y, clip[0], clip[1], lac)
        r = {"x": x, "y": y, "packed": packed, "scale": scale[:, 0], "zero": zero[:, 0], "q": q8, "mask": unpinned(y, clip, lac),
             "deq": O.kv_asym_dequant(packed, scale, zero, lac)}
        for v in r.values():
            v.setflags(write=False)
        _refs[key] = r
    return _refs[key]
