"""Edge accumulators and edge scales for every INT4 GEMM epilogue: shared builders (numpy only; no GPU, no torch.cuda).

Every integer GEMM ends in sym_dequant (csrc/fq_gemm_common.hpp: dequant1 / dequant16f): int(q / 10) clamped to +-65176, converted to fp16,
times the two scales, times 10. Random nibbles keep |q| / 10 in the hundreds; `operands` builds nibble matrices whose product is PRESCRIBED:

    columns [0, K - T)   the level: x[m] is -8 on its first A[m] columns and 0 behind them, w[n] is all -8 (+64 per column) or all 7 (-56)
    the last T = 16      the fine offset: x is 1, w[n] holds floor(r[n] / T), plus 1 on the first r[n] mod T columns -> sum r[n]

so q[m, n] = c[n] A[m] + r[n] with c[n] in {64, -56} and r[n] = -128 .. 111: 240 features (signs alternating) times a list of levels is a dense
window of accumulators around every level. Two full-scale token rows (all -8, all 7) follow the level rows; feature 0 (c = 64, r = -128) IS the
all -8 weight row, and `full_scale_w` gives the all -8 / all 7 weight rows on their own for the accumulator-range cases.

`scales` gives the two scale cases (ordinary | the ends of fp16 on a few rows and columns) and `bias` the bias vector of both."""
import numpy as np

from oracle import fq_oracle as O

T = 16                      # columns of the fine offset
N_FEATURES = 240            # r = -128 .. 111
# accumulator levels A (clipped to K - T): around 0; |q| / 10 at 2048, 4096, ... (64 A / 10: A = 320, 640, 1280, 2560, 5120 — the binades of
# half(int) from where integers are no longer exact); the +65176 clamp (64 A = 651760: A = 10183.75) and the -65176 clamp (56 A: A = 11638.6)
BASE_LEVELS = (0, 1, 2, 31, 32, 33, 319, 320, 321, 639, 640, 641, 1279, 1280, 2559, 2560, 5119, 5120, 10183, 10184, 10185, 11638, 11639, 11640)
CLAMP = 65176


def levels(K):
    """the levels of one K: BASE_LEVELS clipped to K - T, then K - T - 1 and K - T (sorted, each once)"""
    top = K - T
    return np.unique(np.array([min(a, top) for a in BASE_LEVELS] + [top - 1, top], dtype=np.int64))


def feature_terms(n=N_FEATURES):
    """-> (c [n], r [n]): feature j adds c[j] per level column (64: weights -8; -56: weights 7, alternating) and r[j] = -128 + j in the last T"""
    assert 1 <= n <= N_FEATURES
    j = np.arange(n, dtype=np.int64)
    return np.where(j % 2 == 0, 64, -56), j - 128


def operands(K, n=N_FEATURES, A=None, full_scale=True):
    """-> (xq int32 [M, K], wq int32 [n, K], q int64 [M, n]): the nibble operands and the product they are built to have. M = len(A) (default:
    levels(K)) plus the two full-scale token rows (all -8, all 7) when `full_scale`."""
    assert K > T and K % 2 == 0
    A = levels(K) if A is None else np.asarray(A, dtype=np.int64)
    assert A.min() >= 0 and A.max() <= K - T
    c, r = feature_terms(n)
    col = np.arange(K - T)
    xq = np.zeros((len(A), K), dtype=np.int32)
    xq[:, :K - T] = np.where(col[None, :] < A[:, None], -8, 0)
    xq[:, K - T:] = 1
    wq = np.empty((n, K), dtype=np.int32)
    wq[:, :K - T] = np.where(c == 64, -8, 7)[:, None]
    wq[:, K - T:] = (r // T)[:, None] + (np.arange(T)[None, :] < (r % T)[:, None])
    q = c[None, :] * A[:, None] + r[None, :]
    if full_scale:
        lvl, fine = wq[:, :K - T].sum(axis=1, dtype=np.int64), wq[:, K - T:].sum(axis=1, dtype=np.int64)
        xq = np.concatenate([xq, np.full((1, K), -8, dtype=np.int32), np.full((1, K), 7, dtype=np.int32)])
        q = np.concatenate([q, (-8 * (lvl + fine))[None, :], (7 * (lvl + fine))[None, :]])
    return xq, wq, q


def repeat_rows(xq, q, M):
    """the token rows repeated (cyclically) up to M rows: the shapes that select a kernel by its row count"""
    idx = np.arange(M) % xq.shape[0]
    return xq[idx], q[idx]


def decode_levels(K=4096):
    """the fused 64 x 64 decode launch quantises its own tokens: rows of -c on the first A columns and +c behind them become digits -7 / +7.
    Against the weights above q = 7 (c[n] / -8) (2 A - (K - T)) + 7 r[n] (A <= K - T): 16 levels — the ends (|q| / 10 = 22848), the quarters,
    |q| / 10 near 3000 and 5600 (the binades from 2048 and 4096), the middle (A = 2040: q = 7 r, through 0) and the all-negative row A = K."""
    h = (K - T) // 2
    return np.array([0, 1, h // 2, h // 2 + 1, h - 500, h - 268, h - 1, h, h + 1, h + 268, h + 500, h + h // 2, K - T - 1, K - T, K - T + 1, K],
                    dtype=np.int64)


# the largest K of each accumulator: the int8 path carries 256 x the product — 64 K 256 < 2^31 needs K < 131072; the general-shape
# kernel adds unscaled products — 64 K < 2^31; the FP6 path's fp32 accumulator holds integers up to 2^24 = 64 * 2^18
INT8_K_LIMIT = 131072                  # the first K the weight-streaming launches refuse and the tile launcher hands to the general-shape kernel
GENERAL_K_CAP = (1 << 25) - 32         # the largest K fq_int4_gemm_i32 / fq_int4_linear_f16 accept
FP6_K_CAP = 1 << 18                    # the largest K of the FP6 path


def full_scale_w(n, K):
    """n weight rows, all -8 (even rows) / all 7 (odd rows)"""
    return np.where(np.arange(n)[:, None] % 2 == 0, -8, 7).astype(np.int32) * np.ones((1, K), dtype=np.int32)


# ---- scales and biases ----------------------------------------------------------------------------------------------------------------
SCALE_CASES = ("ordinary", "ends")
X_ENDS = (0.0, 6e-8, 1.0, 65504.0, -0.5, np.inf)                       # 6e-8: the smallest subnormal
W_ENDS = (0.0, 6e-8, 6.1e-5, 1.0, 65504.0, -1.0, np.inf, np.nan)       # 6.1e-5: the smallest normal number


# where they go. Rows: the subnormal and the 1 on the two lowest levels (row 0: q = r, row 1: q = c + r — |q| / 10 <= 18, so their products with
# the column ends stay SUBNORMAL instead of leaving the format), the Inf on a high row (few |q| < 10 there: Inf * 0 is NaN). Columns: 1 + 30 i.
X_END_ROWS = (3, 0, 1, 5, 7, 9)
W_END_COLS = tuple(1 + 30 * i for i in range(len(W_ENDS)))


def scales(case, M, N, seed=0):
    """-> (x_scale fp16 [M], w_scale fp16 [N]). "ordinary": the suite's random scales (0.001 .. 0.051 / 0.0005 .. 0.0205); "ends": the same with
    X_ENDS on rows X_END_ROWS and W_ENDS on columns W_END_COLS (those that exist: a batch of fewer rows or columns gets the first ones)."""
    assert case in SCALE_CASES
    rng = np.random.default_rng(1000 + seed)
    sx = (rng.random(M) * 0.05 + 0.001).astype(np.float16)
    sw = (rng.random(N) * 0.02 + 0.0005).astype(np.float16)
    if case == "ends":
        with np.errstate(over="ignore"):
            for v, i in zip(X_ENDS, X_END_ROWS):
                if i < M:
                    sx[i] = np.float16(v)
            for v, j in zip(W_ENDS, W_END_COLS):
                if j < N:
                    sw[j] = np.float16(v)
    return sx, sw


def bias(N, seed=0):
    """random N(0, 1) with one +65504, one -65504 and one Inf (N >= 8; else plain random)"""
    rng = np.random.default_rng(2000 + seed)
    b = rng.standard_normal(N).astype(np.float16)
    if N >= 8:
        b[2], b[5], b[7] = 65504.0, -65504.0, np.inf
    return b


# ---- what the oracle does with an accumulator (the branches the CPU file counts) --------------------------------------------------------
def classify(q):
    """per accumulator: the branch of sym_dequant's integer part it takes — dict of boolean arrays"""
    q = np.asarray(q, dtype=np.int64)
    iv = np.where(q >= 0, q // 10, -((-q) // 10))                      # int(q / 10.0f) for |q| <= 2^24 (tests/test_dequant_identity.py)
    ivc = np.clip(iv, -CLAMP, CLAMP)
    with np.errstate(over="ignore"):
        h = ivc.astype(np.float32).astype(np.float16)
        unclamped = iv.astype(np.float32).astype(np.float16)
    inexact = h.astype(np.int64) != ivc
    # a tie of half(int): iv exactly between two neighbouring fp16 values (spacing 2^(e-10) in [2^e, 2^(e+1)): iv odd multiple of half of it)
    a = np.abs(ivc)
    e = np.floor(np.log2(np.maximum(a, 1))).astype(np.int64)
    half_ulp = np.where(e >= 11, 1 << np.maximum(e - 11, 0), 0)
    tie = (e >= 11) & (a % np.maximum(half_ulp, 1) == 0) & ((a // np.maximum(half_ulp, 1)) % 2 == 1)
    return {
        "clamped_high": iv > CLAMP, "clamped_low": iv < -CLAMP, "on_bound": np.abs(iv) == CLAMP,
        "inexact": inexact, "tie": tie, "binade": np.where(a >= 2048, e, -1),
        "inf_without_clamp": np.isinf(unclamped), "minus9_to_minus1": (q >= -9) & (q <= -1), "iv": iv,
    }


def const_product(xv, wv, K, slice_k=1 << 16):
    """O.int4_matmul of a constant row (every nibble xv) against a constant row (every nibble wv) of K columns, as a Python int: the oracle on one
    slice of up to 2^16 columns, times the number of slices (the rows are constant, the product is a sum over slices) — K up to 2^25 without
    gigabytes of unpacked nibbles."""
    total, done = 0, 0
    cache = {}
    while done < K:
        k = min(slice_k, K - done)
        if k not in cache:
            cache[k] = int(O.int4_matmul(O.pack_i4(np.full((1, k), xv, dtype=np.int32)), O.pack_i4(np.full((1, k), wv, dtype=np.int32)))[0, 0])
        total += cache[k]
        done += k
    return total


# ops.sym_dequant on its own: the int32 values of the issue's list
def dequant_values():
    v = [0, 9, 10, 11] + list(range(20479, 20492)) + [651759, 651760, 651769, 651770, (1 << 24) - 1, 1 << 24, (1 << 24) + 1]
    v = sorted(set(v + [-a for a in v]))
    return np.array(v + [np.iinfo(np.int32).max, np.iinfo(np.int32).min], dtype=np.int64).astype(np.int32)


def dequant_grid(rows=16, reps=4):
    """-> int32 [rows, reps * len(dequant_values())]: element (i, j) is value (i + j) mod n, so every value meets every row scale and, over the
    rows, every column scale of a run of `rows` columns"""
    v = dequant_values()
    i, j = np.arange(rows)[:, None], np.arange(reps * len(v))[None, :]
    return v[(i + j) % len(v)]
