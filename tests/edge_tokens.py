"""Edge tokens for every fused transform + INT4 family: shared builders (numpy only; no GPU, no torch.cuda).

`edge_rows` are the twelve tokens of tests/golden/edge_64x64.npz's kind at ANY factor pair, `batch` puts each of them between two ordinary
rows, `exact_factors` are signed permutations with entries in {-1, -2}: every element of L^T.X.R is then ONE product x * r * l with
r l in {1, 2, 4} — exact in fp16 / bf16 / fp32 whatever order a kernel adds the (zero) other terms in, so every output of every family is
pinned bit for bit by the oracle. (No 1/2 among the entries: it would push the subnormals of rows 6 and 8 below the format.)

bf16 arrays follow the oracle's convention: float32 arrays of bf16-representable values."""
import numpy as np

from oracle import fq_oracle as O

# the clip pairs: (1, 1) and the deployed sigmoid(4) pair (magic-number rounding, no clamp), (0.9, 0.33) / (0.5, 0.6) (the clamp binds),
# (0.94, 0.93) (quotients up to 7 / 0.93 = 7.53, rounded without the clamp except where a token exceeds the guards), (0.9346, 0.9346)
# (7 / sigma = 7.4898: just inside fq_needs_clamp's 7.49), (1e-7, 1e-7) / (3e-6, 1.0) (quotients beyond 2^21: true division), (0.33, 0.9)
# (FQ_NO_CLAMP0 on a single-signed row: the scale comes from the smaller extreme, the clamp must bind). SIG_ROUTES is what the CPU file
# asserts of each.
SIGS = [(1.0, 1.0), (0.9820137619972229, 0.9820137619972229), (0.9, 0.33), (0.5, 0.6), (0.94, 0.93), (0.9346, 0.9346), (1e-7, 1e-7),
        (3e-6, 1.0), (0.33, 0.9)]
# what each entry is in the list for: the routes (see routes()) at least one row of the batch must take under it
SIG_ROUTES = [{"plain"}, {"plain"}, {"plain", "clamp"}, {"clamp"}, {"plain"}, {"plain"}, {"div"}, {"plain", "clamp", "div"}, {"clamp"}]
# the factor pairs, by the kernel family their packed-only fp16 launch runs (packed_family() below; the GPU tests hold the labels to it)
PAIRS = {
    "k64": [(64, 64)],
    "wave": [(32, 64), (56, 64), (64, 112), (64, 128)],
    "trio": [(112, 128), (128, 128)],
    "duo": [(112, 224), (128, 224)],
    # (N = 64, 64 < M <= 192 — the pairs fq_kron_tall.hip was written for — run the tiles kernel's N = 64 instantiations since round 5)
    "tiles": [(80, 112), (86, 128), (128, 144), (128, 148), (144, 192), (80, 64), (140, 64), (172, 64)],
    "general": [(2, 2), (3, 6), (60, 62), (130, 16), (40, 100), (129, 254)],
}
ALL_PAIRS = [mn for fam in PAIRS.values() for mn in fam]
FAMILY = {mn: fam for fam, pairs in PAIRS.items() for mn in pairs}


def packed_family(M, N):
    """the label a pair is filed under here and in tests/test_gpu_bounds.py, from the kernel fq_debug_kron_route names for its packed-only
    fp16 launch (a host call: no GPU work)"""
    from flatquant_amd import _lib
    kernel = _lib.kron_route(M, N, 0x01).split("<")[0]
    return {"fq_kron64_kernel": "k64", "fq_kron_fast_kernel": "table"}.get(kernel, kernel[len("fq_kron_"):-len("_kernel")])
N_EDGE, N_BATCH = 12, 25
NONFINITE_ROWS = (1, 3, 9)       # rows of the BATCH (edge rows 0, 1 and 4) that nonfinite() replaces


def _round(a, lowp):
    a = np.asarray(a, dtype=np.float32)
    return O.bf16_round(a) if lowp == "bf16" else a.astype(np.float16)


def _gauss(M, N, tag, rows=1):
    return np.random.default_rng([M, N, tag]).standard_normal((rows, M * N)).astype(np.float32)


def edge_rows(M, N, lowp="f16"):
    d = M * N
    e = np.zeros((N_EDGE, d), np.float32)
    e[1] = np.abs(_gauss(M, N, 1)[0])
    e[2] = -np.abs(_gauss(M, N, 2)[0])
    e[3, 0] = 1.0
    e[4, d - 1] = -3.0                       # last row and column of the block: inside the padded tile where M or N is no tile multiple
    e[5, min(5, d - 1)] = 15000.0
    e[6] = _gauss(M, N, 6)[0] * 1e-3         # fp16 subnormals among them
    ties = [7, .5, 1.5, 2.5, -.5, -1.5, 3.5, -3.5]
    e[7, :min(8, d)] = ties[:d]
    e[8, d // 2] = 6e-8                      # fp16: the smallest subnormal
    e[9] = 7.0
    e[10] = -8.0
    e[10, min(3, d - 1)] = 7.0
    e[11] = _gauss(M, N, 11)[0]
    e[11, :128] = 0.0                        # an all-zero scale group under FQ_GROUP128
    return _round(e, lowp)


def batch(M, N, lowp="f16"):
    """25 rows: 13 ordinary Gaussian rows at the even positions, the edge rows at the odd ones"""
    e = edge_rows(M, N, lowp)
    b = np.empty((N_BATCH, M * N), e.dtype)
    b[0::2] = _round(_gauss(M, N, 100, N_BATCH - N_EDGE), lowp)
    b[1::2] = e
    return b


def _signed_perm(n, rng, sign):
    m = np.zeros((n, n), np.float32)
    m[np.arange(n), rng.permutation(n)] = sign * rng.choice(np.array([1, 2], np.float32), n)
    return m


def exact_factors(M, N, lowp="f16"):
    """seeded signed permutations, both over {-1, -2}: the intermediate X.R has every sign flipped and L^T flips it back, so a single-signed
    token STAYS single-signed through the transform. FQ_NO_CLAMP0 then takes both extremes from the same side of zero, which is where a
    padding lane's 0 would show (the constant-7 row under (3e-6, 1.0): m = its minimum; with a 0 among the extremes, 3e-6 x its maximum)."""
    rng = np.random.default_rng([M, N, 7])
    return _round(_signed_perm(M, rng, -1.0), lowp), _round(_signed_perm(N, rng, -1.0), lowp)


def random_factors(M, N, lowp="f16"):
    """randn / sqrt(n), as the family files use: the transform is no longer exact, the edge rows stay finite"""
    rng = np.random.default_rng([M, N, 8])
    return _round(rng.standard_normal((M, M)) / np.sqrt(M), lowp), _round(rng.standard_normal((N, N)) / np.sqrt(N), lowp)


def nonfinite(b):
    """a copy with row 1 NaN, row 3 holding one +Inf, row 9 constant 65504 (overflows under a random transform)"""
    bad = b.copy()
    bad[1] = np.nan
    bad[3, bad.shape[1] // 3] = np.inf
    bad[9] = 65504.0 if bad.dtype == np.float16 else O.bf16_round(np.float32(65504.0))
    return bad


def routes(y, sig, clamp0=True):
    """the quantiser route of each row of y (fp32 [rows, d]) as the packed-only kernels choose it: fq_magic_ok / fq_needs_clamp of
    csrc/fq_common.hpp restated -> an array of 'div' (true division), 'clamp', 'plain' (magic-number rounding without the clamp)"""
    y = np.asarray(y, np.float32)
    scale = O.token_scale(y, sig[0], sig[1], clamp0)
    inv = (np.float32(1) / scale).astype(np.float32)
    vmax, vmin = y.max(axis=1), y.min(axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        magic = np.maximum(vmax, -vmin) * inv < np.float32(2097152.0)
        clamp = ~((vmax * inv < np.float32(7.49)) & (vmin * inv > np.float32(-8.49)))
    return np.where(~magic, "div", np.where(clamp, "clamp", "plain"))
