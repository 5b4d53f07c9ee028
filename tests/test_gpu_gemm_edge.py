"""Every INT4 GEMM epilogue and accumulator at its edges (builders: tests/gemm_edge.py; their conditions: tests/test_gemm_edge_cpu.py).

The routes — the tile kernel, the general-shape kernel, the weight-streaming kernel with its two-blob, split and multi-problem launches, the
FP6-path tiles with their one-call and multi entries, the fused 64 x 64 decode launch, ops.sym_dequant on its own — all end in the reference's
sym_dequant. The other GEMM files hold them to the oracle on random nibbles and scales of 0.0005 .. 0.05, where |q| / 10 stays in the hundreds.
Here the accumulators are PRESCRIBED: dense windows around 0, around every binade of half(int) from 2048 up, around both clamps, at the K on
either side of the kernels' clamp gate (K <= 10176: dequant16f<false>), under ordinary scales and under scales at the ends of fp16 — and the
accumulators' own range: all -8 x -8 / -8 x 7 at the largest K each launcher accepts.

The bar: the bits of O.linear4bit (O.int4_matmul where a route returns int32). NaN is compared as a class, and the kernel's NaN positions must
be the oracle's (the CPU file caps them at 1 % of the format-end batches and finds none anywhere else)."""
import functools

import numpy as np
import pytest
import torch

from oracle import fq_oracle as O
from tests import gemm_edge as G

pytestmark = pytest.mark.gpu

CASES = G.SCALE_CASES


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def oracle_linear(c, sx, sw, b):
    """O.linear4bit behind its matmul (c = O.int4_matmul(x, w), computed once per K and indexed for repeated rows / features)"""
    with np.errstate(invalid="ignore", over="ignore"):
        y = O.sym_dequant(c, sx, sw)
        if b is not None:
            y = (y.astype(np.float32) + np.asarray(b, dtype=np.float16).reshape(1, -1).astype(np.float32)).astype(np.float16)
    return y


def same_bits(y, ref, what=""):
    y = y.cpu().numpy() if isinstance(y, torch.Tensor) else y
    assert y.shape == ref.shape and y.dtype == ref.dtype == np.float16, (what, y.shape, ref.shape)
    ny, nr = np.isnan(y), np.isnan(ref)
    assert np.array_equal(ny, nr), (what, "NaN positions", np.argwhere(ny != nr)[:8].tolist())
    bad = (y.view(np.uint16) != ref.view(np.uint16)) & ~nr
    if bad.any():
        i = np.argwhere(bad)
        raise AssertionError(f"{what}: {len(i)} of {y.size} outputs differ, first {[(tuple(p), float(y[tuple(p)]), float(ref[tuple(p)])) for p in i[:6].tolist()]}")


def same_ints(c, ref, what=""):
    c = c.cpu().numpy()
    assert c.dtype == np.int32 and c.shape == ref.shape
    bad = c != ref
    if bad.any():
        i = np.argwhere(bad)
        raise AssertionError(f"{what}: {len(i)} of {c.size} accumulators differ, first {[(tuple(p), int(c[tuple(p)]), int(ref[tuple(p)])) for p in i[:6].tolist()]}")


class Batch:
    """the edge operands of one K: `rows` token rows (the level rows + 2 full-scale rows, repeated up to `rows`) x `n` features (the 240,
    cut or repeated), packed, on the host and on the device, with O.int4_matmul of them"""

    def __init__(self, K, rows=None, n=G.N_FEATURES):
        xq, wq, q = base(K)
        ri = np.arange(rows if rows is not None else xq.shape[0]) % xq.shape[0]
        ci = np.arange(n) % wq.shape[0]
        self.K, self.M, self.N = K, len(ri), n
        self.xp, self.wp = O.pack_i4(xq[ri]), O.pack_i4(wq[ci])
        self.c = base_product(K)[np.ix_(ri, ci)]
        assert np.array_equal(self.c, q[np.ix_(ri, ci)].astype(np.int32))
        self.x, self.w = dev(self.xp), dev(self.wp)

    def scales(self, case, seed=0):
        sx, sw = G.scales(case, self.M, self.N, seed)
        return sx, sw, G.bias(self.N, seed)


@functools.lru_cache(maxsize=None)
def base(K):
    return G.operands(K)


@functools.lru_cache(maxsize=None)
def base_product(K):
    xq, wq, _ = base(K)
    return O.int4_matmul(O.pack_i4(xq), O.pack_i4(wq))


@functools.lru_cache(maxsize=None)
def batch(K, rows=None, n=G.N_FEATURES):
    return Batch(K, rows, n)


def check_linear(B, case, run, what, seed=0):
    """run(sx, sw, bias) -> y on the device, with and without bias, against the oracle"""
    sx, sw, b = B.scales(case, seed)
    for bb in (None, b):
        y = run(dev(sx), dev(sw), None if bb is None else dev(bb))
        same_bits(y, oracle_linear(B.c, sx, sw, bb), f"{what} K={B.K} M={B.M} N={B.N} {case} bias={bb is not None}")


def test_the_shared_reference_is_the_oracles_linear4bit():
    B = batch(10240)
    for case in CASES:
        sx, sw, b = B.scales(case)
        with np.errstate(invalid="ignore", over="ignore"):
            for bb in (None, b):
                ref = O.linear4bit(B.xp, sx, B.wp, sw, bb)
                got = oracle_linear(B.c, sx, sw, bb)
                assert np.array_equal(np.isnan(ref), np.isnan(got)) and np.array_equal(ref.view(np.uint16)[~np.isnan(ref)], got.view(np.uint16)[~np.isnan(ref)])


# ---- the int8 matrix path: tile kernel and general-shape kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("K", [128, 10112, 10240, 11776])
def test_tile_kernel(ops, K, case):
    """fq_gemm_i4_kernel: K % 128 == 0 and N % 16 == 0 select it; K = 10112 / 10240 are the two sides of its clamp gate"""
    B = batch(K)
    assert K % 128 == 0 and B.N % 16 == 0 and K < G.INT8_K_LIMIT
    same_ints(ops.int4_matmul(B.x, B.w), B.c, f"int4_matmul K={K}")
    check_linear(B, case, lambda sx, sw, b: ops.int4_linear(B.x, sx, B.w, sw, b), "int4_linear (tile kernel)")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("K,n", [(10208, 240), (11744, 240), (10240, 232)])
def test_general_shape_kernel(ops, K, n, case):
    """fq_gemm_i4_simple_kernel: K % 128 != 0 or N % 16 != 0"""
    B = batch(K, None, n)
    assert K % 128 or n % 16
    same_ints(ops.int4_matmul(B.x, B.w), B.c, f"int4_matmul K={K} N={n}")
    check_linear(B, case, lambda sx, sw, b: ops.int4_linear(B.x, sx, B.w, sw, b), "int4_linear (general-shape kernel)")


# ---- the weight-streaming kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("rows", [None, 47, 97])          # one, two and four token tiles (None: the batch as it is, <= 32 rows)
@pytest.mark.parametrize("K", [10176, 10240, 11776])
def test_weight_streaming_kernel(ops, K, rows, case):
    B = batch(K, rows)
    assert (B.M <= 32) if rows is None else (B.M == rows)
    img = ops.int4_to_frag(B.w)
    same_ints(ops.int4_skinny_matmul(B.x, img, B.N), B.c, f"int4_skinny_matmul K={K} M={B.M}")
    check_linear(B, case, lambda sx, sw, b: ops.int4_skinny_linear(B.x, sx, img, sw, b, B.N, split=False), "int4_skinny_linear (unsplit)")


@pytest.mark.parametrize("case", CASES)
def test_weight_streaming_kernel_two_blobs_in_flight(ops, case):
    """a lone 2048-wide projection of <= 32 rows: the U = 2 instantiation (fq_launch_gemm_i4_skinny: `deep`)"""
    K, N = 11776, 2048
    B = batch(K, None, N)
    assert B.M <= 32 and 64 <= (N + 31) // 32 <= 256 and K // 64 >= 32
    img = ops.int4_to_frag(B.w)
    same_ints(ops.int4_skinny_matmul(B.x, img, N), B.c, "int4_skinny_matmul N=2048")
    check_linear(B, case, lambda sx, sw, b: ops.int4_skinny_linear(B.x, sx, img, sw, b, N, split=False), "int4_skinny_linear (two blobs)")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("K,rows,n", [(10240, None, 240), (11776, 47, 240), (11776, 97, 240), (11776, None, 2048)])
def test_weight_streaming_kernel_split_launch(ops, K, rows, n, case):
    """the K range over 2 - 4 workgroups (int32 partial tiles in a workspace): three launches in a row, the counters return to zero"""
    from flatquant_amd._lib import lib
    B = batch(K, rows, n)
    assert int(lib.fq_int4_skinny_split_workspace_bytes(B.M, B.N, K)) > 0
    img = ops.int4_to_frag(B.w)
    for rep in range(3):
        check_linear(B, case, lambda sx, sw, b: ops.int4_skinny_linear(B.x, sx, img, sw, b, B.N), f"int4_skinny_linear (split, launch {rep})")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("rows", [None, 47])
def test_weight_streaming_kernel_multi_problem_launch(ops, rows, case):
    K = 11776
    B1, B2 = batch(K, rows), batch(K, rows, 232)
    img1, img2 = ops.int4_to_frag(B1.w), ops.int4_to_frag(B2.w)
    (sx1, sw1, b1), (sx2, sw2, b2) = B1.scales(case), B2.scales(case, seed=1)
    for bb1, bb2 in ((None, b2), (b1, None)):
        d = lambda a: None if a is None else dev(a)
        ys = ops.int4_skinny_linear_multi([(B1.x, dev(sx1), img1, dev(sw1), d(bb1)), (B2.x, dev(sx2), img2, dev(sw2), d(bb2))])
        assert len(ys) == 2
        same_bits(ys[0], oracle_linear(B1.c, sx1, sw1, bb1), f"multi problem 0 M={B1.M} {case}")
        same_bits(ys[1], oracle_linear(B2.c, sx2, sw2, bb2), f"multi problem 1 M={B2.M} {case}")


# ---- the FP6 matrix path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("rows", [47, 129])               # 33 .. 128 rows: the 128 x 128 decode tile; 129: 128-token tiles of 256 features
@pytest.mark.parametrize("K", [10112, 10240, 11776])
def test_fp6_path(ops, K, rows, case):
    """bf6_linear on kept blobs, the one-call entry with a kept and with a transient weight image, the multi-problem entry; K = 10112 / 10240
    are the two sides of the kernel's clamp gate. (The 256 x 256 tile needs >= 192 tiles: test_fp6_path_256_tile.)"""
    B = batch(K, rows)
    assert ops.bf6_supported(B.N, K)
    xb, wb = ops.int4_to_bf6(B.x), ops.int4_to_bf6(B.w, weights=True)
    same_ints(ops.bf6_matmul(xb, wb, B.M, B.N, K), B.c, f"bf6_matmul K={K} M={B.M}")
    check_linear(B, case, lambda sx, sw, b: ops.bf6_linear(xb, sx, wb, sw, b, B.M, B.N, K), "bf6_linear")
    check_linear(B, case, lambda sx, sw, b: ops.int4_linear_fp6(B.x, sx, B.w, wb, sw, b), "int4_linear_fp6 (kept image)")
    check_linear(B, case, lambda sx, sw, b: ops.int4_linear_fp6(B.x, sx, B.w, None, sw, b), "int4_linear_fp6 (transient image)")
    B2 = batch(K, rows, 224)
    sx2, sw2, b2 = B2.scales(case, seed=1)

    def multi(sx, sw, b):
        ys = ops.int4_linear_fp6_multi([(B.x, sx, B.w, wb, sw, b), (B2.x, dev(sx2), B2.w, None, dev(sw2), dev(b2))])
        same_bits(ys[1], oracle_linear(B2.c, sx2, sw2, b2), f"int4_linear_fp6_multi problem 1 K={K} M={B.M} {case}")
        return ys[0]
    check_linear(B, case, multi, "int4_linear_fp6_multi problem 0")


@pytest.mark.parametrize("case", CASES)
def test_fp6_path_256_tile(ops, case):
    """the 256 x 256 tile with persistent workgroups is chosen from 3/4 of the CUs' worth of tiles (14 x 14 = 196 here): the edge batch of
    K = 10240 (the clamp variant of the epilogue) repeated along both dimensions — and the int8 tile kernel on the same operands"""
    K, M, N = 10240, 3584, 3584
    B = batch(K)
    ri, ci = np.arange(M) % B.M, np.arange(N) % B.N
    x, w = dev(B.xp[ri]), dev(B.wp[ci])
    sx0, sw0, b0 = B.scales(case)
    sx, sw, b = sx0[ri], sw0[ci], b0[ci]
    for bb0, bb in ((None, None), (b0, b)):
        ref = oracle_linear(B.c, sx0, sw0, bb0)[np.ix_(ri, ci)]          # (row m, column n of the output depend on x[m], w[n] and their scales alone)
        d = None if bb is None else dev(bb)
        same_bits(ops.int4_linear_fp6(x, dev(sx), w, None, dev(sw), d), ref, f"int4_linear_fp6 256 x 256 tiles {case}")
        same_bits(ops.int4_linear(x, dev(sx), w, dev(sw), d), ref, f"int4_linear 256 x 256 tiles {case}")


# ---- the fused 64 x 64 decode launch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_fused_decode_launch(ops, case):
    """fq_kron64_linear_multi_f16 with identity factors on rows of -c | +c: the digits are -7 | +7 under the clip pair (1, 1), |q| / 10 reaches 22848.
    The oracle's input is the packed output of ops.kron_quant on the same x."""
    from flatquant_amd._lib import FQ_OUT_PACKED
    K = 4096
    A = G.decode_levels(K)
    amp = (0.25 * (1 + np.arange(len(A)))).astype(np.float16)
    x = dev(np.where(np.arange(K)[None, :] < A[:, None], -amp[:, None], amp[:, None]).astype(np.float16))
    eye = torch.eye(64, dtype=torch.float16, device="cuda")
    _, wq, _ = G.operands(K, full_scale=False)
    sigs = [(1.0, 1.0), (1.0, 1.0)]
    kq = ops.kron_quant(x, eye, eye, sigs, FQ_OUT_PACKED)
    probs, want = [], []
    for p, n in enumerate((224, 256)):
        wp = O.pack_i4(wq[np.arange(n) % wq.shape[0]])
        sw, b = G.scales(case, len(A), n, seed=p)[1], G.bias(n, seed=p)
        xp, sx = kq.q[p].cpu().numpy(), kq.scale[p].reshape(-1).cpu().numpy()
        digits = O.unpack_i4(xp)
        assert np.array_equal(digits, np.where(np.arange(K)[None, :] < A[:, None], -7, 7))
        c = O.int4_matmul(xp, wp)
        assert np.abs(c).max() // 10 >= 20000
        probs.append((ops.int4_to_frag(dev(wp)), dev(sw), dev(b) if p == 0 else None))
        want.append(oracle_linear(c, sx, sw, b if p == 0 else None))
    got = ops.kron64_linear_multi(x, eye, eye, sigs, probs)
    assert got is not None and len(got) == 2                 # (None: the shape was not covered and the caller would run two launches)
    for p in range(2):
        same_bits(got[p], want[p], f"kron64_linear_multi problem {p} {case}")


# ---- ops.sym_dequant on its own -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_sym_dequant_on_chosen_accumulators(ops, case):
    g = G.dequant_grid()
    sx, sw = G.scales(case, *g.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = O.sym_dequant(g, sx, sw)
    same_bits(ops.sym_dequant(dev(g), dev(sx), dev(sw)), ref, f"sym_dequant {case}")


# ---- the accumulators' range: full-scale operands at the largest K a launcher accepts ----------------------------------------------------------
def const_rows(rows, K, alternate):
    """packed rows of K nibbles on the device: all -8 (0x88), every second one all 7 (0x77) if `alternate`"""
    t = torch.full((rows, K // 2), 0x88, dtype=torch.uint8, device="cuda")
    if alternate:
        t[1::2] = 0x77
    return t


def const_expected(M, N, K):
    """[M, N] int32: rows all -8 against features all -8 (even) / all 7 (odd), from O.int4_matmul (G.const_product)"""
    pos, neg = G.const_product(-8, -8, K), G.const_product(-8, 7, K)
    assert pos == 64 * K and neg == -56 * K and pos < 1 << 31
    return np.tile(np.where(np.arange(N) % 2 == 0, pos, neg).astype(np.int32), (M, 1))


def accepted(fn):
    """fn() -> its result, or None if the library refuses the shape (FQ_EUNSUPPORTED: a refusal is not a wrong result)"""
    from flatquant_amd import _lib
    try:
        return fn()
    except _lib.FqError as e:
        assert e.code == _lib.FQ_EUNSUPPORTED, e
        return None


def range_scales(M, N):
    """scales of 2^-k (the products are exact): an output is +-65176 * 10 * 2^-k, its sign the accumulator's"""
    return np.full(M, 2.0 ** -8, dtype=np.float16), (2.0 ** -(2 + np.arange(N) % 4)).astype(np.float16)


@pytest.mark.parametrize("K", [G.INT8_K_LIMIT - 128, G.INT8_K_LIMIT - 64, G.INT8_K_LIMIT])
def test_accumulator_range_weight_streaming(ops, K):
    """256 * 64 * K reaches 2^31 at K = 131072: every launch of the weight-streaming kernel is exact below and REFUSES from there"""
    from flatquant_amd._lib import lib
    M, N = 2, 32
    x, w = const_rows(M, K, False), const_rows(N, K, True)
    img = ops.int4_to_frag(w)
    c = const_expected(M, N, K)
    sx, sw = range_scales(M, N)
    b = G.bias(N)
    ok = K < G.INT8_K_LIMIT
    runs = {
        "int4_skinny_matmul": lambda: ops.int4_skinny_matmul(x, img, N),
        "int4_skinny_linear unsplit": lambda: ops.int4_skinny_linear(x, dev(sx), img, dev(sw), dev(b), N, split=False),
        "int4_skinny_linear split": lambda: ops.int4_skinny_linear(x, dev(sx), img, dev(sw), None, N),
        "int4_skinny_linear_multi": lambda: ops.int4_skinny_linear_multi([(x, dev(sx), img, dev(sw), None), (x, dev(sx), img, dev(sw), dev(b))]),
    }
    for name, fn in runs.items():
        got = accepted(fn)
        if got is not None:                                # an accepted shape returns no wrapped accumulator
            if name == "int4_skinny_matmul":
                same_ints(got, c, f"{name} K={K}")
            elif name == "int4_skinny_linear_multi":
                same_bits(got[0], oracle_linear(c, sx, sw, None), f"{name}[0] K={K}")
                same_bits(got[1], oracle_linear(c, sx, sw, b), f"{name}[1] K={K}")
            else:
                same_bits(got, oracle_linear(c, sx, sw, b if "unsplit" in name else None), f"{name} K={K}")
        assert (got is not None) == ok, (name, K)
    assert ops.skinny_supported(M, K) == ok
    assert (int(lib.fq_int4_skinny_split_workspace_bytes(M, N, K)) > 0) == ok      # (below the limit the default launch above WAS the split one)


def test_module_leaves_the_weight_streaming_kernel_at_its_k_limit(ops):
    """deploy.nn.Linear4bit follows ops.skinny_supported: in_features = 131072 at decode rows runs the general-shape kernel, exact"""
    import flatquant_amd.deploy as deploy
    K, N, M = G.INT8_K_LIMIT, 32, 2
    lin = deploy.nn.Linear4bit(K, N, bias=True).cuda()
    sx, sw = range_scales(M, N)
    b = G.bias(N)
    lin.weight.copy_(const_rows(N, K, True))
    lin.weight_scales.copy_(dev(sw).reshape(N, 1))
    lin.bias.copy_(dev(b))
    p = deploy.PackedQuantizedTensor(const_rows(M, K, False).reshape(M, 1, K // 2), dev(sx).reshape(M, 1, 1))
    y = lin(p)
    assert getattr(lin, "_dimg", None) is None              # no decode image was built: the weight-streaming kernel did not run
    same_bits(y.reshape(M, N), oracle_linear(const_expected(M, N, K), sx, sw, b), "Linear4bit K=131072")


@pytest.mark.parametrize("K,M", [(G.INT8_K_LIMIT - 128, 2), (G.INT8_K_LIMIT, 2), (G.GENERAL_K_CAP - 32, 1), (G.GENERAL_K_CAP, 1), (G.GENERAL_K_CAP + 32, 1)])
def test_accumulator_range_int8_path(ops, K, M):
    """int4_matmul / int4_linear: the tile kernel up to K = 131072 - 128, the general-shape kernel (unscaled products: 64 K < 2^31) from 131072
    to 2^25 - 32, refused beyond"""
    N = 16
    x, w = const_rows(M, K, False), const_rows(N, K, True)
    ok = K <= G.GENERAL_K_CAP
    sx, sw = range_scales(M, N)
    b = G.bias(N)
    got = accepted(lambda: ops.int4_matmul(x, w))
    if got is not None and 64 * K < 1 << 31:
        same_ints(got, const_expected(M, N, K), f"int4_matmul K={K}")
    assert (got is not None) == ok, K
    for bb in (None, b):
        got = accepted(lambda: ops.int4_linear(x, dev(sx), w, dev(sw), None if bb is None else dev(bb)))
        if got is not None and 64 * K < 1 << 31:
            same_bits(got, oracle_linear(const_expected(M, N, K), sx, sw, bb), f"int4_linear K={K} bias={bb is not None}")
        assert (got is not None) == ok, K


@pytest.mark.parametrize("M", [2, 129])
@pytest.mark.parametrize("K", [G.FP6_K_CAP - 128, G.FP6_K_CAP, G.FP6_K_CAP + 128])
def test_accumulator_range_fp6_path(ops, K, M):
    """the fp32 accumulator holds the integer sum up to 64 * 2^18 = 2^24 exactly; the next K is refused"""
    N = 32
    x, w = const_rows(M, K, False), const_rows(N, K, True)
    ok = K <= G.FP6_K_CAP
    assert ops.bf6_supported(N, K) == ok
    xb, wb = ops.int4_to_bf6(x), ops.int4_to_bf6(w, weights=True)
    sx, sw = range_scales(M, N)
    b = G.bias(N)
    if ok:
        c = const_expected(M, N, K)
    got = accepted(lambda: ops.bf6_matmul(xb, wb, M, N, K))
    if got is not None and ok:
        same_ints(got, c, f"bf6_matmul K={K} M={M}")
    assert (got is not None) == ok
    runs = {
        "bf6_linear": lambda bb: ops.bf6_linear(xb, dev(sx), wb, dev(sw), bb, M, N, K),
        "int4_linear_fp6 kept": lambda bb: ops.int4_linear_fp6(x, dev(sx), w, wb, dev(sw), bb),
        "int4_linear_fp6 transient": lambda bb: ops.int4_linear_fp6(x, dev(sx), w, None, dev(sw), bb),
        "int4_linear_fp6_multi": lambda bb: ops.int4_linear_fp6_multi([(x, dev(sx), w, wb, dev(sw), bb), (x, dev(sx), w, None, dev(sw), bb)])[1],
    }
    for name, fn in runs.items():
        for bb in (None, b):
            got = accepted(lambda: fn(None if bb is None else dev(bb)))
            if got is not None and ok:
                same_bits(got, oracle_linear(c, sx, sw, bb), f"{name} K={K} M={M} bias={bb is not None}")
            assert (got is not None) == ok, (name, K)
