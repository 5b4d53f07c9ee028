"""The grouped INT4 GEMM / Linear4bit (fq_int4_gemm_grouped_i32, fq_int4_linear_grouped_f16, ops.int4_matmul_grouped / int4_linear_grouped,
deploy.nn.Linear4bitGrouped): every expert's GEMM in one launch. Integer work plus the sym_dequant epilogue, so every comparison is
bit-exact and has no tolerance. The reference is always the loop over the groups' row slices — the oracle's
(tests/gemm_grouped_ref.py) and the dense GPU path's (ops.int4_matmul / ops.int4_linear) — never the grouped code itself."""
import functools

import numpy as np
import pytest
import torch

from oracle import fq_oracle as O
from tests import gemm_grouped_ref as R
from tests import guards

pytestmark = pytest.mark.gpu

G = R.G_SIZES


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.cpu().numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def problem(sizes, N, K, seed=0):
    """random nibbles in -8..7, different weights per group, positive scales, a bias -> numpy arrays (shared, never modified)"""
    rng = np.random.default_rng(1000 * seed + 7 * N + K + len(sizes))
    rows, n = int(sum(sizes)), len(sizes)
    xq = rng.integers(-8, 8, (rows, K), dtype=np.int32)
    wq = rng.integers(-8, 8, (n, N, K), dtype=np.int32)
    sx = (rng.random(rows) * 0.05 + 0.001).astype(np.float16)
    sw = (rng.random((n, N)) * 0.02 + 0.0005).astype(np.float16)
    b = rng.standard_normal((n, N)).astype(np.float16)
    return dict(xq=xq, wq=wq, xp=O.pack_i4(xq), wp=O.pack_i4(wq), sx=sx, sw=sw, b=b, off=R.offsets_of(sizes))


def int64_product(p):
    off = p["off"]
    return np.concatenate([p["xq"][off[g]:off[g + 1]].astype(np.int64) @ p["wq"][g].astype(np.int64).T for g in range(len(off) - 1)]).astype(np.int32)


def loop_linear(ops, xp, sx, wp, sw, off, b=None):
    """the dense GPU path group by group, with host-known offsets"""
    parts = [ops.int4_linear(xp[off[g]:off[g + 1]], sx[off[g]:off[g + 1]], wp[g], sw[g], None if b is None else b[g])
             for g in range(len(off) - 1) if off[g + 1] > off[g]]
    return torch.cat(parts) if parts else torch.empty((0, wp.shape[1]), dtype=torch.float16, device="cuda")


# ---- 1. int32, bit-exact
@pytest.mark.parametrize("N,K", [(256, 128), (272, 256), (48, 384), (1024, 512)])   # (272: an N-tile edge)
def test_int32_bit_exact(ops, N, K):
    p = problem(tuple(G), N, K)
    c = ops.int4_matmul_grouped(dev(p["xp"]), dev(p["wp"]), dev(p["off"]))
    assert c.shape == (1549, N) and c.dtype == torch.int32
    assert np.array_equal(c.cpu().numpy(), int64_product(p))


# ---- 2. closed form: a wrong group, a wrong row bound or a clamped-row leak is a wrong constant in a known row
def test_closed_form(ops):
    K, N, n = 128, 32, len(G)
    off = R.offsets_of(G)
    xp = O.pack_i4(np.ones((1549, K), dtype=np.int32))
    wq = np.empty((n, N, K), dtype=np.int32)
    for g in range(n):
        wq[g] = (g % 15) - 7
    c = ops.int4_matmul_grouped(dev(xp), dev(O.pack_i4(wq)), dev(off)).cpu().numpy()
    group_of_row = np.repeat(np.arange(n), G)
    want = (K * ((group_of_row % 15) - 7)).astype(np.int32)
    assert np.array_equal(c, np.broadcast_to(want[:, None], (1549, N)))


# ---- 3. fused linear: the oracle's bits and the dense GPU loop's
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N,K", [(272, 256), (256, 4096)])
def test_fused_linear(ops, N, K, bias):
    p = problem(tuple(G), N, K)
    xp, sx, wp, sw, off = dev(p["xp"]), dev(p["sx"]), dev(p["wp"]), dev(p["sw"]), dev(p["off"])
    b = dev(p["b"]) if bias else None
    y = ops.int4_linear_grouped(xp, sx, wp, sw, off, b)
    assert y.shape == (1549, N) and y.dtype == torch.float16
    ref = R.grouped_linear4bit_ref(p["xp"], p["sx"], p["wp"], p["sw"], p["off"], p["b"] if bias else None)
    assert np.array_equal(bits(y), ref.view(np.uint16))
    assert guards.same_raw(y, loop_linear(ops, xp, sx, wp, sw, p["off"], b))


# ---- 4. the clamp branch of the epilogue (Kb > 10176 / 2 selects dequant16f<true>): int(c / 10) against +-65176
# K = 10240, all nibbles -8 on both sides: c = 655360, int(c / 10) = 65536 > 65176 — the clamp binds on the positive side.
# K = 10240, weights all +7: c = -573440, int(c / 10) = -57344: the clamped epilogue runs, but 57344 < 65176 — at this K no product of
#   nibbles reaches the negative bound (-8 x 7 = -56 per element needs K > 11638), so this case pins the branch, not the bound.
# K = 11776 (the next multiple of 128 beyond that), weights all +7: c = -659456, int(c / 10) = -65945 — the clamp binds on the negative side.
@pytest.mark.parametrize("K,w_nibble,c_want,binds", [(10240, -8, 655360, True), (10240, 7, -573440, False), (11776, 7, -659456, True)])
def test_clamp_branch(ops, K, w_nibble, c_want, binds):
    N, sizes = 32, (3, 0, 130)
    rows, n = sum(sizes), len(sizes)
    assert K > 10176 and c_want == -8 * w_nibble * K and (abs(int(c_want / 10)) > 65176) == binds
    rng = np.random.default_rng(4)
    xp = O.pack_i4(np.full((rows, K), -8, dtype=np.int32))
    wp = O.pack_i4(np.full((n, N, K), w_nibble, dtype=np.int32))
    sx = (rng.random(rows) * 0.01 + 0.001).astype(np.float16)
    sw = (rng.random((n, N)) * 0.01 + 0.0005).astype(np.float16)
    off = R.offsets_of(sizes)
    c = ops.int4_matmul_grouped(dev(xp), dev(wp), dev(off))
    assert bool((c == c_want).all())
    y = ops.int4_linear_grouped(dev(xp), dev(sx), dev(wp), dev(sw), dev(off))
    ref = R.grouped_linear4bit_ref(xp, sx, wp, sw, off)
    assert np.array_equal(bits(y), ref.view(np.uint16))
    # where the clamp binds, the reference is what the accumulator AT the clamp (int(651760 / 10) = 65176) gives
    at_clamp = np.full((rows, N), 651760 * (1 if c_want > 0 else -1), dtype=np.int32)
    same = np.concatenate([O.sym_dequant(at_clamp[off[g]:off[g + 1]], sx[off[g]:off[g + 1]], sw[g]) for g in range(n) if off[g + 1] > off[g]])
    assert np.array_equal(ref.view(np.uint16), same.view(np.uint16)) == binds


# ---- 5. the general-shape kernel
@pytest.mark.parametrize("N,K", [(40, 96), (24, 160)])
def test_general_shape_fallback(ops, N, K):
    p = problem((7, 0, 65), N, K)
    xp, sx, wp, sw, off, b = dev(p["xp"]), dev(p["sx"]), dev(p["wp"]), dev(p["sw"]), dev(p["off"]), dev(p["b"])
    assert np.array_equal(ops.int4_matmul_grouped(xp, wp, off).cpu().numpy(), int64_product(p))
    for bias in (None, b):
        y = ops.int4_linear_grouped(xp, sx, wp, sw, off, bias)
        ref = R.grouped_linear4bit_ref(p["xp"], p["sx"], p["wp"], p["sw"], p["off"], None if bias is None else p["b"])
        assert np.array_equal(bits(y), ref.view(np.uint16))
        assert guards.same_raw(y, loop_linear(ops, xp, sx, wp, sw, p["off"], bias))


# ---- 6. degenerate schedules, N = 32, K = 128
def _zipf_sizes(n_groups, rows, seed):
    rng = np.random.default_rng(seed)
    pop = 1.0 / np.arange(1, n_groups + 1)
    pop = rng.permutation(pop / pop.sum())
    return tuple(int(v) for v in np.bincount(rng.choice(n_groups, size=rows, p=pop), minlength=n_groups))


def _check_schedule(ops, sizes):
    p = problem(tuple(sizes), 32, 128, seed=6)
    xp, sx, wp, sw, off, b = dev(p["xp"]), dev(p["sx"]), dev(p["wp"]), dev(p["sw"]), dev(p["off"]), dev(p["b"])
    c = ops.int4_matmul_grouped(xp, wp, off)
    assert np.array_equal(c.cpu().numpy(), int64_product(p))
    y = ops.int4_linear_grouped(xp, sx, wp, sw, off, b)
    assert np.array_equal(bits(y), R.grouped_linear4bit_ref(p["xp"], p["sx"], p["wp"], p["sw"], p["off"], p["b"]).view(np.uint16))
    return p, c, y


def test_one_group_is_the_dense_launch(ops):
    p, c, y = _check_schedule(ops, (300,))
    assert guards.same_raw(c, ops.int4_matmul(dev(p["xp"]), dev(p["wp"][0])))
    assert guards.same_raw(y, ops.int4_linear(dev(p["xp"]), dev(p["sx"]), dev(p["wp"][0]), dev(p["sw"][0]), dev(p["b"][0])))


@pytest.mark.parametrize("sizes", [(0,) * 7 + (300,), (300,) + (0,) * 7, _zipf_sizes(256, 300, 1), _zipf_sizes(1024, 1100, 2)],
                         ids=["all_in_last_of_8", "all_in_first_of_8", "zipf_256_groups_300_rows", "1024_groups_1100_rows"])
def test_degenerate_schedules(ops, sizes):
    assert len(sizes) in (8, 256, 1024) and sum(sizes) in (300, 1100)
    _check_schedule(ops, sizes)


def test_zipf_draw_is_mostly_tiny_groups():
    s = np.asarray(_zipf_sizes(256, 300, 1))
    assert (s <= 2).sum() > 128 and s.max() > 8


def test_zero_rows(ops):
    p = problem((5, 3), 32, 128, seed=6)
    off = torch.zeros(3, dtype=torch.int64, device="cuda")
    x0 = torch.empty((0, 64), dtype=torch.uint8, device="cuda")
    c = ops.int4_matmul_grouped(x0, dev(p["wp"]), off)
    y = ops.int4_linear_grouped(x0, torch.empty(0, dtype=torch.float16, device="cuda"), dev(p["wp"]), dev(p["sw"]), off)
    assert c.shape == (0, 32) and c.dtype == torch.int32 and y.shape == (0, 32) and y.dtype == torch.float16


# ---- 7. graph capture, offsets changed in place: the grid comes from the host-side bound, nothing is baked in from the offsets
def test_graph_replay_with_new_offsets(ops):
    first, second = (100, 0, 50, 200, 0, 120, 30, 100), (0, 257, 3, 0, 128, 12, 100, 100)    # 600 rows each; group 1 grows from 0 to 257
    assert sum(first) == sum(second) == 600
    p = problem(first, 64, 256, seed=7)                                                         # (rows and weights do not depend on the split)
    xp, sx, wp, sw, b = dev(p["xp"]), dev(p["sx"]), dev(p["wp"]), dev(p["sw"]), dev(p["b"])
    off = dev(R.offsets_of(first))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        ops.int4_linear_grouped(xp, sx, wp, sw, off, b)            # warm-up
        with torch.cuda.graph(graph, stream=side):
            y = ops.int4_linear_grouped(xp, sx, wp, sw, off, b)
    torch.cuda.current_stream().wait_stream(side)
    for sizes in (first, second, first):
        off.copy_(dev(R.offsets_of(sizes)))
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        ref = R.grouped_linear4bit_ref(p["xp"], p["sx"], p["wp"], p["sw"], R.offsets_of(sizes), p["b"])
        assert np.array_equal(bits(y), ref.view(np.uint16)), sizes


# ---- 8. the chain: the grouped transform's packed rows into the grouped linear
def test_chain_from_grouped_transform(ops):
    from flatquant_amd._lib import FQ_OUT_PACKED
    sizes, N = (40, 0, 1, 200, 15), 64
    rows, n = sum(sizes), len(sizes)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(rows, 2048, generator=gen).half().cuda()
    L = (torch.randn(32, 32, generator=gen) / 32 ** 0.5).half().cuda()
    Rm = (torch.randn(64, 64, generator=gen) / 8).half().cuda()
    smax = (0.5 + 0.5 * torch.rand(n, generator=gen)).cuda()
    smin = (0.3 + 0.7 * torch.rand(n, generator=gen)).cuda()
    off_np = R.offsets_of(sizes)
    off = dev(off_np)
    o = ops.kron_quant_grouped(x, L, Rm, off, smax, smin, FQ_OUT_PACKED)
    q, s = o.q[0], o.scale[0]
    assert q.shape == (rows, 1024) and s.shape == (rows,) and s.dtype == torch.float16
    p = problem(sizes, N, 2048, seed=8)
    wp, sw, b = dev(p["wp"]), dev(p["sw"]), dev(p["b"])
    y = ops.int4_linear_grouped(q, s, wp, sw, off, b)
    assert guards.same_raw(y, loop_linear(ops, q, s, wp, sw, off_np, b))
    ref = R.grouped_linear4bit_ref(q.cpu().numpy(), s.cpu().numpy(), p["wp"], p["sw"], off_np, p["b"])
    assert np.array_equal(bits(y), ref.view(np.uint16))


# ---- 9. memory contract
@pytest.mark.parametrize("N,K", [(272, 256), (256, 4096)])
def test_memory_contract_under_guard_bands(ops, N, K):
    """x and w_g between 0xFF / 0x88 pads, the scales and the bias between NaN pads, group_offsets between valid entries (its last one
    repeated), the outputs poisoned with poisoned pads: nothing outside the outputs is written, every byte of them is (the two poisons
    give the same bytes), and the results are the unguarded ones."""
    p = problem(tuple(G), N, K)
    ins = [dev(p[k]) for k in ("xp", "sx", "wp", "sw", "off", "b")]
    want_y = ops.int4_linear_grouped(*ins)
    want_c = ops.int4_matmul_grouped(ins[0], ins[2], ins[4])
    got = []
    for poison in guards.POISONS:
        g = guards.Guard(poison)
        with g.on(ops):
            gx, gsx, gw, gsw, goff, gb = (g.guard_input(t) for t in ins)
            y = ops.int4_linear_grouped(gx, gsx, gw, gsw, goff, gb)
            c = ops.int4_matmul_grouped(gx, gw, goff)
            torch.cuda.synchronize()
        g.check()
        assert sum(r.what == "empty" and r.shape == (1549, N) for r in g.records) == 2, "the outputs were not allocated under the guard"
        got.append((y, c))
    assert guards.same_raw(got[0][0], got[1][0]) and guards.same_raw(got[0][1], got[1][1]), "an output byte was not written, or a pad was read"
    assert guards.same_raw(got[0][0], want_y) and guards.same_raw(got[0][1], want_c)


# ---- 10. the module
@pytest.mark.parametrize("bias", [False, True])
def test_module(ops, bias):
    import flatquant_amd.deploy as deploy
    E, K, N, sizes = 4, 256, 48, (37, 0, 130, 5)
    torch.manual_seed(10)
    linears = [torch.nn.Linear(K, N, bias=bias).half() for _ in range(E)]
    scales = [(m.weight.data.abs().amax(dim=1, keepdim=True).float() / 7).half().cuda() for m in linears]
    grouped = deploy.nn.Linear4bitGrouped.from_float(linears, scales).cuda()
    singles = [deploy.nn.Linear4bit.from_float(m, s).cuda() for m, s in zip(linears, scales)]
    assert set(grouped.state_dict()) == {"weight", "weight_scales"} | ({"bias"} if bias else set())
    assert grouped.weight.shape == (E, N, K // 2) and grouped.weight.dtype == torch.uint8 and grouped.weight_scales.shape == (E, N, 1)
    assert grouped.weight_scales.dtype == singles[0].weight_scales.dtype
    for e in range(E):
        assert torch.equal(grouped.weight[e], singles[e].weight) and torch.equal(grouped.weight_scales[e], singles[e].weight_scales)
    p = problem(sizes, N, K, seed=10)
    q, s, off_np = dev(p["xp"]), dev(p["sx"]), R.offsets_of(sizes)
    y = grouped(deploy.PackedQuantizedTensor(q, s), dev(off_np))
    assert y.shape == (sum(sizes), N) and y.dtype == torch.float16
    for e in range(E):
        a, b_ = off_np[e], off_np[e + 1]
        if b_ > a:
            one = singles[e](deploy.PackedQuantizedTensor(q[a:b_], s[a:b_]))
            assert guards.same_raw(y[a:b_], one), e
