"""The head transform as the GEMM's prologue, decode regime (fq_block_linear_f16): ONE launch for o_proj_trans -> quantizer -> o_proj on 1..16
tokens of hidden size 4096 (deploy/transformers/modeling_llama.py:141-148; deploy/kernels/block_matmul.py; deploy/nn/linear.py:40-54).
The bar is bit-exactness against the two launches it replaces (fq_block_quant_f16 -> fq_int4_skinny_linear_f16, which test_gpu_block.py and
test_gpu_gemm.py hold to the oracle), directly against the oracle's own chain, the memory contract under guard bands, and the module / fuse
layers above the op."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fq_oracle as O
from tests import edge_tokens, guards

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
R, C, K = 128, 32, 4096


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


def _P(seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(C, C, generator=gen) / C ** 0.5 + torch.eye(C) * 0.5).half().cuda()


def tokens(M, seed):
    """M tokens [M, R, C]: ordinary Gaussian tokens at the even positions, edge tokens (tests/edge_tokens.py) between them at the odd ones —
    all-zero, one-hot, single-signed, subnormal, rounding ties, a second one-hot (last element), the 15000 outlier, the smallest subnormal —
    and the outlier x[2, 99, 5] = 1500 inside an ordinary token."""
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=gen) * (1 + 3 * torch.rand(M, 1, generator=gen))).half()
    e = torch.from_numpy(edge_tokens.edge_rows(R, C))
    for pos, row in zip(range(1, M, 2), (0, 3, 1, 6, 7, 4, 5, 8)):
        x[pos] = e[row]
    x = x.reshape(M, R, C)
    if M > 2:
        x[2, 99, 5] = 1500.0
    return x.cuda()


_PROBLEMS = {}


def problem(ops, N):
    """(packed weights [N, K/2], their image, scales, bias) of an N-feature Linear4bit, built once per N on the device"""
    if N not in _PROBLEMS:
        gen = torch.Generator(device="cuda").manual_seed(N)
        wp = torch.randint(0, 256, (N, K // 2), generator=gen, device="cuda", dtype=torch.uint8)
        ws = (torch.rand(N, generator=gen, device="cuda") * 0.01 + 0.001).half()
        b = (torch.randn(N, generator=gen, device="cuda") * 0.1).half()
        _PROBLEMS[N] = (wp, ops.int4_to_frag(wp), ws, b)
    return _PROBLEMS[N]


def two_launches(ops, x, P, sig, fl, img, ws, b, N):
    from flatquant_amd._lib import FQ_OUT_PACKED
    o = ops.block_quant(x, P, [sig], FQ_OUT_PACKED | fl, transpose_out=True)
    return ops.int4_skinny_linear(o.q[0].reshape(x.shape[0], K // 2), o.scale[0], img, ws, b, N)


# one tile in all, one tile per workgroup, five tiles per workgroup on 256 CUs (every wait count of the ring)
@pytest.mark.parametrize("N", [32, 4096, 40960])
@pytest.mark.parametrize("M", [1, 2, 7, 8, 9, 16])
def test_fused_launch_equals_the_two_launches(ops, M, N):
    from flatquant_amd._lib import FQ_NO_CLAMP0
    x, P = tokens(M, 100 * M + N % 97), _P(M)
    _, img, ws, b = problem(ops, N)
    for fl in (0, FQ_NO_CLAMP0):
        for sig in ((1.0, 1.0), (0.71, 0.83)):
            for bias in (None, b):
                ref = two_launches(ops, x, P, sig, fl, img, ws, bias, N)
                for _ in range(3):          # (repeatable: no state survives a launch)
                    got = ops.block_linear(x, P, sig, img, ws, bias, N, flags=fl)
                    assert got is not None and got.shape == (M, N)
                    assert torch.equal(ref, got), (M, N, fl, sig, bias is not None, int((ref != got).sum()))


@pytest.mark.parametrize("N", [256, 96])
def test_fused_launch_against_the_oracle_chain(ops, N):
    """x -> block_quant (oracle) -> linear4bit (oracle), 5 tokens"""
    from flatquant_amd._lib import FQ_NO_CLAMP0, FQ_OUT_PACKED
    M, sig = 5, (0.9, 0.8)
    gen = torch.Generator().manual_seed(3 + N)
    x = torch.randn(M, R, C, generator=gen).half()
    P = _P(7)
    wp, img, ws, b = problem(ops, N)
    got = ops.block_linear(x.cuda(), P, sig, img, ws, b, N, flags=FQ_NO_CLAMP0).cpu().numpy()
    o = O.block_quant(x.numpy(), P.cpu().numpy(), sig_max=sig[0], sig_min=sig[1], transpose_out=True, clamp0=False)
    y = O.linear4bit(o["packed"].reshape(M, K // 2), o["scale16"], wp.cpu().numpy(), ws.cpu().numpy(), b.cpu().numpy())
    # the oracle's transform accumulates in another order than the MFMA: a digit may flip on a rounding tie; compare the outputs of the tokens
    # whose digits agree with the kernel's own packed launch
    kq = ops.block_quant(x.cuda(), P, [sig], FQ_OUT_PACKED | FQ_NO_CLAMP0, transpose_out=True)
    same = (O.unpack_i4(kq.q[0].cpu().numpy().reshape(M, K // 2)) == np.asarray(o["q"]).reshape(M, K)).all(axis=1)
    assert same.sum() >= M - 1
    assert np.array_equal(got[same].view(np.uint16), y[same].view(np.uint16))


def test_uncovered_shapes_return_none_or_say_so(ops):
    from flatquant_amd import _lib
    _, img, ws, _ = problem(ops, 96)
    P = _P(1)
    x17 = torch.randn(17, R, C).half().cuda()
    assert ops.block_linear(x17, P, (1.0, 1.0), img, ws, None, 96) is None                                       # M = 17
    x64 = torch.randn(2, 64, 64).half().cuda()
    assert ops.block_linear(x64, torch.eye(64).half().cuda(), (1.0, 1.0), img, ws, None, 96) is None             # (R, C) = (64, 64)
    x2 = torch.randn(2, R, C).half().cuda()
    assert ops.block_linear(x2, P, (1.0, 1.0), img, ws[:48].contiguous(), None, 48) is None                      # N = 48
    y = torch.full((17, 96), 3.0, dtype=torch.float16, device="cuda")
    one = ctypes.c_float(1.0)

    def raw(x, Pm, M, Rr, Cc, N):
        return _lib.lib.fq_block_linear_f16(x.data_ptr(), Pm.data_ptr(), M, Rr, Cc, one, one, 0, img.data_ptr(), ws.data_ptr(), None, N,
                                            y.data_ptr(), None)
    assert raw(x17, P, 17, R, C, 96) == _lib.FQ_EUNSUPPORTED
    assert raw(x64, P, 2, 64, 64, 96) == _lib.FQ_EUNSUPPORTED
    assert raw(x2, P, 2, R, C, 48) == _lib.FQ_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())                                                                                 # nothing was launched


@pytest.mark.parametrize("M", [1, 7, 16])
def test_memory_contract_under_guard_bands(ops, M):
    """x, P, the image, the scales and the bias sit between pads that would change a result if they were read (NaN / 0xFF-class bytes), y
    between poisoned pads with a poisoned payload: nothing outside y is written, every byte of y is (the two poisons give the same bytes),
    and the result is the unguarded one."""
    from flatquant_amd._lib import FQ_NO_CLAMP0
    N, sig = 4096 + 64, (0.9, 0.33)         # 130 feature tiles, no power of two
    x, P = tokens(M, 11 * M), _P(20 + M)
    _, img, ws, b = problem(ops, N)
    want = ops.block_linear(x, P, sig, img, ws, b, N, flags=FQ_NO_CLAMP0)
    assert torch.equal(want, two_launches(ops, x, P, sig, FQ_NO_CLAMP0, img, ws, b, N))
    got = []
    for poison in guards.POISONS:
        g = guards.Guard(poison)
        with g.on(ops):
            gx, gP, gi, gw, gb = (g.guard_input(t) for t in (x, P, img, ws, b))
            y = ops.block_linear(gx, gP, sig, gi, gw, gb, N, flags=FQ_NO_CLAMP0)
            torch.cuda.synchronize()
        g.check()
        assert any(r.what == "empty" and r.shape == (M, N) for r in g.records), "y was not allocated under the guard"
        got.append(y)
    assert guards.same_raw(got[0], got[1]), "differs between the two poisons: y not written completely, or a pad was read"
    assert guards.same_raw(got[0], want)


def _pair(N, bias, seed):
    import flatquant_amd.deploy as deploy
    g = torch.Generator(device="cuda").manual_seed(seed)
    o_t = deploy.nn.OnlineTrans(C, trans="matmul", decompose=False).cuda()
    o_t.right_matrix.copy_(torch.randn(C, C, generator=g, device="cuda") / C ** 0.5)
    o_t.clip_factor_a_max.fill_(2.5), o_t.clip_factor_a_min.fill_(1.75)
    o_l = deploy.nn.Linear4bit(K, N, bias=bias).cuda()
    o_l.weight.copy_(torch.randint(0, 256, o_l.weight.shape, generator=g, device="cuda", dtype=torch.uint8))
    o_l.weight_scales.copy_(torch.rand(o_l.weight_scales.shape, generator=g, device="cuda") * 0.02 + 0.005)
    if bias:
        o_l.bias.copy_(torch.randn(N, generator=g, device="cuda") * 0.1)
    return o_t, o_l


def _chain(o_t, o_l, x4):
    """the reference's module chain, modeling_llama.py:143-146"""
    bsz, seq = x4.shape[:2]
    p = o_t(x4)
    p.quantized_x = p.quantized_x.contiguous().reshape(bsz, seq, -1)
    return o_l(p)


def test_fused_transform_linear_takes_the_head_transform(ops, monkeypatch):
    import flatquant_amd.deploy as deploy
    from flatquant_amd.deploy.nn import linear
    assert 0 <= linear.FUSED_HEAD_ROWS <= 16
    with torch.no_grad():
        o_t, o_l = _pair(4096, True, 5)
        calls = []
        real = ops.block_linear
        monkeypatch.setattr(ops, "block_linear", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        shapes = [(1, 1), (8, 1), (2, 4)] + [(linear.FUSED_HEAD_ROWS + 1, 1)]          # bsz x seq in {1, 8}, and one token above the constant
        for forced_off in (False, True):
            if forced_off:
                monkeypatch.setattr(linear, "FUSED_HEAD_ROWS", 0)
            for bsz, seq in shapes:
                x4 = tokens(bsz * seq, 31 * bsz + seq).reshape(bsz, seq, R, C)
                want = _chain(o_t, o_l, x4)
                n0 = len(calls)
                got = deploy.nn.fused_transform_linear(x4, [o_t], [o_l])
                assert len(got) == 1 and got[0].shape == (bsz, seq, 4096) and torch.equal(got[0], want), (bsz, seq, forced_off)
                fused = not forced_off and 1 <= bsz * seq <= linear.FUSED_HEAD_ROWS
                assert len(calls) - n0 == (1 if fused else 0), (bsz, seq, forced_off)
        # the decomposed route is what it was: a non-decomposed transform among several still raises
        with pytest.raises(RuntimeError):
            deploy.nn.fused_transform_linear(torch.zeros(1, 1, K, device="cuda", dtype=torch.float16), [o_t, o_t], [o_l, o_l])


def _capture(fn, x):
    xs = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        fn(xs)                                               # (warm-up on the side stream: images, host scalars)
        with torch.cuda.graph(graph, stream=s):
            got = fn(xs)
    torch.cuda.synchronize()
    return graph, xs, got


@pytest.fixture
def route_on(monkeypatch):
    """the fuse tests are about the mechanism, whatever the measured routing constant says (0 turns the route off)"""
    from flatquant_amd.deploy.nn import linear
    monkeypatch.setattr(linear, "FUSED_HEAD_ROWS", 16)


def test_fuse_o_proj_joins_the_pair_under_capture(route_on):
    import flatquant_amd.deploy as deploy
    from flatquant_amd.deploy.fuse import HeadGroup
    from ref_layer import RefLayer
    with torch.no_grad():
        layer = RefLayer("tiny", seed=5)
        g = torch.Generator(device="cuda").manual_seed(13)
        x = torch.randn(3, 1, 4096, generator=g, device="cuda", dtype=torch.float16)
        x2 = torch.randn(3, 1, 4096, generator=g, device="cuda", dtype=torch.float16)
        want, want2 = layer(x), layer(x2)                                        # the eager unfused layer
        assert deploy.fuse(layer) == {"transform_groups": 2, "linear_groups": 2, "down_proj": 1}      # without the flag: today's dict
        deploy.unfuse(layer)
        rep = deploy.fuse(layer, o_proj=True)
        assert rep["o_proj"] == 1 and rep["transform_groups"] == 2
        assert deploy.fuse(layer, o_proj=True)["o_proj"] == 0                    # idempotent
        a = layer.self_attn
        hg = a.o_proj_trans.__dict__["_group"]
        assert isinstance(hg, HeadGroup) and a.o_proj[1].__dict__["_group"] is hg
        for u, v in zip(layer(x), want):                                         # eager decode-sized: the modules' own forward
            assert torch.equal(u, v)
        big = torch.randn(1, 130, 4096, generator=g, device="cuda", dtype=torch.float16)
        ref_big = layer(big)
        assert (hg.fused, hg.launches, hg.lazy) == (0, 0, 0)
        graph, xs, got = _capture(layer, x)
        assert (hg.fused, hg.launches, hg.lazy) == (1, 0, 1)                     # one fused launch, no transform launch, no bytes materialised
        assert hg._out is None and hg._lazy_x is None                            # nothing activation-sized is kept
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(got, want):
            assert torch.equal(u, v)
        xs.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(got, want2):
            assert torch.equal(u, v)
        del graph
        deploy.unfuse(layer)
        assert "_group" not in a.o_proj_trans.__dict__ and "_group" not in a.o_proj[1].__dict__
        for u, v in zip(layer(x), want):                                         # the reference structure again
            assert torch.equal(u, v)
        for u, v in zip(layer(big), ref_big):
            assert torch.equal(u, v)


def test_fuse_o_proj_through_graphed_decode(route_on):
    import flatquant_amd.deploy as deploy
    from ref_layer import RefLayer
    with torch.no_grad():
        layer = RefLayer("tiny", seed=9)
        g = torch.Generator(device="cuda").manual_seed(17)
        xs = [torch.randn(3, 1, 4096, generator=g, device="cuda", dtype=torch.float16) for _ in range(4)]
        want = [[t.clone() for t in layer(x)] for x in xs]
        rep = deploy.fuse(layer, capture=True, o_proj=True)
        assert rep["o_proj"] == 1 and rep["graphed_layers"] == 1
        hg = layer.self_attn.o_proj_trans.__dict__["_group"]
        gd = layer.__dict__["forward"]
        for x, w in zip(xs, want):                                               # two eager warm-ups, the capture, a replay
            for u, v in zip(layer(x), w):
                assert torch.equal(u, v)
        assert gd.captures == 1 and gd.replays >= 2
        assert (hg.fused, hg.launches, hg.lazy) == (1, 0, 1)
        deploy.unfuse(layer)
        for u, v in zip(layer(xs[0]), want[0]):
            assert torch.equal(u, v)


def test_lazy_head_tensor_gives_the_bytes_to_anyone_who_asks(route_on):
    """Under capture the o_proj transform hands out a lazy packed tensor: shape, dtype and device are answered, the reference's reshape
    stays lazy; a real tensor assigned to .quantized_x, a read of .scales_x, or another consumer get the two-launch bytes, once."""
    import flatquant_amd.deploy as deploy
    from flatquant_amd.deploy import LazyHeadPackedQuantizedTensor, PackedQuantizedTensor
    with torch.no_grad():
        o_t, o_l = _pair(256, False, 3)
        other = _pair(256, False, 4)[1]
        holder = torch.nn.Module()
        holder.o_proj_trans, holder.o_proj = o_t, torch.nn.Sequential(deploy.nn.Quantizer(lac=True).cuda(), o_l)
        x4 = tokens(3, 77).reshape(3, 1, R, C)
        ref = o_t(x4)
        want_other = other(PackedQuantizedTensor(ref.quantized_x.reshape(3, 1, -1), ref.scales_x))
        assert deploy.fuse(holder, o_proj=True)["o_proj"] == 1
        hg = o_t.__dict__["_group"]
        seen = {}

        def step(x):
            p = o_t(x)
            seen["lazy"] = type(p) is LazyHeadPackedQuantizedTensor
            seen["meta"] = (p.quantized_x.device.type, tuple(p.size()), p.dtype, p.device.type)
            p.quantized_x = p.quantized_x.contiguous().reshape(3, 1, -1)
            seen["still_lazy"] = type(p) is LazyHeadPackedQuantizedTensor and tuple(p.size()) == (3, 1, K // 2)
            y = other(p)                                                          # a consumer other than the group's Linear4bit
            seen["plain"] = type(p) is PackedQuantizedTensor
            return y, p.quantized_x, p.scales_x

        graph, xs, (y, q, sc) = _capture(step, x4)
        graph.replay()
        torch.cuda.synchronize()
        assert seen == {"lazy": True, "meta": ("meta", (3, 1, R // 2, C), torch.uint8, "cuda"), "still_lazy": True, "plain": True}
        assert (hg.fused, hg.launches, hg.lazy) == (0, 1, 1)
        assert torch.equal(q.reshape(-1), ref.quantized_x.reshape(-1)) and torch.equal(sc.reshape(-1), ref.scales_x.reshape(-1))
        assert torch.equal(y, want_other)
