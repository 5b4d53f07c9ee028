"""deploy.fuse(model, capture=True) / deploy.GraphedDecode: a decoder layer's decode step served from captured HIP graphs with no graph code
on the caller's side (the reference's eager decode loop: deploy/transformers/modeling_llama.py:45-153,
benchmarks/layer_benchmark.py:131-143). The replayed step must be the eager step bit for bit, token after token, with the paged INT4 cache
really growing: two identical caches, one driven eagerly, one through the wrapper."""
import gc
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


def build(bsz, page, prompt, max_len, seed=0):
    import flatquant_amd.deploy as deploy
    import flatquant_amd.deploy.transformers as dt
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    hidden, heads, kv_heads, hd = 4096, 32, 8, 128

    def trans(dim, decompose=True):
        t = deploy.nn.OnlineTrans(dim, trans="matmul", decompose=decompose, lac=True).to(dev)
        for name in ("left_matrix", "right_matrix"):
            if name in t._buffers:
                b = t._buffers[name]
                b.copy_(torch.randn(b.shape, generator=g, device=dev) / b.shape[0] ** 0.5)
        t.clip_factor_a_max.fill_(4.0), t.clip_factor_a_min.fill_(3.5)
        return t

    def lin(k_in, n_out):
        m = deploy.nn.Linear4bit(k_in, n_out).to(dev)
        m.weight.copy_(torch.randint(0, 256, m.weight.shape, generator=g, device=dev, dtype=torch.uint8))
        m.weight_scales.copy_(torch.rand(m.weight_scales.shape, generator=g, device=dev) * 0.02 + 0.005)
        return m

    class Attn(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inp_trans_q = trans(hidden)
            self.q_proj, self.k_proj, self.v_proj, self.o_proj = lin(hidden, hidden), lin(hidden, kv_heads * hd), lin(hidden, kv_heads * hd), lin(hidden, hidden)
            self.o_proj_trans = trans(heads, decompose=False)
            self.register_buffer("tk", (torch.randn(hd, hd, generator=g, device=dev) / hd ** 0.5).half())

        def forward(self, h, cache):
            b = h.shape[0]
            p = self.inp_trans_q(h)
            q, k, v = self.q_proj(p), self.k_proj(p), self.v_proj(p)
            kw = {"trans_matrix_k": self.tk, "trans_matrix_k_inv_t": self.tk}
            attend = cache.update(k.view(b, 1, kv_heads, hd), v.view(b, 1, kv_heads, hd), 0, kw)
            po = self.o_proj_trans(attend(q.view(b, 1, heads, hd), transposed=True))
            po.quantized_x = po.quantized_x.contiguous().reshape(b, 1, -1)
            return self.o_proj(po)

    class Mlp(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inp_trans_u = trans(hidden)
            self.up_proj = lin(hidden, 1024)

        def forward(self, h):
            return self.up_proj(self.inp_trans_u(h))

    class Layer(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.self_attn, self.mlp = Attn(), Mlp()

        def forward(self, h, cache, scale=1.0):
            a = self.self_attn(h, cache)
            return h + a * scale, self.mlp(a)

    def new_cache(bsz=bsz, max_len=max_len, prompt=prompt):
        c = dt.MultiLayerPagedKVCache4Bit(bsz, page, max_len, dev, 1, heads, hd, trans="matmul", group_size=heads // kv_heads)
        gk = torch.Generator(device=dev).manual_seed(99)
        c.update(torch.randn(bsz, prompt, kv_heads, hd, generator=gk, device=dev).half(),
                 torch.randn(bsz, prompt, kv_heads, hd, generator=gk, device=dev).half(), 0,
                 {"trans_matrix_k": layer.self_attn.tk, "trans_matrix_k_inv_t": layer.self_attn.tk})
        return c

    layer = Layer()
    return layer, new_cache, g


@pytest.mark.parametrize("bsz", [1, 3])
def test_graphed_layer_replays_the_eager_step_token_after_token(bsz):
    import flatquant_amd.deploy as deploy
    with torch.no_grad():
        layer, new_cache, g = build(bsz, page=16, prompt=21, max_len=64)
        xs = [torch.randn(bsz, 1, 4096, generator=g, device="cuda", dtype=torch.float16) for _ in range(14)]
        ref_cache = new_cache()
        want = [tuple(t.clone() for t in layer(x, ref_cache)) for x in xs]           # eager, cache growing 21 -> 35 (crosses a page at 32)
        rep = deploy.fuse(layer, capture=True)
        assert rep["graphed_layers"] == 1
        gd = layer.__dict__["forward"]
        cache = new_cache()
        for i, x in enumerate(xs):
            got = layer(x, cache)
            assert cache.length == 21 + i + 1
            for a, b in zip(got, want[i]):
                assert torch.equal(a, b), i
        assert gd.eager_calls == 2 and gd.captures == 1 and gd.replays == 12        # two warm-up calls, then every step from the graph
        for pg in range(cache.page_cnt_from_length(cache.length)):                   # the rows the steps wrote (the pages are torch.empty beyond them)
            rows = min(cache.page_size, cache.length - pg * cache.page_size)
            for b in range(bsz):
                i = pg * bsz + b
                assert torch.equal(cache.pages[i, :, :, :, :rows], ref_cache.pages[i, :, :, :, :rows])
                assert torch.equal(cache.scales[i, :, :, :, :rows], ref_cache.scales[i, :, :, :, :rows])
        # another signature (a different python scalar argument) gets its own warm-up + graph; prefill-sized calls stay eager
        c2, c3 = new_cache(), new_cache()
        for x in xs[:4]:
            a = layer(x, c2, scale=0.5)
        deploy.unfuse(layer)
        for x in xs[:4]:
            b = layer(x, c3, scale=0.5)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        assert "forward" not in layer.__dict__


def test_page_growth_makes_the_graph_stale_and_it_is_recaptured():
    """max_seq_len 32 -> two pages per request allocated; the 33rd token re-allocates the pages (every pointer moves): the wrapper sees it
    coming (would_grow), runs that step eagerly and captures again over the new storage."""
    import flatquant_amd.deploy as deploy
    with torch.no_grad():
        layer, new_cache, g = build(2, page=16, prompt=26, max_len=32, seed=3)
        xs = [torch.randn(2, 1, 4096, generator=g, device="cuda", dtype=torch.float16) for _ in range(12)]
        ref_cache = new_cache()
        want = [tuple(t.clone() for t in layer(x, ref_cache)) for x in xs]           # 26 -> 38: grows at 33
        gd = deploy.GraphedDecode(layer.forward)
        cache = new_cache()
        gen0 = cache.generation
        for i, x in enumerate(xs):
            got = gd(x, cache)
            for a, b in zip(got, want[i]):
                assert torch.equal(a, b), i
        assert cache.generation > gen0 and gd.captures == 2 and cache.length == 38
        assert gd.eager_calls == 3                                                   # two warm-ups + the step that grew the pages


def test_calls_that_are_not_decode_steps_stay_eager():
    import flatquant_amd.deploy as deploy
    layer, new_cache, g = build(1, page=16, prompt=5, max_len=64, seed=5)
    gd = deploy.GraphedDecode(layer.mlp.forward)
    with torch.no_grad():
        big = torch.randn(1, 200, 4096, generator=g, device="cuda", dtype=torch.float16)
        for _ in range(4):
            gd(big)                                                                  # prefill-sized
        assert gd.captures == 0 and gd.replays == 0
        x = torch.randn(1, 1, 4096, generator=g, device="cuda", dtype=torch.float16)
        outs = [gd(x).clone() for _ in range(5)]
        assert gd.captures == 1 and gd.replays == 3 and all(torch.equal(o, outs[0]) for o in outs)
    xg = torch.randn(1, 1, 4096, device="cuda", dtype=torch.float16)
    n = gd.replays
    with torch.enable_grad():
        gd(xg)                                                                       # autograd on: eager
    assert gd.replays == n


def test_tensors_inside_containers_are_graph_inputs_and_changing_signatures_stay_bounded():
    """HF passes ``position_embeddings=(cos, sin)``: tensors inside tuples / dicts are copied into static inputs like top-level ones; a caller
    whose signature changes on every call (a growing mask) never captures, stays correct and does not grow the wrapper's tables."""
    import flatquant_amd.deploy as deploy

    def fn(h, pe=None, extra=None):
        cos, sin = pe
        return h * cos + sin + (0 if extra is None else extra["b"])

    gd = deploy.GraphedDecode(fn)
    g = torch.Generator(device="cuda").manual_seed(1)
    with torch.no_grad():
        for i in range(6):
            h, c, s_, b = (torch.randn(2, 1, 64, generator=g, device="cuda", dtype=torch.float16) for _ in range(4))
            got = gd(h, pe=(c, s_), extra={"b": b})
            assert torch.equal(got, fn(h, pe=(c, s_), extra={"b": b})), i
        assert gd.captures == 1 and gd.replays == 4
        gd.MAX_SIGNATURES = 8
        for i in range(40):                                   # a new shape every call: warm-up forever, tables bounded
            m = torch.ones(2, 1, 3 + i, device="cuda", dtype=torch.float16)
            assert gd(m, pe=(m, m)).shape == m.shape
        assert gd.captures == 1 and len(gd._seen) <= 8 and len(gd._logs) <= 8 and len(gd._entries) <= 8


def test_a_callable_that_cannot_be_captured_falls_back_to_eager_for_good():
    """An op that synchronises inside the callable makes stream capture fail: the wrapper runs that call eagerly, remembers the signature and never
    tries again — results stay right, nothing raises."""
    import flatquant_amd.deploy as deploy

    def fn(h):
        return h * float(h.abs().max().item())          # .item(): a device synchronisation, illegal under capture

    gd = deploy.GraphedDecode(fn)
    g = torch.Generator(device="cuda").manual_seed(2)
    with torch.no_grad():
        for i in range(6):
            h = torch.randn(1, 1, 64, generator=g, device="cuda", dtype=torch.float16)
            assert torch.equal(gd(h), fn(h)), i
    assert gd.captures == 0 and gd.replays == 0 and len(gd._blocked) == 1
    # the wrapper still captures other callables' signatures afterwards (the failed capture left no capture state behind)
    gd2 = deploy.GraphedDecode(lambda h: h + 1)
    with torch.no_grad():
        outs = [gd2(torch.ones(1, 1, 8, device="cuda", dtype=torch.float16)).clone() for _ in range(4)]
    assert gd2.captures == 1 and all(torch.equal(o, outs[0]) for o in outs)


def test_hf_shaped_layer_call_with_keyword_arguments():
    """The call shape of the reference's decoder layer (deploy/transformers/modeling_llama.py:45-153 behind HF's LlamaDecoderLayer.forward):
    everything by keyword — position ids and cache position as tensors that change every step, (cos, sin) as a tuple, the cache as
    ``past_key_value``, flags as Python bools, a tuple coming back — through deploy.fuse(model, capture=True), against the eager layer."""
    import flatquant_amd.deploy as deploy
    with torch.no_grad():
        inner, new_cache, g = build(2, page=16, prompt=9, max_len=64, seed=8)

        class HFLayer(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.self_attn, self.mlp = inner.self_attn, inner.mlp

            def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_value=None, output_attentions=False,
                        use_cache=False, cache_position=None, position_embeddings=None):
                cos, sin = position_embeddings
                h = hidden_states * cos + sin + position_ids.to(hidden_states.dtype).unsqueeze(-1) * 0.001
                a = self.self_attn(h, past_key_value)
                out = (hidden_states + a + cache_position.to(a.dtype).reshape(1, 1, 1) * 0.01,)
                return out + ((self.mlp(a),) if use_cache else ())

        layer = HFLayer()
        steps = []
        for t in range(8):
            steps.append(dict(hidden_states=torch.randn(2, 1, 4096, generator=g, device="cuda", dtype=torch.float16), attention_mask=None,
                              position_ids=torch.full((2, 1), 9 + t, device="cuda"), output_attentions=False, use_cache=True,
                              cache_position=torch.tensor([9 + t], device="cuda"),
                              position_embeddings=(torch.rand(2, 1, 4096, generator=g, device="cuda", dtype=torch.float16),
                                                   torch.rand(2, 1, 4096, generator=g, device="cuda", dtype=torch.float16))))
        ref_cache = new_cache()
        want = [tuple(o.clone() for o in layer(past_key_value=ref_cache, **kw)) for kw in steps]
        assert deploy.fuse(layer, capture=True)["graphed_layers"] == 1
        cache = new_cache()
        for t, kw in enumerate(steps):
            got = layer(past_key_value=cache, **kw)
            assert isinstance(got, tuple) and len(got) == 2
            for a, b in zip(got, want[t]):
                assert torch.equal(a, b), t
        gd = layer.__dict__["forward"]
        assert gd.captures == 1 and gd.replays == 6 and cache.length == ref_cache.length == 17


# ---------------------------------------------------------------------------------------------------------------------------------------
# Graph and image LIFETIMES: which cache a captured graph belongs to, what happens when that cache dies or another takes its place, a graph
# replayed far past the length it was captured at, operand images after an in-place reload. The oracle is the file's own: an eager twin, bit
# for bit, outputs AND the cache bytes the steps wrote. (The host logic alone: tests/test_graphed_cpu.py.)
# ---------------------------------------------------------------------------------------------------------------------------------------
def assert_same_rows(cache, ref):
    """the rows the steps wrote (the pages are torch.empty beyond them): same bytes in both caches"""
    assert cache.length == ref.length and cache.batch_size == ref.batch_size
    bsz = cache.batch_size
    for pg in range(cache.page_cnt_from_length(cache.length)):
        rows = min(cache.page_size, cache.length - pg * cache.page_size)
        sl = slice(pg * bsz, (pg + 1) * bsz)
        assert torch.equal(cache.pages[sl, :, :, :, :rows], ref.pages[sl, :, :, :, :rows]), pg
        assert torch.equal(cache.scales[sl, :, :, :, :rows].view(torch.int16), ref.scales[sl, :, :, :, :rows].view(torch.int16)), pg


def run_against_twin(call, layer, cache, twin, xs, what=""):
    """every step through ``call`` (the wrapper) on ``cache`` and eagerly on ``twin``: same outputs, one more token each"""
    for i, x in enumerate(xs):
        l0 = cache.length
        got = call(x, cache)
        want = layer(x, twin)
        assert cache.length == l0 + 1 == twin.length, (what, i)
        for a, b in zip(got, want):
            assert torch.equal(a, b), (what, i)


def inputs(g, bsz, n):
    return [torch.randn(bsz, 1, 4096, generator=g, device="cuda", dtype=torch.float16) for _ in range(n)]


@pytest.mark.parametrize("bsz_b", [2, 3])
def test_new_cache_object_behind_a_captured_wrapper(bsz_b):
    """Serving code builds a cache per generation run. Cache A is dropped with a plain ``del`` (no gc.collect(): the sequence in which the next
    object of the class inherits A's id(), tests/test_graphed_cpu.py) and cache B — more pages, in the second case another batch size — takes
    its place behind the same wrapper. B must get a graph of its own over ITS pages: the graph captured for A holds A's (freed) addresses."""
    import flatquant_amd.deploy as deploy
    with torch.no_grad():
        layer, new_cache, g = build(2, page=16, prompt=21, max_len=64, seed=11)
        gd = deploy.GraphedDecode(layer.forward)
        a, twin = new_cache(), new_cache()
        run_against_twin(gd, layer, a, twin, inputs(g, 2, 6), "A")         # two warm-ups, the capture, three replays
        assert_same_rows(a, twin)
        assert gd.captures == 1 and gd.eager_calls == 2 and gd.replays == 4
        del a, twin
        b, twin_b = new_cache(bsz=bsz_b, max_len=256), new_cache(bsz=bsz_b, max_len=256)
        run_against_twin(gd, layer, b, twin_b, inputs(g, bsz_b, 8), "B")
        assert_same_rows(b, twin_b)
        assert b.length == 29
        assert gd.captures == 2 and gd.eager_calls == 4 and gd.replays == 4 + 6     # two warm-ups per cache, no more
        assert len(gd._entries) == 1                                        # A's graph went with A


def test_six_generations_each_with_a_fresh_cache():
    """A cache per generation run, six runs behind one wrapper: every run right, one capture per cache, at most one live graph, and the device
    memory in use after the last cache is dropped equal (within one cache's pages) to what it was after the first was."""
    import flatquant_amd.deploy as deploy
    with torch.no_grad():
        layer, new_cache, g = build(2, page=16, prompt=21, max_len=64, seed=12)
        gd = deploy.GraphedDecode(layer.forward)
        xs = inputs(g, 2, 6)
        after = []
        for gen in range(6):
            cache, twin = new_cache(), new_cache()
            one_cache = cache.pages.nbytes + cache.scales.nbytes
            run_against_twin(gd, layer, cache, twin, xs, gen)
            assert_same_rows(cache, twin)
            assert gd.captures == gen + 1 and gd.eager_calls == 2 * (gen + 1)
            del cache, twin
            assert len(gd._entries) <= 1
            gc.collect()
            torch.cuda.synchronize()
            assert len(gd._entries) == 0 and len(gd._seen) == 0 and len(gd._logs) == 0 and len(gd._watched) == 0
            after.append(torch.cuda.memory_allocated())
        print(f"memory_allocated after each generation's drop: {after}, one cache: {one_cache} bytes")
        assert after[-1] - after[0] <= one_cache, (after, one_cache)


def test_two_live_caches_alternate_behind_one_wrapper():
    """A, B, A, B, ... with different lengths: each keeps its own graph, neither is replayed for the other (a fix that remembers "the last
    cache seen" would re-capture on every call, or worse)."""
    import flatquant_amd.deploy as deploy
    with torch.no_grad():
        layer, new_cache, g = build(2, page=16, prompt=21, max_len=64, seed=13)
        gd = deploy.GraphedDecode(layer.forward)
        a, ta = new_cache(), new_cache()
        b, tb = new_cache(prompt=9), new_cache(prompt=9)
        for i, x in enumerate(inputs(g, 2, 14)):
            cache, twin = (a, ta) if i % 2 == 0 else (b, tb)
            run_against_twin(gd, layer, cache, twin, [x], i)
        assert a.length == 28 and b.length == 16
        assert_same_rows(a, ta), assert_same_rows(b, tb)
        assert gd.captures == 2 and gd.eager_calls == 4 and gd.replays == 10 and len(gd._entries) == 2


class Adapter:
    """what an integration may put around the cache: holds it as ``.inner`` and forwards ``update``"""

    def __init__(self, inner):
        self.inner = inner

    def update(self, *a, **k):
        return self.inner.update(*a, **k)


class Opaque:
    """a cache behind something the wrapper cannot see through"""

    def __init__(self, hidden):
        self._hidden = hidden

    def update(self, *a, **k):
        return self._hidden.update(*a, **k)


def test_wrapped_cache():
    """The cache one level inside an adapter (``.inner``) is recognised: the step is captured and replayed like a bare cache's (documented in
    deploy/graphed.py) — the length advances by one per step and the rows land in consecutive slots. Behind an object the wrapper cannot
    see through the step is NOT captured (an ``update`` attribute on an unrecognised argument) and stays eager — and right."""
    import flatquant_amd.deploy as deploy
    with torch.no_grad():
        layer, new_cache, g = build(2, page=16, prompt=21, max_len=64, seed=14)
        xs = inputs(g, 2, 8)
        gd = deploy.GraphedDecode(layer.forward)
        cache, twin = new_cache(), new_cache()
        ad = Adapter(cache)
        run_against_twin(lambda x, c: gd(x, ad), layer, cache, twin, xs, "adapter")
        assert cache.length == 29
        assert_same_rows(cache, twin)
        assert gd.captures == 1 and gd.eager_calls == 2 and gd.replays == 6
        gd2 = deploy.GraphedDecode(layer.forward)
        cache2, twin2 = new_cache(), new_cache()
        op = Opaque(cache2)
        run_against_twin(lambda x, c: gd2(x, op), layer, cache2, twin2, xs, "opaque")
        assert_same_rows(cache2, twin2)
        assert gd2.captures == 0 and gd2.replays == 0 and len(gd2._entries) == 0
        # a cache the wrapper never sees as an argument at all (an attribute of some object): the capture reaches update(), which refuses; the
        # signature is blocked and every step runs eagerly
        class Held:
            def __init__(self, kv):
                self.kv = kv
        gd3 = deploy.GraphedDecode(lambda x, h: layer(x, h.kv))
        cache3, twin3 = new_cache(), new_cache()
        held = Held(cache3)
        run_against_twin(lambda x, c: gd3(x, held), layer, cache3, twin3, xs, "held")
        assert_same_rows(cache3, twin3)
        assert gd3.captures == 0 and gd3.replays == 0 and len(gd3._blocked) == 1


def test_manual_capture_of_update_is_refused():
    """torch.cuda.graph around a bare cache.update(): the host step (length + 1, the index tensors' fills) would run ONCE and be frozen into
    the graph. update() raises before it does or launches anything; the cache is untouched and goes on working."""
    with torch.no_grad():
        layer, new_cache, g = build(2, page=16, prompt=21, max_len=64, seed=15)
        cache, twin = new_cache(), new_cache()
        kw = {"trans_matrix_k": layer.self_attn.tk, "trans_matrix_k_inv_t": layer.self_attn.tk}
        k = torch.randn(2, 1, 8, 128, generator=g, device="cuda").half()
        v = torch.randn(2, 1, 8, 128, generator=g, device="cuda").half()
        q = torch.randn(2, 1, 32, 128, generator=g, device="cuda").half()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="stream capture"):
            with torch.cuda.graph(graph, stream=s):
                k2 = k + 0                                          # (one node: the capture that is abandoned is not an empty one)
                cache.update(k2, v, 0, kw)
        torch.cuda.synchronize()
        assert not torch.cuda.is_current_stream_capturing()
        assert cache.length == 21 and cache._pending is None
        for _ in range(2):
            assert torch.equal(cache.update(k, v, 0, kw)(q), twin.update(k, v, 0, kw)(q))
        assert cache.length == 23
        assert_same_rows(cache, twin)


# -- (f) a graph replayed far past its capture length, against fp64 -----------------------------------------------------------------------
LONG_TO, LONG_PROMPT, LONG_CHECKS = 700, 21, {24, 255, 256, 257, 511, 512, 513, 700} | set(range(24, 700, 37))


def stored_rows_f64(cache, which):
    """[bsz, length, cache heads, head_dim] float64: what the cache holds (``which`` 0 keys, 1 values), read from its own pages —
    INT4 rows de-quantised n * scale - zero as the decode kernel evaluates it (tests/test_gpu_kvcache.py deq32), here in float64."""
    bsz, n_pg = cache.batch_size, cache.page_cnt_from_length(cache.length)
    pages, scales = cache.pages[:n_pg * bsz, 0, which], cache.scales[:n_pg * bsz, 0, which]      # [n_pg * bsz, heads, page, ..]: page p of request b at p * bsz + b
    heads = pages.shape[1]
    if cache.disable_quant:
        x = pages.double()
    else:
        n = torch.stack((pages & 15, pages >> 4), dim=-1).reshape(*pages.shape[:-1], -1).double()
        par = scales.double()
        x = n * par[..., 0:1] - par[..., 1:2]
    x = x.reshape(n_pg, bsz, heads, cache.page_size, -1).permute(1, 0, 3, 2, 4).reshape(bsz, n_pg * cache.page_size, heads, -1)
    return x[:, :cache.length]


def dense_f64(K, V, q_rot):
    """dense attention in float64 over stored rows K, V [bsz, length, heads, hd] for the (already transformed) query [bsz, heads, hd]"""
    x = torch.einsum("bhd,bshd->bhs", q_rot.double(), K) / q_rot.shape[-1] ** 0.5
    return torch.einsum("bhs,bshd->bhd", torch.softmax(x, dim=-1), V)


def row_err(o, ref):
    """largest deviation of a [bsz, heads, hd] output from ``ref``, per (request, head) row as a fraction of that row's maximum"""
    return ((o.reshape(ref.shape).double() - ref).abs().amax(-1) / ref.abs().amax(-1)).max().item()


def k_transform(hd, seed):
    """A learned K transform as FlatQuant has them: a well-conditioned dense matrix (they are initialised orthogonal and trained from there) —
    a random orthogonal matrix with its columns scaled by 0.5 .. 2, and its exact inverse-transpose, both rounded to fp16.
    Why not a Gaussian matrix and its inverse, as tests/test_gpu_kvcache.py takes for a few steps: the launch rounds q' = q . tk_inv_t to fp16
    (kv_cache.py:139-140 does), and so must the reference — but WHICH fp16 value an element a hair from a rounding tie gets depends on the order
    of the fp32 additions, the launch's or torch.matmul's. With a Gaussian 128 x 128 matrix (condition number 1258, |q'| up to 480, one fp16 ulp
    of an element up to 0.25) one such element moves a whole score. Measured on the MI355X at (INT4, bsz 3, length 246): the fp64 reference
    with torch's q' and the fp64 reference with the correctly rounded q' differ by 5.8e-3 of the row maximum from each other — the launch was
    5.0e-4 from the second and 5.7e-3 from the first, and 4.4e-4 from the first when handed torch's q' itself. A reference that is ambiguous
    beyond the 3e-3 bar cannot hold a launch to it. With this matrix |q'| stays below ~10, an ulp is 2^-7 at most, a flipped element moves a
    score by < 4e-3 and the output by well under 1e-3: the reference is defined to a fraction of the bar (the test records by how much)."""
    gen = torch.Generator().manual_seed(seed)
    qo, _ = torch.linalg.qr(torch.randn(hd, hd, generator=gen, dtype=torch.float64))
    tk = (qo * (torch.rand(hd, generator=gen, dtype=torch.float64) * 1.5 + 0.5)).half()
    return tk.cuda(), torch.linalg.inv(tk.double()).T.contiguous().half().cuda()


@pytest.mark.parametrize("bsz", [1, 3])
@pytest.mark.parametrize("trans", ["matmul", "had"])
@pytest.mark.parametrize("mode", ["int4_fused_append", "int4_two_launches", "fp16_pages"])
def test_graph_replayed_far_past_its_capture_length(ops, mode, trans, bsz):
    """The attention-only step ``cache.update(k, v, 0, kw)(q)`` (no GEMM to mask an error) captured at length 24 and replayed to 700, page 16,
    32 query heads over 8 KV heads, no page growth (max_seq_len 1024). The page count changes 42 times under the graph, the row range of every
    wave moves, and the eager twin switches to the split launch at 512 (fq_kv_decode_splits: seq_hint / 256) while the graph keeps the unsplit
    one it was captured with (``seq_hint`` is a launch argument frozen at capture). At every step: the row appended equals the twin's
    bit for bit (the append does not depend on splits); the outputs are bit-equal while length < 512 (both unsplit; ``wide`` in
    fq_launch_kv_decode depends on the split count only) and within 1e-3 of the output's maximum from 512 on (the bar of
    test_split_decode_equals_the_unsplit_launch: same result up to the order of fp32 additions). At LONG_CHECKS both outputs are compared
    with dense float64 attention over the cache's own stored rows: 3e-3 of the row maximum, the bar tests/test_gpu_kvcache.py asserts for these
    launches. The largest errors are printed, and appended to $FLATQUANT_REPORT_DIR/graphed_long_replay.txt when that variable names a directory (a run's
    record is kept as profiles/r08_graphed_long_replay.txt)."""
    import flatquant_amd.deploy as deploy
    import flatquant_amd.deploy.transformers as T
    heads, kv_heads, hd, page = 32, 8, 128, 16
    g = torch.Generator(device="cuda").manual_seed(100 + bsz)
    tk, tk_inv_t = k_transform(hd, 7)
    kw = {"trans_matrix_k": tk, "trans_matrix_k_inv_t": tk_inv_t}
    opts = {"int4_fused_append": dict(fuse_append=True), "int4_two_launches": dict(fuse_append=False), "fp16_pages": dict(disable_quant=True)}[mode]

    def new():
        return T.MultiLayerPagedKVCache4Bit(bsz, page, 1024, torch.device("cuda"), 1, heads, hd, trans=trans, group_size=heads // kv_heads, **opts)

    def fn(q, k, v, cache):
        return cache.update(k, v, 0, kw)(q)

    def rot(q):     # the query as the launch transforms it
        q = q.reshape(bsz, heads, hd)
        return torch.matmul(q, tk_inv_t) if trans == "matmul" else ops.hadamard(q.contiguous())

    with torch.no_grad():
        cache, twin = new(), new()
        k0 = torch.randn(bsz, LONG_PROMPT, kv_heads, hd, generator=g, device="cuda").half()
        v0 = torch.randn(bsz, LONG_PROMPT, kv_heads, hd, generator=g, device="cuda").half()
        cache.update(k0, v0, 0, kw), twin.update(k0, v0, 0, kw)
        gd = deploy.GraphedDecode(fn)
        gen0 = cache.generation
        steps = LONG_TO - LONG_PROMPT
        zero = torch.zeros((), device="cuda")
        bad_rows, bad_out, far = zero.clone(), zero.clone(), zero.clone()      # accumulated on the device: one read-back per check point
        worst = {"graph": 0.0, "eager": 0.0, "graph_vs_eager_from_512": 0.0, "reference": 0.0}
        for i in range(steps):
            k = torch.randn(bsz, 1, kv_heads, hd, generator=g, device="cuda").half()
            v = torch.randn(bsz, 1, kv_heads, hd, generator=g, device="cuda").half()
            q = torch.randn(bsz, 1, heads, hd, generator=g, device="cuda").half()
            got = gd(q, k, v, cache)
            want = fn(q, k, v, twin)
            n = cache.length
            assert n == twin.length == LONG_PROMPT + i + 1
            pg, slot = (n - 1) // page, (n - 1) % page
            sl = slice(pg * bsz, (pg + 1) * bsz)                                  # the step's own row, every request
            bad_rows += (cache._pages[sl, :, :, :, slot] != twin._pages[sl, :, :, :, slot]).sum()
            if not cache.disable_quant:
                bad_rows += (cache._scales[sl, :, :, :, slot].view(torch.int16) != twin._scales[sl, :, :, :, slot].view(torch.int16)).sum()
            if n < 512:
                bad_out += (got.view(torch.int16) != want.view(torch.int16)).sum()
            else:
                far = torch.maximum(far, (got.float() - want.float()).abs().amax() / want.float().abs().amax())
            if n in LONG_CHECKS:
                assert bad_rows.item() == 0, f"appended rows differ from the eager twin's at or before length {n}"
                assert bad_out.item() == 0, f"replayed output differs from the eager step's at or before length {n} (< 512: both unsplit)"
                worst["graph_vs_eager_from_512"] = max(worst["graph_vs_eager_from_512"], far.item())
                assert far.item() <= 1e-3, (n, far.item())
                assert_same_rows(cache, twin)
                K, V = stored_rows_f64(cache, 0), stored_rows_f64(cache, 1)
                ref = dense_f64(K, V, rot(q))
                if trans == "matmul":       # how well the reference itself is defined: against the one over the correctly rounded q' (k_transform)
                    exact = (q.reshape(bsz, heads, hd).double() @ tk_inv_t.double()).half()
                    worst["reference"] = max(worst["reference"], row_err(dense_f64(K, V, exact), ref))
                for name, o in (("graph", got), ("eager", want)):
                    err = row_err(o, ref)
                    worst[name] = max(worst[name], err)
                    print(f"{mode} {trans} bsz {bsz} length {n}: {name} vs fp64 {err:.3e}")
                    assert err <= 3e-3, (name, n, err)
        assert cache.length == LONG_TO and cache.generation == gen0
        assert gd.captures == 1 and gd.eager_calls == 2 and gd.replays == steps - 2
    line = (f"{mode:18s} {trans:6s} bsz {bsz}  max err vs fp64 (of the row maximum, bar 3e-3): graph {worst['graph']:.3e}  eager {worst['eager']:.3e}"
            f"   graph vs eager, length >= 512 (of the output maximum, bar 1e-3): {worst['graph_vs_eager_from_512']:.3e}"
            f"   the fp64 reference against itself over the correctly rounded q': {worst['reference']:.3e}")
    print(line)
    out = os.environ.get("FLATQUANT_REPORT_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "graphed_long_replay.txt"), "a") as fh:
            fh.write(line + "\n")


# -- (g) Linear4bit's operand images after an in-place reload -----------------------------------------------------------------------------
def _lin_parts(g, n_out, k_in):
    return (torch.randint(0, 256, (n_out, k_in // 2), generator=g, device="cuda", dtype=torch.uint8),
            torch.rand(n_out, 1, generator=g, device="cuda") * 0.02 + 0.005, torch.randn(n_out, generator=g, device="cuda").half())


def _lin_inputs(deploy, g, lin, k_in):
    ps = []
    for rows in (4, lin.fp6_transient_rows + 3):                        # the decode image's route, the FP6 image's route
        ps.append(deploy.PackedQuantizedTensor(torch.randint(0, 256, (1, rows, k_in // 2), generator=g, device="cuda", dtype=torch.uint8),
                                               (torch.rand(1, 1, rows, generator=g, device="cuda") * 0.05 + 0.001).half()))
    return ps


def _lin_ref(ops, p, w, sw, b):
    return ops.int4_linear(p.quantized_x.reshape(-1, p.quantized_x.shape[-1]), p.scales_x.reshape(-1), w, sw.reshape(-1).half(), b.half())


@pytest.mark.parametrize("how", ["inference_mode_copy", "data_copy", "load_state_dict"])
def test_linear4bit_images_follow_an_in_place_reload(ops, how):
    """The decode image, the FP6 image and the fp16 scales of a Linear4bit are derived from its buffers. A reload that no version counter
    shows — copy_ into INFERENCE tensors (ops.ver is 0 for them), a write through ``.data`` — is followed by ops.invalidate_caches(), the
    documented protocol; load_state_dict calls it itself (the module's post hook). After it both call sizes compute with the NEW weights:
    the bits of ops.int4_linear on the new tensors."""
    import flatquant_amd.deploy as deploy
    n_out, k_in = 384, 512
    g = torch.Generator(device="cuda").manual_seed(31)
    built_under_inference = how != "data_copy"
    with torch.inference_mode(built_under_inference):
        lin = deploy.nn.Linear4bit(k_in, n_out, bias=True).cuda()
        lin.fp6_image, lin.fp6_min_out_features = True, 0
        w0, s0, b0 = _lin_parts(g, n_out, k_in)
        lin.weight.copy_(w0), lin.weight_scales.copy_(s0), lin.bias.copy_(b0)
        if built_under_inference:
            assert lin.weight.is_inference() and ops.ver(lin.weight) == 0
        ps = _lin_inputs(deploy, g, lin, k_in)
        old = [lin(p).clone() for p in ps]
        for y, p in zip(old, ps):
            assert torch.equal(y.reshape(-1, n_out), _lin_ref(ops, p, w0, s0, b0))
        assert lin.__dict__.get("_dimg") is not None and lin._weight_image() is not None      # both images exist: the routes under test ran
        w1, s1, b1 = _lin_parts(g, n_out, k_in)
        if how == "inference_mode_copy":
            lin.weight.copy_(w1), lin.weight_scales.copy_(s1), lin.bias.copy_(b1)
            ops.invalidate_caches()
        elif how == "data_copy":
            lin.weight.data.copy_(w1), lin.weight_scales.data.copy_(s1), lin.bias.data.copy_(b1)
            ops.invalidate_caches()
        else:
            lin.load_state_dict({"weight": w1, "weight_scales": s1, "bias": b1})
        for y0, p in zip(old, ps):
            y = lin(p)
            assert torch.equal(y.reshape(-1, n_out), _lin_ref(ops, p, w1, s1, b1)), p.quantized_x.shape
            assert not torch.equal(y, y0)


def test_graphed_linear4bit_is_recaptured_with_the_new_images_after_a_reload(ops):
    """the same reload with the module inside a GraphedDecode: the epoch change makes the entry stale, one eager call re-derives the images,
    the re-captured graph computes with the new weights"""
    import flatquant_amd.deploy as deploy
    n_out, k_in = 384, 512
    g = torch.Generator(device="cuda").manual_seed(32)
    with torch.inference_mode():
        lin = deploy.nn.Linear4bit(k_in, n_out, bias=True).cuda()
        w0, s0, b0 = _lin_parts(g, n_out, k_in)
        lin.weight.copy_(w0), lin.weight_scales.copy_(s0), lin.bias.copy_(b0)
        gd = deploy.GraphedDecode(lambda q, s: lin(deploy.PackedQuantizedTensor(q, s)))
        ps = [_lin_inputs(deploy, g, lin, k_in)[0] for _ in range(5)]
        for p in ps[:4]:
            assert torch.equal(gd(p.quantized_x, p.scales_x).reshape(-1, n_out), _lin_ref(ops, p, w0, s0, b0))
        assert gd.captures == 1 and gd.replays == 2
        w1, s1, b1 = _lin_parts(g, n_out, k_in)
        lin.weight.copy_(w1), lin.weight_scales.copy_(s1), lin.bias.copy_(b1)
        ops.invalidate_caches()
        for p in ps:
            assert torch.equal(gd(p.quantized_x, p.scales_x).reshape(-1, n_out), _lin_ref(ops, p, w1, s1, b1))
        assert gd.captures == 2 and gd.eager_calls == 3 and gd.replays == 2 + 4
