"""Rotary position embedding inside the decode step's launches (round 8): the standalone launch (ops.rope, fq_rope_f16), the decode launch that
rotates its own queries and new K row (ops.kv_decode_append(rope=...), fq_kv_decode_append_rope_i4), the cache's ``rotate`` option on every
route, the captured step, and the memory contract of the two launch families.

What is asserted is bit identity throughout: ops.rope against torch's fp16 expression ``(x * cos) + (rotate_half(x) * sin)`` on the device and
against tests/rope_ref.py (three fp16 roundings; a fused multiply-add would differ in about three elements of ten, tests/test_rope_cpu.py);
the fused launch against ops.rope followed by the launch without rope (same geometry, so not even the order of additions differs); the
cache with ``rotate`` against caller-side torch rotation and the cache without it."""
import pytest
import torch

from tests import guards
from tests.conftest import same_bits
from tests.rope_ref import llama3_tables, rope_ref, rope_torch
from tests.test_gpu_bounds import IDX_PADS, addressed, drive, paged, rnd
from tests.test_gpu_kv_decode_append import _cache

pytestmark = pytest.mark.gpu
F16 = torch.float16


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


def tables(shape, seed):
    """random cos / sin in [-1, 1] whose two halves differ (the tables are taken as given)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1).half().cuda(), (torch.rand(*shape, generator=g) * 2 - 1).half().cuda()


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == F16 and bool(torch.equal(a.view(torch.int16), b.view(torch.int16)))


# ------------------------------------------------------------------------------------------------ ops.rope

@pytest.mark.parametrize("tokens", [1, 7, 2051])
@pytest.mark.parametrize("hq,hk", [(32, 8), (8, 8)])
@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("which", ["both", "q", "k"])
@pytest.mark.parametrize("in_place", [False, True])
def test_rope_is_the_torch_expression_bit_for_bit(ops, tokens, hq, hk, hd, which, in_place):
    q = rnd((tokens, hq, hd), tokens + hq, F16, 1.5) if which != "k" else None
    k = rnd((tokens, hk, hd), tokens + hk + 1, F16, 1.5) if which != "q" else None
    if tokens == 2051:
        pos = torch.arange(8191 - tokens + 1, 8192)
        cos, sin = (t.cuda() for t in llama3_tables(pos, hd))
    else:
        cos, sin = tables((tokens, hd), tokens + hd)
    want = [None if t is None else rope_torch(t, cos, sin) for t in (q, k)]
    ref = [None if t is None else rope_ref(t.cpu(), cos.cpu(), sin.cpu()) for t in (q, k)]
    src = [None if t is None else t.clone() for t in (q, k)]
    got = ops.rope(src[0], src[1], cos, sin, out=(src[0], src[1]) if in_place else None)
    for g, w, r, s, x in zip(got, want, ref, src, (q, k)):
        if x is None:
            assert g is None
            continue
        assert (g.data_ptr() == s.data_ptr()) == in_place
        assert bits_equal(g, w)
        assert same_bits(g.cpu().numpy(), r.numpy())
        if not in_place:
            assert bits_equal(s, x)                 # the input is left alone


def test_rope_leading_dimensions_and_the_functional_drop_in(ops):
    from flatquant_amd.deploy import functional
    bsz, seq, hq, hk, hd = 3, 5, 8, 2, 128
    q, k = rnd((bsz, seq, hq, hd), 1), rnd((bsz, seq, hk, hd), 2)
    cos, sin = tables((bsz, seq, hd), 3)
    qe, ke = functional.apply_rotary_pos_emb(q, k, cos, sin)
    assert bits_equal(qe, rope_torch(q, cos, sin)) and bits_equal(ke, rope_torch(k, cos, sin))
    qe2, ke2 = ops.rope(q, k, cos, sin)
    assert bits_equal(qe2, qe) and bits_equal(ke2, ke)
    # tables shared by the requests ([1, seq, head_dim], as HF builds them for equal position_ids) and fp32 tables
    qe3, ke3 = functional.apply_rotary_pos_emb(q, k, cos[:1].float(), sin[:1].float(), position_ids=None, unsqueeze_dim=2)
    assert bits_equal(qe3, rope_torch(q, cos[:1].expand(bsz, seq, hd), sin[:1].expand(bsz, seq, hd)))
    assert bits_equal(ke3, rope_torch(k, cos[:1].expand(bsz, seq, hd), sin[:1].expand(bsz, seq, hd)))
    with pytest.raises(NotImplementedError):
        functional.apply_rotary_pos_emb(q, k, cos, sin, unsqueeze_dim=1)
    with pytest.raises(ValueError):
        ops.rope(None, None, cos, sin)
    with pytest.raises(ValueError):
        ops.rope(q, k[:, :4].contiguous(), cos, sin)
    from flatquant_amd import _lib
    with pytest.raises(_lib.FqError) as e:
        ops.rope(rnd((4, 2, 96), 1), None, *tables((4, 96), 2))
    assert e.value.code == _lib.FQ_EUNSUPPORTED


# ------------------------------------------------------------------------------------------------ the fused launch

FUSED = [
    # bsz, lens, src_heads, copies per source head in the cache, query heads per cache head, page, read_one_copy
    (1, [2048], 8, 4, 1, 2048, False),                                # one request: the split launch
    (1, [2048], 8, 4, 1, 2048, True),                                 # ... reading one copy of the replicated layout
    (1, [2049], 8, 1, 4, 2048, False),                                # ... the shared layout, the new row first on a fresh page
    (64, [300 + 7 * i for i in range(64)], 8, 1, 4, 64, False),       # 64 requests, shared layout: unsplit, one workgroup per four query heads
    (64, [1024] * 64, 8, 4, 1, 1024, True),                           # ... the replicated layout read one copy per group (the same merged launch)
    (40, [70 + i for i in range(40)], 8, 1, 2, 16, False),            # shared layout, two query heads per workgroup
    (6, [17, 32, 33, 48, 1, 16], 2, 2, 1, 16, True),                  # the new row in the FIRST (17, 33, 1) and the LAST (32, 48, 16) slot of a page
    (6, [17, 32, 33, 48, 1, 16], 4, 1, 4, 16, False),                 # ... shared layout, four query heads per cache head, split
    (33, [16 * (i % 3 + 1) + (i % 2) for i in range(33)], 8, 1, 4, 16, False),   # ... the merged launch (264 pairs), first / last slots
    (16, [2048] * 16, 8, 4, 1, 2048, False),                          # 512 pairs head by head: unsplit, four waves
]


@pytest.mark.parametrize("bsz,lens,src_heads,copies,q_group,page,one_copy", FUSED)
@pytest.mark.parametrize("trans,q_trans", [(True, True), (False, False), (True, False)])
@pytest.mark.parametrize("transpose_out", [False, True])
def test_fused_rope_equals_rope_then_decode_append(ops, bsz, lens, src_heads, copies, q_group, page, one_copy, trans, q_trans, transpose_out):
    g = torch.Generator(device="cuda").manual_seed(bsz * 1000 + lens[0] + src_heads)
    hd, layer = 128, 1
    cache_heads, heads = src_heads * copies, src_heads * copies * q_group
    data, param, indptr, indices, last = _cache(g, bsz, lens, cache_heads, page)
    k = (torch.randn(bsz, src_heads, hd, generator=g, device="cuda") * 2).half()
    v = (torch.randn(bsz, src_heads, hd, generator=g, device="cuda") * 2).half()
    T = (torch.randn(hd, hd, generator=g, device="cuda") / hd ** 0.5).half() if trans else None
    qt = (torch.randn(hd, hd, generator=g, device="cuda") / hd ** 0.5).half() if q_trans else None
    q = (torch.randn(bsz, heads, hd, generator=g, device="cuda") * 0.5).half()
    cos, sin = tables((bsz, hd), bsz + lens[0])
    hint = max(lens)
    for split in (True, False):
        d1, p1 = data.clone(), param.clone()
        qr, kr = ops.rope(q, k, cos, sin)
        assert bits_equal(qr, rope_torch(q, cos, sin)) and bits_equal(kr, rope_torch(k, cos, sin))
        o1 = ops.kv_decode_append(qr, kr, v, T, d1, p1, indptr, indices, last, layer, qt, transpose_out, seq_hint=hint, split=split, read_one_copy=one_copy)
        d2, p2 = data.clone(), param.clone()
        o2 = ops.kv_decode_append(q, k, v, T, d2, p2, indptr, indices, last, layer, qt, transpose_out, seq_hint=hint, split=split, read_one_copy=one_copy,
                                  rope=(cos, sin))
        assert not torch.equal(d1, data)                       # (the step did append something)
        assert torch.equal(d2, d1), "cache bytes"
        assert torch.equal(p2.view(torch.int16), p1.view(torch.int16)), "cache parameters"
        assert bits_equal(o2, o1), "attention output"
        assert bool(torch.isfinite(o2.float()).all())
        # ... and the rotation does matter here: the launch without the tables leaves another row and another output
        d3, p3 = data.clone(), param.clone()
        o3 = ops.kv_decode_append(q, k, v, T, d3, p3, indptr, indices, last, layer, qt, transpose_out, seq_hint=hint, split=split, read_one_copy=one_copy)
        assert not torch.equal(d3, d1) and not bits_equal(o3, o1)


def test_fused_rope_refuses_bad_tables(ops):
    g = torch.Generator(device="cuda").manual_seed(3)
    data, param, indptr, indices, last = _cache(g, 2, [20, 21], 2, 16)
    q, k = rnd((2, 2, 128), 1), rnd((2, 2, 128), 2)
    cos, sin = tables((2, 128), 1)
    with pytest.raises(ValueError):
        ops.kv_decode_append(q, k, k, None, data, param, indptr, indices, last, 0, rope=(cos[:1].contiguous(), sin))
    with pytest.raises(TypeError):
        ops.kv_decode_append(q, k, k, None, data, param, indptr, indices, last, 0, rope=(cos.float(), sin))


# ------------------------------------------------------------------------------------------------ the cache class

def _k_transform(hd, seed):
    gen = torch.Generator().manual_seed(seed)
    qo, _ = torch.linalg.qr(torch.randn(hd, hd, generator=gen, dtype=torch.float64))
    tk = (qo * (torch.rand(hd, generator=gen, dtype=torch.float64) * 1.5 + 0.5)).half()
    return tk.cuda(), torch.linalg.inv(tk.double()).T.contiguous().half().cuda()


ROUTES = {
    # name: (constructor options, trans, steps as tokens added per request, ragged mask, FUSE_APPEND_MAX_PAIRS for the test or None)
    # ("four_heads_*": four requests = 32 (request, KV head) pairs, the launch that serves four query heads per workgroup)
    "fused": (dict(), "matmul", [1, 1, 1], False, None),
    "fused_shared_heads": (dict(share_kv_heads=True), "matmul", [1, 1, 1], False, None),
    "fused_no_transform": (dict(), "none", [1, 1], False, None),
    "fuse_append_off": (dict(fuse_append=False), "matmul", [1, 1, 1], False, None),
    "too_many_pairs": (dict(), "matmul", [1, 1], False, 8),
    "hadamard": (dict(), "had", [1, 1, 1], False, None),
    "fp16_pages": (dict(disable_quant=True), "matmul", [1, 1], False, None),
    "extend": (dict(), "matmul", [1, 3, 1, 4], False, None),
    "ragged_mask": (dict(), "matmul", [1, 1, 1], True, None),
    "four_heads_fused": (dict(), "matmul", [1, 1, 1], False, None),
    "four_heads_beyond_one_workgroup_per_cu": (dict(share_kv_heads=True), "matmul", [1, 1, 1], False, None),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("call_closure", [True, False])
def test_cache_rotate_equals_caller_side_rotation(ops, monkeypatch, route, call_closure):
    """``cache_kwargs["rotate"]`` against transformers' expression applied by the caller and the cache without the key: the states the prompt
    call returns, every step's output, and in the end the pages and the scales, byte for byte. ``call_closure`` False: the closure of the
    middle steps is never called, so their rows reach the cache through ``_flush_pending`` (or were appended by ``update`` already)."""
    import flatquant_amd.deploy.transformers as T
    from flatquant_amd.deploy.transformers import kv_cache as kvc
    opts, trans, steps, ragged, bound = ROUTES[route]
    if bound is not None:
        monkeypatch.setattr(kvc, "FUSE_APPEND_MAX_PAIRS", bound)
    bsz, heads, kv_heads, hd, page, prompt = 4 if route.startswith("four_heads") else 3, 32, 8, 128, 16, 13
    if route == "four_heads_beyond_one_workgroup_per_cu":
        monkeypatch.setattr(kvc, "ROPE_FUSE_MAX_FOUR_HEAD_WGS", 16)       # (32 such workgroups here)
    tk, tk_inv_t = _k_transform(hd, 7)
    base_kw = {"trans_matrix_k": tk, "trans_matrix_k_inv_t": tk_inv_t}
    launches = []
    real_fused, real_rope = ops.kv_decode_append, ops.rope
    monkeypatch.setattr(ops, "kv_decode_append", lambda *a, **k: (launches.append("fused_rope" if k.get("rope") is not None else "fused"), real_fused(*a, **k))[1])
    monkeypatch.setattr(ops, "rope", lambda *a, **k: (launches.append("rope"), real_rope(*a, **k))[1])

    def run(rotate):
        g = torch.Generator(device="cuda").manual_seed(11)
        cache = T.MultiLayerPagedKVCache4Bit(bsz, page, 64, torch.device("cuda"), 1, heads, hd, trans=trans, group_size=heads // kv_heads, **opts)
        cache._pages.fill_(0x11 if not cache.disable_quant else 0.5), cache._scales.fill_(0.25)       # (torch.empty: equal bytes wherever nothing is appended)
        valid = [prompt, prompt - 4, prompt - 9] if ragged else [prompt] * bsz
        mask = torch.zeros(bsz, prompt, dtype=torch.int64, device="cuda")
        for i, n in enumerate(valid):
            mask[i, prompt - n:] = 1
        outs, pos = [], 0

        def kw_for(added):
            nonlocal pos
            p = torch.arange(pos, pos + added)
            pos += added
            cos, sin = (t.cuda()[None].expand(bsz, added, hd).contiguous() for t in llama3_tables(p * 37 + 5, hd))
            cos = cos + (torch.arange(bsz, device="cuda")[:, None, None] * 0.01).half()               # (a different row per request)
            kw = dict(base_kw, cos=cos, sin=sin)                                                      # (the reference passes them either way)
            if ragged:
                kw["attention_mask"] = mask
            if rotate:
                kw["rotate"] = True
            return kw, cos, sin

        kw, cos, sin = kw_for(prompt)
        k = torch.randn(bsz, prompt, kv_heads, hd, generator=g, device="cuda").half()
        v = torch.randn(bsz, prompt, kv_heads, hd, generator=g, device="cuda").half()
        ks, vs = cache.update(k if rotate else rope_torch(k, cos, sin), v, 0, kw)
        outs += [ks, vs]
        for si, added in enumerate(steps):
            if ragged:
                mask = torch.cat([mask, torch.ones(bsz, added, dtype=mask.dtype, device="cuda")], dim=1)
            kw, cos, sin = kw_for(added)
            k = torch.randn(bsz, added, kv_heads, hd, generator=g, device="cuda").half()
            v = torch.randn(bsz, added, kv_heads, hd, generator=g, device="cuda").half()
            q = (torch.randn(bsz, added, heads, hd, generator=g, device="cuda") * 0.5).half()
            att = cache.update(k if rotate else rope_torch(k, cos, sin), v, 0, kw)
            if call_closure or si == len(steps) - 1:
                outs.append(att(q if rotate else rope_torch(q, cos, sin)))
        return outs, cache.pages.clone(), cache.scales.clone()

    with torch.no_grad():
        del launches[:]
        got, pages, scales = run(True)
        seen = list(launches)
        del launches[:]
        want, pages_w, scales_w = run(False)
        assert "rope" not in launches and "fused_rope" not in launches       # (the twin rotates with torch)
    assert len(got) == len(want) and len(got) >= 3
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))
        assert bool(torch.isfinite(a.float()).all())
    assert guards.same_raw(pages, pages_w) and guards.same_raw(scales, scales_w)
    # the route that was meant is the route that ran (the prompt's keys always go through ops.rope: one call)
    if route in ("fused", "fused_shared_heads", "fused_no_transform", "four_heads_fused"):
        assert "fused_rope" in seen
        # every closure called: nothing else is rotated by a launch of its own; un-called closures: their rows are rotated by _flush_pending
        assert seen.count("rope") == (1 if call_closure else len(steps))
    else:
        assert ("fused_rope" in seen) == (route == "extend" and call_closure)      # (the one-token steps between the multi-token ones)
        assert seen.count("rope") >= 1 + len(steps)
        if route == "four_heads_beyond_one_workgroup_per_cu":
            assert seen.count("rope") == 1 + len(steps)             # ONE launch per step: q and k together in the closure, or k alone in _flush_pending
        if route in ("hadamard", "ragged_mask", "four_heads_beyond_one_workgroup_per_cu"):
            assert "fused" in seen                                  # the append stays fused, without the rotation


# ------------------------------------------------------------------------------------------------ the captured step

@pytest.mark.parametrize("bsz", [1, 3])
def test_graphed_decode_takes_new_tables_every_step(bsz):
    """20 successive steps of ``cache.update(k, v, 0, {.., cos, sin, rotate})(q)`` behind deploy.GraphedDecode, a different cos / sin row at
    every step, across a page boundary (lengths 11 .. 30, pages of 16): bit-identical to the eager twin's — the tables are inputs of the graph,
    not constants frozen at capture."""
    import flatquant_amd.deploy as deploy
    import flatquant_amd.deploy.transformers as T
    heads, kv_heads, hd, page, prompt = 32, 8, 128, 16, 10
    g = torch.Generator(device="cuda").manual_seed(50 + bsz)
    tk, tk_inv_t = _k_transform(hd, 9)
    kw = {"trans_matrix_k": tk, "trans_matrix_k_inv_t": tk_inv_t}

    def new():
        c = T.MultiLayerPagedKVCache4Bit(bsz, page, 64, torch.device("cuda"), 1, heads, hd, trans="matmul", group_size=heads // kv_heads)
        c._pages.fill_(0x11), c._scales.fill_(0.25)
        return c

    def fn(q, k, v, cos, sin, cache):
        return cache.update(k, v, 0, dict(kw, cos=cos, sin=sin, rotate=True))(q)

    with torch.no_grad():
        cache, twin = new(), new()
        k0 = torch.randn(bsz, prompt, kv_heads, hd, generator=g, device="cuda").half()
        v0 = torch.randn(bsz, prompt, kv_heads, hd, generator=g, device="cuda").half()
        c0, s0 = (t.cuda()[None].expand(bsz, prompt, hd).contiguous() for t in llama3_tables(torch.arange(prompt), hd))
        for c in (cache, twin):
            c.update(k0, v0, 0, dict(kw, cos=c0, sin=s0, rotate=True))
        gd = deploy.GraphedDecode(fn)
        outs = []
        for i in range(20):
            k = torch.randn(bsz, 1, kv_heads, hd, generator=g, device="cuda").half()
            v = torch.randn(bsz, 1, kv_heads, hd, generator=g, device="cuda").half()
            q = (torch.randn(bsz, 1, heads, hd, generator=g, device="cuda") * 0.5).half()
            cos, sin = (t.cuda()[None].expand(bsz, 1, hd).contiguous() for t in llama3_tables(torch.tensor([prompt + 97 * i]), hd))
            got = gd(q, k, v, cos, sin, cache)
            want = fn(q, k, v, cos, sin, twin)
            assert cache.length == twin.length == prompt + i + 1
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), i
            outs.append(got.clone())
        assert guards.same_raw(cache.pages, twin.pages) and guards.same_raw(cache.scales, twin.scales)
        assert cache.length == prompt + 20 and (prompt + 20 - 1) // page > prompt // page      # (a page boundary was crossed)
        # a graph that had frozen the tables of its capture step would have appended other rows: show that the tables matter here
        frozen = new()
        frozen.update(k0, v0, 0, dict(kw, cos=c0, sin=s0, rotate=True))
        frozen.update(k, v, 0, dict(kw, cos=c0[:, :1].contiguous(), sin=s0[:, :1].contiguous(), rotate=True))(q)
        assert not torch.equal(frozen.pages[:bsz, :, :, :, prompt], cache.pages[bsz:2 * bsz, :, :, :, (prompt + 19) % page])


# ------------------------------------------------------------------------------------------------ memory contract

@pytest.mark.parametrize("tokens,hq,hk,hd", [(1, 32, 8, 128), (7, 8, 8, 64), (2051, 32, 8, 128), (2051, 8, 8, 64), (33, 5, 3, 128)])
@pytest.mark.parametrize("which", ["both", "q", "k"])
def test_rope_stays_inside_its_buffers_and_writes_all_of_them(ops, tokens, hq, hk, hd, which):
    q = rnd((tokens, hq, hd), 1) if which != "k" else None
    k = rnd((tokens, hk, hd), 2) if which != "q" else None
    cos, sin = tables((tokens, hd), 3)
    # fresh outputs between poisoned bands, inputs between NaN bands
    want, _, _ = drive(ops, lambda **a: ops.rope(a["q"], a["k"], a["cos"], a["sin"]), dict(q=q, k=k, cos=cos, sin=sin))
    for w, x in zip(want, [t for t in (q, k) if t is not None]):
        assert bits_equal(w, rope_torch(x, cos, sin))
    # in place: the guarded inputs ARE the outputs (their NaN bands must stay NaN, every element must change to the rotated value)
    inout = tuple(n for n, t in (("q", q), ("k", k)) if t is not None)
    want2, _, _ = drive(ops, lambda **a: ops.rope(a["q"], a["k"], a["cos"], a["sin"], out=(a["q"], a["k"])), dict(q=q, k=k, cos=cos, sin=sin), inout=inout)
    for w2, w in zip(want2[:len(want)], want):
        assert bits_equal(w2, w)


@pytest.mark.parametrize("lens,cache_heads,src_heads,q_group,page,one_copy,split", [
    ([1, 300, 37], 4, 4, 1, 16, False, True), ([1, 2048, 16, 17], 8, 2, 1, 16, True, True), ([1, 2048, 16, 17], 8, 2, 1, 16, False, False),
    ([700, 1, 33], 2, 2, 4, 32, False, True),
    ([600, 1, 300, 520], 8, 8, 4, 16, False, True), ([600, 1, 300, 520], 8, 8, 4, 16, False, False), ([90, 1, 33, 520], 8, 8, 2, 32, False, True),
    ([600, 1, 300, 520], 32, 8, 1, 16, True, True)])
@pytest.mark.parametrize("trans,qt,transpose_out", [(False, False, False), (True, True, True)])
def test_fused_rope_writes_one_row_and_its_output(ops, lens, cache_heads, src_heads, q_group, page, one_copy, split, trans, qt, transpose_out):
    """the fused launch between guard bands: o and the cache equal the plain run's, the cache changes in the new token's rows and nowhere else,
    q / k_new / cos / sin (NaN-padded) are read inside their bounds and left as they were"""
    hd, layers, layer = 128, 2, 1
    data, param, indptr, indices, last, used = paged(lens, cache_heads, page, False, hd, layers)
    mask = addressed(used.shape, layers, cache_heads, indptr, indices, last, page, layer, [1] * len(lens))
    data[mask], param[mask] = 0xFF, float("nan")
    bsz = len(lens)
    q = rnd((bsz, cache_heads * q_group, hd), 1, F16, 0.5)
    kn, vn = rnd((bsz, src_heads, hd), 2), rnd((bsz, src_heads, hd), 3)
    cos, sin = tables((bsz, hd), 6)
    tk = rnd((hd, hd), 4, F16, hd ** -0.5) if trans else None
    tq = rnd((hd, hd), 5, F16, hd ** -0.5) if qt else None
    before = {}

    def call(q, kn, vn, tk, data, param, indptr, indices, last, tq, cos, sin):
        before[data.data_ptr()] = (data, data.clone(), param, param.clone(), q, q.clone(), kn, kn.clone())
        return ops.kv_decode_append(q, kn, vn, tk, data, param, indptr, indices, last, layer, tq, transpose_out, seq_hint=max(lens), split=split,
                                    read_one_copy=one_copy, rope=(cos, sin))

    want, _, _ = drive(ops, call, dict(q=q, kn=kn, vn=vn, tk=tk, data=data, param=param, indptr=indptr, indices=indices, last=last, tq=tq, cos=cos, sin=sin),
                       pads=IDX_PADS, inout=("data", "param"))
    assert bool(torch.isfinite(want[0].float()).all()) and len(before) == 3
    for d1, d0, p1, p0, q1, q0, k1, k0 in before.values():
        assert torch.equal(d1[~mask], d0[~mask]) and guards.same_raw(p1[~mask], p0[~mask])
        assert not bool((d1[mask] == 0xFF).all()) and bool(torch.isfinite(p1[mask].float()).all())
        assert bits_equal(q1, q0) and bits_equal(k1, k0)            # the launch rotates in LDS, never in the caller's tensors
    # the launches it replaces leave the same cache and the same output
    d2, p2 = data.clone(), param.clone()
    qr, kr = ops.rope(q, kn, cos, sin)
    o2 = ops.kv_decode_append(qr, kr, vn, tk, d2, p2, indptr, indices, last, layer, tq, transpose_out, seq_hint=max(lens), split=split, read_one_copy=one_copy)
    assert bits_equal(o2, want[0]) and torch.equal(d2, want[1]) and guards.same_raw(p2, want[2])
