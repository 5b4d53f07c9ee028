"""Several new tokens per request over the paged KV cache (fq_kv_batch_extend / ops.kv_batch_extend, round 7): causal attention of a step's
T tokens — token t attends the rows before the step and the step's tokens 0 .. t — against an fp64 dense attention over the de-quantised
cache; causality bit for bit; T = 1 against the decode launch; MultiLayerPagedKVCache4Bit taking T > 1 tokens after the prompt (every
trans / quant / head configuration, with and without a ragged mask); a verify step against the same tokens as sequential decode steps;
capture and replay; repeated split launches; argument errors."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


def _cache(g, lens, cache_heads, page, f16, hd=128, layers=2):
    """a cache whose request b holds lens[b] rows, pages scattered"""
    n_pg = [(n + page - 1) // page for n in lens]
    tot = sum(n_pg)
    if f16:
        data = (torch.randn(tot, layers, 2, cache_heads, page, hd, generator=g, device="cuda") * 1.5).half()
    else:
        data = torch.randint(0, 256, (tot, layers, 2, cache_heads, page, hd // 2), generator=g, device="cuda", dtype=torch.uint8)
    param = torch.stack([torch.rand(tot, layers, 2, cache_heads, page, generator=g, device="cuda") * 0.3 + 0.02,
                         torch.rand(tot, layers, 2, cache_heads, page, generator=g, device="cuda") * 2.0 + 0.1], dim=-1).half()
    indptr = torch.tensor([0] + list(torch.tensor(n_pg).cumsum(0)), dtype=torch.int32, device="cuda")
    indices = torch.randperm(tot, generator=g, device="cuda").to(torch.int32)
    last = torch.tensor([(n - 1) % page + 1 for n in lens], dtype=torch.int32, device="cuda")
    return data, param, indptr, indices, last


def _dense(data, param, indptr, indices, last, layer):
    """-> per request (K, V) [L, cache_heads, hd] fp64, de-quantised as n * scale - zero (fp16 pages: the values)"""
    page = data.shape[4]
    f16 = data.dtype == torch.float16
    out = []
    ip, ix, la = indptr.tolist(), indices.tolist(), last.tolist()
    for b in range(len(ip) - 1):
        pages = ix[ip[b]:ip[b + 1]]
        L = (len(pages) - 1) * page + la[b]
        kv = []
        for kvi in range(2):
            rows = data[pages, layer, kvi].permute(1, 0, 2, 3).reshape(data.shape[3], len(pages) * page, -1)[:, :L]   # [heads, L, .]
            if f16:
                x = rows.double()
            else:
                n = torch.stack((rows & 15, rows >> 4), dim=-1).reshape(*rows.shape[:-1], -1).double()
                par = param[pages, layer, kvi].permute(1, 0, 2, 3).reshape(data.shape[3], len(pages) * page, 2)[:, :L].double()
                x = n * par[..., 0:1] - par[..., 1:2]
            kv.append(x.permute(1, 0, 2))
        out.append(tuple(kv))
    return out


def _ref(q, dense, q_group, copies, qt=None):
    """fp64 causal attention: q [b, T, H, hd]; query head h reads cache head (h // q_group) * copies; token t sees rows 0 .. L - T + t"""
    b, T, H, hd = q.shape
    qq = q.double() if qt is None else torch.matmul(q.float(), qt.float()).half().double()   # (the launch rounds q . q_trans to fp16 as the reference does)
    heads = torch.tensor([(h // q_group) * copies for h in range(H)], device=q.device)
    out = torch.zeros(b, T, H, hd, dtype=torch.float64, device=q.device)
    for i in range(b):
        K, V = dense[i]
        L = K.shape[0]
        Kh, Vh = K[:, heads], V[:, heads]                                     # [L, H, hd]
        x = torch.einsum("thd,lhd->thl", qq[i], Kh) / hd ** 0.5
        mask = torch.arange(L, device=q.device)[None, :] > (L - T + torch.arange(T, device=q.device))[:, None]   # [T, L]
        x = x.masked_fill(mask[:, None, :], float("-inf"))
        out[i] = torch.einsum("thl,lhd->thd", torch.softmax(x, dim=-1), Vh)
    return out


def _close(o, ref, transpose_out=False, bar=1e-3):
    if transpose_out:
        o = o.transpose(-1, -2)
    err = (o.double() - ref).abs().amax(-1)
    scale = ref.abs().amax(-1)
    assert torch.isfinite(o.float()).all()
    assert (err <= bar * scale).all(), (err / scale).max().item()


CASES = [
    # bsz, lens, cache heads, q_group, copies, page, T, fp16 pages
    (1, [2048], 8, 4, 4, 2048, 4, False),               # Llama-3-8B replicated, read one copy (8 query heads here): split
    (1, [2048], 8, 4, 1, 2048, 4, False),               # ... the shared layout
    (1, [1500], 8, 4, 1, 2048, 16, True),               # fp16 pages
    (2, [700, 333], 4, 1, 1, 16, 2, False),             # multi-head attention, ragged, small pages
    (3, [3, 16, 18], 2, 4, 1, 16, 3, False),            # a request whose whole cache is its 3 new rows; new rows straddling a page
    (3, [5, 40, 23], 2, 4, 1, 8, 5, False),             # page_size 8 (a wave's rows straddle pages)
    (3, [17, 64, 49], 8, 4, 4, 24, 17, False),          # page_size 24; 17 tokens x 4 heads = 5 tiles; L == T
    (2, [100, 81], 1, 8, 1, 24, 8, True),               # group of 8 on fp16 pages of 24
    (4, [40, 90, 41, 300], 2, 8, 1, 16, 40, False),     # T = 40: the causal tail spans strides
    (2, [300, 64], 2, 1, 1, 16, 40, True),              # MHA, T = 40, fp16
    (16, [200 + 9 * i for i in range(16)], 8, 4, 4, 16, 4, False),   # replicated, 32 row sets
    (64, [100 + 3 * i for i in range(64)], 8, 4, 1, 64, 8, False),  # 64 x 8 x 2 tiles = 1024 workgroups: four waves (unsplit)
    (65, [50 + i for i in range(65)], 8, 4, 1, 16, 4, True),        # 520 workgroups: four waves, fp16 pages
    (66, [40 + 2 * i for i in range(66)], 32, 4, 4, 24, 4, False),  # 528: four waves, replicated, pages of 24 (rows straddle pages)
    (64, [60 + i for i in range(64)], 8, 4, 1, 8, 8, True),         # 1024: four waves, fp16 pages of 8
    (64, [60 + i for i in range(64)], 2, 4, 1, 8, 8, True),         # 256: eight waves, fp16, straddling
    (2, [900, 700], 2, 4, 1, 24, 4, True),                          # split, fp16 pages of 24
    (5, [513, 17, 260, 1000, 16], 4, 2, 2, 16, 16, False),          # replicated groups of 2
    (1, [700], 2, 2, 1, 24, 1, False),                              # T = 1
]


def _route(bsz, lens, cache_heads, q_group, copies, page, T, f16, split=True):
    """(waves per workgroup, rows never straddle a page, fp16 pages, split) of the launch fq_launch_kv_extend makes for a case"""
    wgs = bsz * (cache_heads // copies) * ((T * q_group + 15) // 16)
    s = min(16, 256 // wgs) if (split and wgs <= 128) else 1
    s = min(s, max(lens) // 128) if split else 1
    s = s if s >= 2 else 1
    return (8 if wgs * s <= 512 else 4, page % 16 == 0, f16, s > 1)


def test_the_cases_reach_every_compiled_kernel():
    """(the launch routing replayed over CASES with the three parameter sets below: all twelve kernels of fq_kvextend.hip run)"""
    seen = {_route(*c, split=sp) for c in CASES for sp in (True, False)}
    want = {(nw, uni, f16, sp) for nw in (4, 8) for uni in (False, True) for f16 in (False, True) for sp in (False, True) if nw == 8 or not sp}
    assert seen == want, sorted(want - seen)


@pytest.mark.parametrize("bsz,lens,cache_heads,q_group,copies,page,T,f16", CASES)
@pytest.mark.parametrize("trans,transpose_out,split", [(False, False, True), (True, True, True), (True, False, False)])
def test_extend_matches_fp64_causal_attention(ops, bsz, lens, cache_heads, q_group, copies, page, T, f16, trans, transpose_out, split):
    g = torch.Generator(device="cuda").manual_seed(bsz * 1000 + lens[0] + T)
    hd, layer = 128, 1
    data, param, indptr, indices, last = _cache(g, lens, cache_heads, page, f16)
    H = cache_heads // copies * q_group
    q = (torch.randn(bsz, T, H, hd, generator=g, device="cuda") * 0.5).half()
    qt = (torch.randn(hd, hd, generator=g, device="cuda") / hd ** 0.5).half() if trans else None
    o = ops.kv_batch_extend(q, data, param, indptr, indices, last, layer, qt, transpose_out, seq_hint=max(lens), split=split, kv_copies=copies)
    assert o.shape == ((bsz, T, hd, H) if transpose_out else (bsz, T, H, hd))
    ref = _ref(q, _dense(data, param, indptr, indices, last, layer), q_group, copies, qt)
    _close(o, ref, transpose_out)


@pytest.mark.parametrize("f16,page,split", [(False, 16, True), (False, 24, False), (True, 16, True), (True, 8, False)])
def test_causality_bit_for_bit(ops, f16, page, split):
    """Rewriting row L - 1 (the step's last token) changes nothing for tokens 0 .. T - 2, and token T - 1's output; NaN in the unused tail of every
    last page changes nothing at all."""
    g = torch.Generator(device="cuda").manual_seed(7 + page)
    hd, layer, T = 128, 0, 5
    lens = [300, 37, 5, 130]
    data, param, indptr, indices, last = _cache(g, lens, 2, page, f16)
    q = (torch.randn(len(lens), T, 8, hd, generator=g, device="cuda") * 0.5).half()
    run = lambda d, p: ops.kv_batch_extend(q, d, p, indptr, indices, last, layer, split=split)     # (no length hint: 16 splits, some empty)
    o0 = run(data, param)
    d1, p1 = data.clone(), param.clone()
    ip, ix = indptr.tolist(), indices.tolist()
    for b, L in enumerate(lens):
        pg, ent = ix[ip[b] + (L - 1) // page], (L - 1) % page
        if f16:
            d1[pg, layer, :, :, ent] = (torch.randn(2, 2, hd, generator=g, device="cuda") * 3).half()
        else:
            d1[pg, layer, :, :, ent] = torch.randint(0, 256, (2, 2, hd // 2), generator=g, device="cuda", dtype=torch.uint8)
            p1[pg, layer, :, :, ent] = torch.tensor([0.25, -1.0], device="cuda").half()
    o1 = run(d1, p1)
    assert torch.equal(o1[:, :T - 1], o0[:, :T - 1])
    for b in range(len(lens)):
        assert not torch.equal(o1[b, T - 1], o0[b, T - 1])
    d2, p2 = data.clone(), param.clone()
    for b, L in enumerate(lens):
        pg, used = ix[ip[b + 1] - 1], (L - 1) % page + 1
        p2[pg, :, :, :, used:] = float("nan")
        if f16:
            d2[pg, :, :, :, used:] = float("nan")
    o2 = run(d2, p2)
    assert torch.isfinite(o2.float()).all() and torch.equal(o2, o0)


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("bsz,cache_heads,q_group,copies", [(1, 8, 4, 4), (3, 2, 4, 1), (5, 4, 1, 1), (40, 8, 4, 4)])
def test_one_token_equals_the_decode_launch(ops, f16, bsz, cache_heads, q_group, copies):
    g = torch.Generator(device="cuda").manual_seed(bsz + cache_heads + q_group + f16)
    hd, layer = 128, 1
    lens = [50 + 131 * i for i in range(bsz)]
    data, param, indptr, indices, last = _cache(g, lens, cache_heads, 16, f16)
    H = cache_heads // copies * q_group
    q = (torch.randn(bsz, 1, H, hd, generator=g, device="cuda") * 0.5).half()
    o = ops.kv_batch_extend(q, data, param, indptr, indices, last, layer, seq_hint=max(lens), kv_copies=copies)
    od = ops.kv_batch_decode(q[:, 0].contiguous(), data, param, indptr, indices, last, layer, seq_hint=max(lens), kv_copies=copies)
    ref = _ref(q, _dense(data, param, indptr, indices, last, layer), q_group, copies)
    _close(o, ref)
    _close(od.unsqueeze(1), ref)
    err = (o[:, 0].double() - od.double()).abs().amax(-1)
    assert (err <= 1e-3 * ref[:, 0].abs().amax(-1)).all()


def _written(cache):
    """(rows, parameters) of every written cache entry, entry by entry: pages beyond a request's length hold whatever the allocator left"""
    cache._flush_pending()
    s = cache._specs
    data, param = s["kv_data"], s["kv_param"]
    page = data.shape[4]
    keep = torch.zeros(data.shape[0], page, dtype=torch.bool, device=data.device)
    ip, ix, la = s["kv_indptr"].tolist(), s["kv_indices"].tolist(), s["last_page_offset"].tolist()
    for b in range(len(ip) - 1):
        pages = ix[ip[b]:ip[b + 1]]
        for j, pg in enumerate(pages):
            keep[pg, :(la[b] if j == len(pages) - 1 else page)] = True
    return data.permute(0, 4, 1, 2, 3, 5)[keep], param.permute(0, 4, 1, 2, 3, 5)[keep].view(torch.int16)


def _cache_rows(cache, layer, n_heads_cache):
    """the cache's de-quantised rows per request and its index tensors, as the closure's launch reads them"""
    s = cache._specs
    return _dense(s["kv_data"], s["kv_param"], s["kv_indptr"], s["kv_indices"], s["last_page_offset"], layer)


CLASS_CASES = [
    # trans, disable_quant, share_kv_heads, group_size, ragged mask
    ("matmul", False, False, 4, False),
    ("matmul", False, False, 4, True),
    ("had", False, False, 4, False),
    ("none", False, True, 4, True),
    ("matmul", True, False, 4, False),
    ("had", True, True, 8, True),
    ("matmul", False, True, 8, False),
    ("none", True, False, 8, False),
]


@pytest.mark.parametrize("trans,disable_quant,share,group,ragged", CLASS_CASES)
def test_cache_class_multi_token_steps_match_dense_attention(ops, trans, disable_quant, share, group, ragged):
    """prompt -> 2 decode steps -> a 4-token step -> 2 decode steps -> a 3-token step, 2 layers; every attention against dense fp64 causal
    attention over what the cache holds."""
    import flatquant_amd.deploy.transformers as TR
    g = torch.Generator(device="cuda").manual_seed(len(trans) + group + 10 * disable_quant + 100 * share + 1000 * ragged)
    bsz, prompt, kv_heads, hd, layers, page = 3, 21, 2, 128, 2, 16
    H = kv_heads * group
    cache = TR.MultiLayerPagedKVCache4Bit(bsz, page, 64, "cuda", layers, H, hd, disable_quant=disable_quant, trans=trans, group_size=group,
                                          share_kv_heads=share)
    tk = torch.linalg.qr(torch.randn(hd, hd, generator=g, device="cuda"))[0].half()      # (a well-conditioned learned transform)
    tk_inv_t = torch.linalg.inv(tk.float()).T.contiguous().half()
    mask = torch.ones(bsz, prompt, dtype=torch.int64, device="cuda")
    if ragged:
        mask[1, :3] = 0
        mask[2, :1] = 0
    kw = {"trans_matrix_k": tk, "trans_matrix_k_inv_t": tk_inv_t}
    if ragged:
        kw["attention_mask"] = mask
    for layer in range(layers):
        k = torch.randn(bsz, prompt, kv_heads, hd, generator=g, device="cuda").half()
        v = torch.randn(bsz, prompt, kv_heads, hd, generator=g, device="cuda").half()
        cache.update(k, v, layer, dict(kw))
    copies = group if (not share and cache.read_one_copy) else 1
    n_cache = cache._pages.shape[3]
    for added in (1, 1, 4, 1, 1, 3):
        if ragged:
            mask = torch.cat([mask, torch.ones(bsz, added, dtype=mask.dtype, device="cuda")], dim=1)
            kw["attention_mask"] = mask
        for layer in range(layers):
            k = torch.randn(bsz, added, kv_heads, hd, generator=g, device="cuda").half()
            v = torch.randn(bsz, added, kv_heads, hd, generator=g, device="cuda").half()
            attend = cache.update(k, v, layer, dict(kw))
            q = (torch.randn(bsz, added, H, hd, generator=g, device="cuda") * 0.5).half()
            o = attend(q)
            assert o.shape == q.shape
            ot = attend(q, transposed=True)
            assert ((ot.transpose(-1, -2).float() - o.float()).abs().amax() <= 1e-3 * o.float().abs().amax()).item()
            qq = ops.hadamard(q.contiguous()) if trans == "had" else q
            qtm = tk_inv_t if trans == "matmul" else None
            q_group = group if share else 1
            ref = _ref(qq, _cache_rows(cache, layer, n_cache), q_group if copies == 1 else group, copies if copies > 1 else 1, qtm)
            err = (o.double() - ref).abs().amax(-1) / ref.abs().amax(-1)
            assert err.max().item() <= 3e-3, (added, layer, err.max().item())
    if not ragged:
        assert cache.get_seq_length() == prompt + 11


@pytest.mark.parametrize("fuse_append,disable_quant,trans", [(True, False, "matmul"), (False, False, "matmul"), (True, True, "had"), (False, True, "none")])
def test_a_verify_step_equals_sequential_decode(ops, fuse_append, disable_quant, trans):
    import flatquant_amd.deploy.transformers as TR
    g = torch.Generator(device="cuda").manual_seed(5)
    bsz, prompt, kv_heads, group, hd, layers, T = 2, 30, 2, 4, 128, 2, 4
    H = kv_heads * group
    tk = (torch.randn(hd, hd, generator=g, device="cuda") / hd ** 0.5).half()
    kw = {"trans_matrix_k": tk, "trans_matrix_k_inv_t": torch.linalg.inv(tk.float()).T.contiguous().half()}
    mk = lambda: TR.MultiLayerPagedKVCache4Bit(bsz, 16, 64, "cuda", layers, H, hd, trans=trans, group_size=group, fuse_append=fuse_append,
                                               disable_quant=disable_quant)
    a, s = mk(), mk()
    for layer in range(layers):
        k = torch.randn(bsz, prompt, kv_heads, hd, generator=g, device="cuda").half()
        v = torch.randn(bsz, prompt, kv_heads, hd, generator=g, device="cuda").half()
        a.update(k, v, layer, dict(kw)), s.update(k, v, layer, dict(kw))
    ks = [torch.randn(bsz, T, kv_heads, hd, generator=g, device="cuda").half() for _ in range(layers)]
    vs = [torch.randn(bsz, T, kv_heads, hd, generator=g, device="cuda").half() for _ in range(layers)]
    qs = [(torch.randn(bsz, T, H, hd, generator=g, device="cuda") * 0.5).half() for _ in range(layers)]
    oa = [a.update(ks[l], vs[l], l, dict(kw))(qs[l]) for l in range(layers)]
    os_ = [[] for _ in range(layers)]
    for t in range(T):
        for l in range(layers):
            att = s.update(ks[l][:, t:t + 1].contiguous(), vs[l][:, t:t + 1].contiguous(), l, dict(kw))
            os_[l].append(att(qs[l][:, t:t + 1].contiguous()))
    (da, pa), (ds, ps) = _written(a), _written(s)
    assert torch.equal(da, ds) and torch.equal(pa, ps)
    if disable_quant:
        # fp16 pages: the T-token append stored exactly the step's (rotated) keys and its values, every request at ITS positions L - T .. L - 1,
        # one copy per query head of the group
        sp = a._specs
        ip, ix, page, L = sp["kv_indptr"].tolist(), sp["kv_indices"].tolist(), a.page_size, a.length
        for l in range(layers):
            kk = ops.hadamard(ks[l].contiguous()) if trans == "had" else ks[l]
            for b in range(bsz):
                for t in range(T):
                    pos = L - T + t
                    pg, ent = ix[ip[b] + pos // page], pos % page
                    assert torch.equal(a.pages[pg, l, 0, :, ent], kk[b, t].repeat_interleave(group, dim=0))
                    assert torch.equal(a.pages[pg, l, 1, :, ent], vs[l][b, t].repeat_interleave(group, dim=0))
    for l in range(layers):
        o2 = torch.cat(os_[l], dim=1)
        err = (oa[l].float() - o2.float()).abs().amax(-1)
        assert (err <= 2e-3 * o2.float().abs().amax(-1)).all(), err.max().item()


def test_closure_capture_replays_bit_for_bit_and_graphed_decode_replays_verify_steps(ops):
    import flatquant_amd.deploy as deploy
    import flatquant_amd.deploy.transformers as TR
    g = torch.Generator(device="cuda").manual_seed(11)
    bsz, prompt, kv_heads, group, hd, T = 1, 900, 8, 4, 128, 4
    H = kv_heads * group
    cache = TR.MultiLayerPagedKVCache4Bit(bsz, 16, 1200, "cuda", 1, H, hd, trans="none", group_size=group)
    cache.update(torch.randn(bsz, prompt, kv_heads, hd, generator=g, device="cuda").half(),
                 torch.randn(bsz, prompt, kv_heads, hd, generator=g, device="cuda").half(), 0)
    attend = cache.update(torch.randn(bsz, T, kv_heads, hd, generator=g, device="cuda").half(),
                          torch.randn(bsz, T, kv_heads, hd, generator=g, device="cuda").half(), 0)
    qs = [(torch.randn(bsz, T, H, hd, generator=g, device="cuda") * 0.5).half() for _ in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [attend(q).clone() for q in qs]               # (warms the split workspace on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    q_static = qs[0].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = attend(q_static)
    for q, e in zip(qs, eager):
        q_static.copy_(q)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, e)
    # GraphedDecode around a whole verify step (append + attention): two eager warm-ups, one capture, replays — against an eager twin
    twin = TR.MultiLayerPagedKVCache4Bit(bsz, 16, 1200, "cuda", 1, H, hd, trans="none", group_size=group)
    a = TR.MultiLayerPagedKVCache4Bit(bsz, 16, 1200, "cuda", 1, H, hd, trans="none", group_size=group)
    k0 = torch.randn(bsz, 40, kv_heads, hd, generator=g, device="cuda").half()
    v0 = torch.randn(bsz, 40, kv_heads, hd, generator=g, device="cuda").half()
    twin.update(k0, v0, 0), a.update(k0, v0, 0)

    def step(k, v, q, c):
        return c.update(k, v, 0)(q)

    gd = deploy.GraphedDecode(step)
    with torch.no_grad():
        for i in range(7):
            k = torch.randn(bsz, T, kv_heads, hd, generator=g, device="cuda").half()
            v = torch.randn(bsz, T, kv_heads, hd, generator=g, device="cuda").half()
            q = (torch.randn(bsz, T, H, hd, generator=g, device="cuda") * 0.5).half()
            got = gd(k, v, q, a).clone()
            want = step(k, v, q, twin)
            err = (got.float() - want.float()).abs().amax(-1)
            assert (err <= 2e-3 * want.float().abs().amax(-1)).all(), (i, err.max().item())
    assert gd.captures == 1 and gd.replays >= 3 and a.get_seq_length() == twin.get_seq_length() == 40 + 7 * T
    (da, pa), (dt, pt) = _written(a), _written(twin)
    assert torch.equal(da, dt) and torch.equal(pa, pt)


@pytest.mark.parametrize("disable_quant", [True, False])
def test_graphed_decode_alternating_step_sizes(ops, disable_quant):
    """Steps of 1, 4 and 3 tokens alternating under deploy.GraphedDecode (a decode step, a verify step, a chunked prompt's remainder): each size
    is warmed up, captured and replayed; every output against an eager twin, the cache's written rows bit for bit at the end. On fp16 pages the
    append of every size reads a per-size seqlen_indptr and the (1, 0) parameters that a captured step holds by address."""
    import flatquant_amd.deploy as deploy
    import flatquant_amd.deploy.transformers as TR
    g = torch.Generator(device="cuda").manual_seed(13)
    bsz, kv_heads, group, hd, layers = 2, 2, 4, 128, 2
    H = kv_heads * group
    mk = lambda: TR.MultiLayerPagedKVCache4Bit(bsz, 16, 256, "cuda", layers, H, hd, trans="had", group_size=group, disable_quant=disable_quant)
    a, twin = mk(), mk()
    for l in range(layers):
        k0 = torch.randn(bsz, 20, kv_heads, hd, generator=g, device="cuda").half()
        v0 = torch.randn(bsz, 20, kv_heads, hd, generator=g, device="cuda").half()
        a.update(k0, v0, l), twin.update(k0, v0, l)

    def step(k, v, q, c):
        return torch.stack([c.update(k[l], v[l], l)(q[l]) for l in range(layers)])

    gd = deploy.GraphedDecode(step)
    with torch.no_grad():
        for i, T in enumerate([1, 4, 3] * 5):
            k = torch.randn(layers, bsz, T, kv_heads, hd, generator=g, device="cuda").half()
            v = torch.randn(layers, bsz, T, kv_heads, hd, generator=g, device="cuda").half()
            q = (torch.randn(layers, bsz, T, H, hd, generator=g, device="cuda") * 0.5).half()
            got = gd(k, v, q, a).clone()
            want = step(k, v, q, twin)
            err = (got.float() - want.float()).abs().amax(-1)
            assert (err <= 2e-3 * want.float().abs().amax(-1)).all(), (i, T, err.max().item())
    assert gd.captures == 3 and gd.replays >= 6
    assert a.get_seq_length() == twin.get_seq_length() == 20 + 5 * 8
    (da, pa), (dt, pt) = _written(a), _written(twin)
    assert torch.equal(da, dt) and torch.equal(pa, pt)


def test_repeated_split_launches_are_bit_identical(ops):
    g = torch.Generator(device="cuda").manual_seed(3)
    data, param, indptr, indices, last = _cache(g, [2048], 32, 2048, False)      # the replicated layout, 8 KV heads
    q = (torch.randn(1, 4, 32, 128, generator=g, device="cuda") * 0.5).half()
    outs = [ops.kv_batch_extend(q, data, param, indptr, indices, last, 1, seq_hint=2048, kv_copies=4) for _ in range(50)]
    assert all(torch.equal(o, outs[0]) for o in outs)
    ref = _ref(q, _dense(data, param, indptr, indices, last, 1), 4, 4)
    _close(outs[0], ref)


def test_errors(ops):
    import ctypes
    import flatquant_amd.deploy.transformers as TR
    from flatquant_amd._lib import FQ_EINVAL, FQ_EUNSUPPORTED, lib
    cache = TR.MultiLayerPagedKVCache4Bit(1, 16, 64, "cuda", 1, 8, 128, trans="none", group_size=4)
    g = torch.Generator(device="cuda").manual_seed(0)
    cache.update(torch.randn(1, 10, 2, 128, generator=g, device="cuda").half(), torch.randn(1, 10, 2, 128, generator=g, device="cuda").half(), 0)
    attend = cache.update(torch.randn(1, 3, 2, 128, generator=g, device="cuda").half(), torch.randn(1, 3, 2, 128, generator=g, device="cuda").half(), 0)
    with pytest.raises(ValueError):
        attend(torch.randn(1, 2, 8, 128, device="cuda").half())
    vp = ctypes.c_void_p(4096)
    assert lib.fq_kv_batch_extend(0, vp, vp, None, 0, vp, vp, vp, vp, vp, 1, 0, 8, 1, 1, 0, 16, 128, 1, 0, None, 0, None) == FQ_EINVAL
    assert lib.fq_kv_batch_extend(0, vp, vp, None, 0, vp, vp, vp, vp, vp, 1, 0, 8, 3, 2, 2, 16, 128, 1, 0, None, 0, None) == FQ_EINVAL
    assert lib.fq_kv_batch_extend(0, vp, vp, None, 0, vp, vp, vp, vp, vp, 1, 0, 8, 1, 1, 2, 16, 64, 1, 0, None, 0, None) == FQ_EUNSUPPORTED
    assert lib.fq_kv_extend_workspace_bytes(1, 32, 0, 128) < 0
