"""Prompt-sized steps over the paged KV cache (fq_kv_chunk_extend / ops.kv_chunk_extend): fq_kv_batch_extend's contract computed 128
(token, head) rows per workgroup. Against an fp64 dense causal attention over the de-quantised cache (the project's bar for every attention
launch: the worst row within 1e-3 of its maximum) and against ops.kv_batch_extend (2e-3: the sum of the two launches' bars); causality, the
pieces of a step, repeated launches bit for bit; the memory contract under guard bands (tests/guards.py); MultiLayerPagedKVCache4Bit routed to
it; argument errors.

The cache builder, the fp64 reference and the closeness check restate tests/test_gpu_kv_extend.py's _cache, _dense, _ref and _close (random
pages, q * 0.5, the q_trans product rounded to fp16 in the reference); the builder can also leave pages no request owns and fill everything no
request holds — the unused tail of every last page, the unowned pages — with 0xFF bytes / NaN."""
import functools

import pytest
import torch

from tests import guards

pytestmark = pytest.mark.gpu

HD = 128


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


def _cache(g, lens, cache_heads, page, f16, hd=HD, layers=2, spare=0, dead=False):
    """a cache whose request b holds lens[b] rows, pages scattered; `spare` pages no request owns; `dead`: rows no request holds are 0xFF / NaN"""
    n_pg = [(n + page - 1) // page for n in lens]
    tot = sum(n_pg) + spare
    if f16:
        data = (torch.randn(tot, layers, 2, cache_heads, page, hd, generator=g, device="cuda") * 1.5).half()
    else:
        data = torch.randint(0, 256, (tot, layers, 2, cache_heads, page, hd // 2), generator=g, device="cuda", dtype=torch.uint8)
    param = torch.stack([torch.rand(tot, layers, 2, cache_heads, page, generator=g, device="cuda") * 0.3 + 0.02,
                         torch.rand(tot, layers, 2, cache_heads, page, generator=g, device="cuda") * 2.0 + 0.1], dim=-1).half()
    indptr = torch.tensor([0] + list(torch.tensor(n_pg).cumsum(0)), dtype=torch.int32, device="cuda")
    indices = torch.randperm(tot, generator=g, device="cuda").to(torch.int32)[:sum(n_pg)].contiguous()
    last = torch.tensor([(n - 1) % page + 1 for n in lens], dtype=torch.int32, device="cuda")
    if dead:
        _kill(data, param, indptr, indices, lens)
    return data, param, indptr, indices, last


def _kill(data, param, indptr, indices, lens):
    """every row no request holds (the tail of a last page, a page nobody owns), in every layer and head: 0xFF bytes / NaN rows, NaN parameters"""
    page = data.shape[4]
    used = torch.zeros(data.shape[0], page, dtype=torch.bool, device=data.device)
    ip, ix = indptr.tolist(), indices.tolist()
    for b, n in enumerate(lens):
        for i, pg in enumerate(ix[ip[b]:ip[b + 1]]):
            used[pg, :max(0, min(page, n - i * page))] = True
    deadrows = ~used[:, None, None, None, :].expand(data.shape[:5])
    data[deadrows] = float("nan") if data.dtype == torch.float16 else 0xFF
    param[deadrows] = float("nan")


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


def _worst(o, ref, transpose_out=False):
    """the worst row's error as a fraction of the row's maximum"""
    if transpose_out:
        o = o.transpose(-1, -2)
    assert torch.isfinite(o.float()).all()
    return ((o.double() - ref).abs().amax(-1) / ref.abs().amax(-1)).max().item()


CASES = [
    # bsz, lens, cache heads, q_group, copies, page, T, fp16 pages
    (1, [2048], 8, 4, 4, 2048, 32, False),              # exactly one block, 32 tiles, one page, the replicated layout read one copy
    (1, [300], 2, 4, 1, 16, 33, False),                 # the second block holds one token: three idle waves
    (3, [70, 200, 71], 2, 4, 1, 24, 70, False),         # L = T (token 0 sees one row), L - T = 1, tile rows straddling pages of 24
    (2, [513, 140], 2, 1, 1, 16, 130, False),           # MHA with 128 tokens per block, the diagonal in mid-tile
    (2, [200, 90], 1, 8, 1, 8, 17, True),               # group 8, 16 tokens per block, fp16 pages of 8
    (2, [333, 100], 2, 2, 2, 16, 65, False),            # group 2, replicated
    (4, [40, 90, 41, 300], 2, 8, 1, 16, 40, False),     # tests/test_gpu_kv_extend.py's T = 40 case
    (1, [1500], 8, 4, 1, 2048, 5, True),                # fewer rows than one wave holds
    (1, [64], 1, 4, 1, 64, 64, False),                  # L = T = one tile
    (2, [129, 128], 1, 1, 1, 16, 128, False),           # one full MHA block, L - T = 1 and 0
]
MODES = [(False, False), (True, True)]                   # (q_trans, transpose_out)


@functools.lru_cache(maxsize=None)
def _case(i, trans):
    """a case's inputs, its fp64 reference and both launches' outputs: computed once, shared by the tests below, never changed"""
    from flatquant_amd import ops
    bsz, lens, cache_heads, q_group, copies, page, T, f16 = CASES[i]
    g = torch.Generator(device="cuda").manual_seed(bsz * 1000 + lens[0] + T)
    data, param, indptr, indices, last = _cache(g, lens, cache_heads, page, f16)
    H = cache_heads // copies * q_group
    q = (torch.randn(bsz, T, H, HD, generator=g, device="cuda") * 0.5).half()
    qt = (torch.randn(HD, HD, generator=g, device="cuda") / HD ** 0.5).half() if trans else None
    ref = _ref(q, _dense(data, param, indptr, indices, last, 1), q_group, copies, qt)
    new = ops.kv_chunk_extend(q, data, param, indptr, indices, last, 1, qt, trans, kv_copies=copies)
    old = ops.kv_batch_extend(q, data, param, indptr, indices, last, 1, qt, trans, seq_hint=max(lens), kv_copies=copies)
    return dict(q=q, qt=qt, ref=ref, new=new, old=old, H=H)


@pytest.mark.parametrize("i", range(len(CASES)))
@pytest.mark.parametrize("trans,transpose_out", MODES)
def test_chunk_extend_matches_fp64_causal_attention(ops, i, trans, transpose_out):
    c = _case(i, trans)
    bsz, T = CASES[i][0], CASES[i][6]
    assert c["new"].shape == ((bsz, T, HD, c["H"]) if transpose_out else (bsz, T, c["H"], HD))
    worst = _worst(c["new"], c["ref"], transpose_out)
    print(f"case {i} q_trans={trans}: worst row {worst:.3e} of its maximum (fq_kv_batch_extend {_worst(c['old'], c['ref'], transpose_out):.3e})")
    assert worst <= 1e-3, worst


@pytest.mark.parametrize("i", range(len(CASES)))
@pytest.mark.parametrize("trans,transpose_out", MODES)
def test_chunk_extend_agrees_with_the_extend_launch(ops, i, trans, transpose_out):
    """|new - old| within 2e-3 of the row maximum: the sum of the two launches' bars against fp64"""
    c = _case(i, trans)
    new, old = (t.transpose(-1, -2) if transpose_out else t for t in (c["new"], c["old"]))
    err = ((new.double() - old.double()).abs().amax(-1) / c["ref"].abs().amax(-1)).max().item()
    print(f"case {i} q_trans={trans}: |new - old| {err:.3e} of the row maximum")
    assert err <= 2e-3, err


@pytest.mark.parametrize("f16,page", [(False, 16), (False, 24), (True, 16), (True, 8)])
def test_causality_bit_for_bit(ops, f16, page):
    """Rewriting row L - 1 (the step's last token) with other finite values leaves tokens 0 .. T - 2 unchanged (and changes token T - 1). NaN
    (fp16 pages) or 0xFF bytes with NaN parameters (INT4) change nothing at all in the unused tail of every last page, in the other layer, in
    the cache heads no query head maps to, in pages no request owns."""
    g = torch.Generator(device="cuda").manual_seed(7 + page)
    layer, T, cache_heads, copies = 0, 37, 4, 2
    lens = [300, 37, 38, 130]
    data, param, indptr, indices, last = _cache(g, lens, cache_heads, page, f16, spare=2)
    q = (torch.randn(len(lens), T, cache_heads, HD, generator=g, device="cuda") * 0.5).half()      # replicated pairs: query head h reads cache head (h // 2) * 2
    run = lambda d, p: ops.kv_chunk_extend(q, d, p, indptr, indices, last, layer, kv_copies=copies)
    o0 = run(data, param)
    assert torch.isfinite(o0.float()).all()
    d1, p1 = data.clone(), param.clone()
    ip, ix = indptr.tolist(), indices.tolist()
    for b, L in enumerate(lens):
        pg, ent = ix[ip[b] + (L - 1) // page], (L - 1) % page
        if f16:
            d1[pg, layer, :, :, ent] = (torch.randn(2, cache_heads, HD, generator=g, device="cuda") * 3).half()
        else:
            d1[pg, layer, :, :, ent] = torch.randint(0, 256, (2, cache_heads, HD // 2), generator=g, device="cuda", dtype=torch.uint8)
            p1[pg, layer, :, :, ent] = torch.tensor([0.25, -1.0], device="cuda").half()
    o1 = run(d1, p1)
    assert torch.equal(o1[:, :T - 1], o0[:, :T - 1])
    for b in range(len(lens)):
        assert not torch.equal(o1[b, T - 1], o0[b, T - 1])
    d2, p2 = data.clone(), param.clone()
    _kill(d2, p2, indptr, indices, lens)                         # tails of last pages and unowned pages, every layer and head
    bad = float("nan") if f16 else 0xFF
    d2[:, 1 - layer], p2[:, 1 - layer] = bad, float("nan")       # the other layer
    d2[:, :, :, 1::2], p2[:, :, :, 1::2] = bad, float("nan")     # the second copy of every pair: no query head maps to it
    o2 = run(d2, p2)
    assert torch.isfinite(o2.float()).all() and torch.equal(o2, o0)


def _shorter(indptr, indices, last, lens, page, cut):
    """index tensors that describe lens[b] - cut rows over the same pages"""
    ip, ix = indptr.tolist(), indices.tolist()
    short = [n - cut for n in lens]
    n_pg = [(n + page - 1) // page for n in short]
    idx = [pg for b in range(len(lens)) for pg in ix[ip[b]:ip[b] + n_pg[b]]]
    return (torch.tensor([0] + list(torch.tensor(n_pg).cumsum(0)), dtype=torch.int32, device="cuda"),
            torch.tensor(idx, dtype=torch.int32, device="cuda"),
            torch.tensor([(n - 1) % page + 1 for n in short], dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("f16,page", [(False, 16), (True, 24)])
@pytest.mark.parametrize("trans,transpose_out", MODES)
def test_the_pieces_of_a_step_equal_the_step_bit_for_bit(ops, f16, page, trans, transpose_out):
    """One launch of T = 70 against the launches of its first 33 and its last 37 tokens; the first of those reads index tensors that say L - 37."""
    g = torch.Generator(device="cuda").manual_seed(70 + page)
    T, T2, layer = 70, 37, 1
    lens = [70, 200, 71, 333]
    data, param, indptr, indices, last = _cache(g, lens, 2, page, f16)
    q = (torch.randn(len(lens), T, 8, HD, generator=g, device="cuda") * 0.5).half()
    qt = (torch.randn(HD, HD, generator=g, device="cuda") / HD ** 0.5).half() if trans else None
    whole = ops.kv_chunk_extend(q, data, param, indptr, indices, last, layer, qt, transpose_out)
    first = ops.kv_chunk_extend(q[:, :T - T2].contiguous(), data, param, *_shorter(indptr, indices, last, lens, page, T2), layer, qt, transpose_out)
    second = ops.kv_chunk_extend(q[:, T - T2:].contiguous(), data, param, indptr, indices, last, layer, qt, transpose_out)
    assert torch.isfinite(whole.float()).all()
    assert torch.equal(whole[:, :T - T2], first) and torch.equal(whole[:, T - T2:], second)


@pytest.mark.parametrize("i", [0, 2, 4])
def test_two_launches_are_bit_identical(ops, i):
    bsz, lens, cache_heads, q_group, copies, page, T, f16 = CASES[i]
    g = torch.Generator(device="cuda").manual_seed(i)
    data, param, indptr, indices, last = _cache(g, lens, cache_heads, page, f16)
    q = (torch.randn(bsz, T, cache_heads // copies * q_group, HD, generator=g, device="cuda") * 0.5).half()
    outs = [ops.kv_chunk_extend(q, data, param, indptr, indices, last, 0, kv_copies=copies) for _ in range(3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("lens,cache_heads,q_group,copies,page,T,f16", [([300, 33, 161], 2, 4, 1, 16, 33, False), ([200, 90, 17], 4, 2, 2, 24, 17, True)])
@pytest.mark.parametrize("trans,transpose_out", MODES)
def test_memory_contract_under_guard_bands(ops, lens, cache_heads, q_group, copies, page, T, f16, trans, transpose_out):
    """Under both poisons the output is written completely (bit-identical between them and to the plain run) and nothing outside it is touched;
    q, q_trans, the pages and the parameters between pads that would change a result (NaN / 0xFF), the index tensors between valid pads, the
    dead rows of the cache 0xFF / NaN: none of it changes a result."""
    g = torch.Generator(device="cuda").manual_seed(sum(lens))
    data, param, indptr, indices, last = _cache(g, lens, cache_heads, page, f16, spare=3, dead=True)
    q = (torch.randn(len(lens), T, cache_heads // copies * q_group, HD, generator=g, device="cuda") * 0.5).half()
    qt = (torch.randn(HD, HD, generator=g, device="cuda") / HD ** 0.5).half() if trans else None
    call = lambda q, data, param, indptr, indices, last, qt: ops.kv_chunk_extend(q, data, param, indptr, indices, last, 0, qt, transpose_out, kv_copies=copies)
    inputs = dict(q=q, data=data, param=param, indptr=indptr, indices=indices, last=last, qt=qt)
    want = call(**inputs)
    torch.cuda.synchronize()
    assert torch.isfinite(want.float()).all()
    got = []
    for poison in guards.POISONS:
        guard = guards.Guard(poison)
        with guard.on(ops):
            gi = {k: (None if v is None else guard.guard_input(v, "repeat" if k in ("indptr", "indices", "last") else "auto")) for k, v in inputs.items()}
            got.append(call(**gi))
            torch.cuda.synchronize()
        guard.check()
        assert len(guard.find("empty")) == 1                     # the output is the launch's one allocation: no workspace
    assert guards.same_raw(got[0], got[1]), "differs between the two poisons: not written completely, or a pad was read"
    assert guards.same_raw(got[0], want), "differs from the plain run"


CLASS_CASES = [
    # trans, disable_quant, share_kv_heads, group_size, ragged mask  (tests/test_gpu_kv_extend.py's configurations)
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
def test_cache_class_routes_long_steps_to_the_chunk_launch(ops, monkeypatch, trans, disable_quant, share, group, ragged):
    """EXTEND_CHUNK_MIN_TOKENS patched to 16: a 21-token prompt, two decode steps, a 40-token step, a decode step and a 17-token step over two
    layers; every attention within 3e-3 of dense fp64 causal attention over what the cache holds (the class test's bar), the transposed form
    agreeing with the plain one as there, and the two long steps on ops.kv_chunk_extend. Pages of 16 as there, of 24 with a ragged mask: the class
    wants every request to need the same number of pages (kv_cache.py:371-372), and after this test's 81 tokens a request with fewer rows would
    need fewer pages of 16."""
    import flatquant_amd.deploy.transformers as TR
    from flatquant_amd.deploy.transformers import kv_cache as KC
    monkeypatch.setattr(KC, "EXTEND_CHUNK_MIN_TOKENS", 16)
    calls = []
    real = ops.kv_chunk_extend
    monkeypatch.setattr(ops, "kv_chunk_extend", lambda q, *a, **k: (calls.append(q.shape[1]), real(q, *a, **k))[1])
    g = torch.Generator(device="cuda").manual_seed(len(trans) + group + 10 * disable_quant + 100 * share + 1000 * ragged)
    bsz, prompt, kv_heads, layers, page = 3, 21, 2, 2, 24 if ragged else 16
    H = kv_heads * group
    cache = TR.MultiLayerPagedKVCache4Bit(bsz, page, 128, "cuda", layers, H, HD, disable_quant=disable_quant, trans=trans, group_size=group,
                                          share_kv_heads=share)
    tk = torch.linalg.qr(torch.randn(HD, HD, generator=g, device="cuda"))[0].half()      # (a well-conditioned learned transform)
    tk_inv_t = torch.linalg.inv(tk.float()).T.contiguous().half()
    mask = torch.ones(bsz, prompt, dtype=torch.int64, device="cuda")
    if ragged:
        mask[1, :3] = 0
        mask[2, :1] = 0
    kw = {"trans_matrix_k": tk, "trans_matrix_k_inv_t": tk_inv_t}
    if ragged:
        kw["attention_mask"] = mask
    for layer in range(layers):
        k = torch.randn(bsz, prompt, kv_heads, HD, generator=g, device="cuda").half()
        v = torch.randn(bsz, prompt, kv_heads, HD, generator=g, device="cuda").half()
        cache.update(k, v, layer, dict(kw))
    copies = group if (not share and cache.read_one_copy) else 1
    steps = (1, 1, 40, 1, 17)
    for added in steps:
        if ragged:
            mask = torch.cat([mask, torch.ones(bsz, added, dtype=mask.dtype, device="cuda")], dim=1)
            kw["attention_mask"] = mask
        for layer in range(layers):
            k = torch.randn(bsz, added, kv_heads, HD, generator=g, device="cuda").half()
            v = torch.randn(bsz, added, kv_heads, HD, generator=g, device="cuda").half()
            attend = cache.update(k, v, layer, dict(kw))
            q = (torch.randn(bsz, added, H, HD, generator=g, device="cuda") * 0.5).half()
            o = attend(q)
            assert o.shape == q.shape
            ot = attend(q, transposed=True)
            assert ((ot.transpose(-1, -2).float() - o.float()).abs().amax() <= 1e-3 * o.float().abs().amax()).item()
            qq = ops.hadamard(q.contiguous()) if trans == "had" else q
            qtm = tk_inv_t if trans == "matmul" else None
            q_group = group if share else 1
            s = cache._specs
            dense = _dense(s["kv_data"], s["kv_param"], s["kv_indptr"], s["kv_indices"], s["last_page_offset"], layer)
            ref = _ref(qq, dense, q_group if copies == 1 else group, copies if copies > 1 else 1, qtm)
            err = (o.double() - ref).abs().amax(-1) / ref.abs().amax(-1)
            assert err.max().item() <= 3e-3, (added, layer, err.max().item())
    assert calls == [40] * (2 * layers) + [17] * (2 * layers), calls   # (plain and transposed, per layer)
    if not ragged:
        assert cache.get_seq_length() == prompt + sum(steps)


def test_a_short_step_stays_on_the_extend_launch_as_shipped(ops, monkeypatch):
    """With the constant as shipped a 4-token step never reaches ops.kv_chunk_extend, and its output is ops.kv_batch_extend's, bit for bit."""
    import flatquant_amd.deploy.transformers as TR
    from flatquant_amd.deploy.transformers import kv_cache as KC
    assert KC.EXTEND_CHUNK_MIN_TOKENS is None or KC.EXTEND_CHUNK_MIN_TOKENS >= 64

    def refuse(*a, **k):
        raise AssertionError("a 4-token step reached ops.kv_chunk_extend")
    monkeypatch.setattr(ops, "kv_chunk_extend", refuse)
    g = torch.Generator(device="cuda").manual_seed(4)
    bsz, kv_heads, group, T = 2, 2, 4, 4
    H = kv_heads * group
    cache = TR.MultiLayerPagedKVCache4Bit(bsz, 16, 64, "cuda", 1, H, HD, trans="none", group_size=group)
    cache.update(torch.randn(bsz, 30, kv_heads, HD, generator=g, device="cuda").half(), torch.randn(bsz, 30, kv_heads, HD, generator=g, device="cuda").half(), 0)
    attend = cache.update(torch.randn(bsz, T, kv_heads, HD, generator=g, device="cuda").half(),
                          torch.randn(bsz, T, kv_heads, HD, generator=g, device="cuda").half(), 0)
    q = (torch.randn(bsz, T, H, HD, generator=g, device="cuda") * 0.5).half()
    o = attend(q)
    s = cache._specs
    copies = group if cache.read_one_copy else 1
    want = ops.kv_batch_extend(q, s["kv_data"], s["kv_param"], s["kv_indptr"], s["kv_indices"], s["last_page_offset"], 0, seq_hint=cache.length,
                               kv_copies=copies)
    assert torch.equal(o, want)


def test_errors(ops):
    from flatquant_amd._lib import FqError
    g = torch.Generator(device="cuda").manual_seed(0)
    data, param, indptr, indices, last = _cache(g, [40, 50], 2, 16, False)
    q = torch.zeros(2, 3, 8, HD, dtype=torch.float16, device="cuda")
    ok = ops.kv_chunk_extend(q, data, param, indptr, indices, last, 0)
    assert ok.shape == q.shape
    for bad in (q[:1], q[:, :, :3], q[..., :64], q[:, :0], q[0]):                                   # batch, heads, head_dim, q_len, rank
        with pytest.raises(ValueError):
            ops.kv_chunk_extend(bad.contiguous(), data, param, indptr, indices, last, 0)
    with pytest.raises(ValueError):
        ops.kv_chunk_extend(q, data, param, indptr, indices, last, 0, q_trans=torch.zeros(64, 64, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):
        ops.kv_chunk_extend(q, data, param, indptr, indices, last, 0, kv_copies=2)                  # copies need query heads == cache heads
    with pytest.raises(TypeError):
        ops.kv_chunk_extend(q, data, param, indptr.long(), indices, last, 0)
    with pytest.raises(FqError, match="q_group=3"):                                                 # the library's own refusal
        ops.kv_chunk_extend(torch.zeros(2, 3, 6, HD, dtype=torch.float16, device="cuda"), data, param, indptr, indices, last, 0)
    with pytest.raises(FqError):
        ops.kv_chunk_extend(q, data, param, indptr, indices, last, 2)                               # layer index
