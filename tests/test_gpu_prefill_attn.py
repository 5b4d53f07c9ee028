"""The prompt's attention (fq_prefill_attention_f16 / ops.prefill_attention / deploy.functional.flash_attention_forward /
deploy.transformers.attention_core): causal self-attention of a prompt against dense fp64 attention at the project's attention bar; causality
and isolation bit for bit; per-request ranges (padding) against the compacted tokens; the memory contract; the Python surface fed by a real
MultiLayerPagedKVCache4Bit prompt call; argument errors."""
import pytest
import torch

from tests import guards

pytestmark = pytest.mark.gpu
HD = 128


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


def _inputs(batch, seq, heads, kv_heads, seed, trans=False):
    """q ~ 0.5 N(0,1), k ~ 1.5 N(0,1), v ~ N(0,1), an orthogonal (well-conditioned) q_trans"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = (torch.randn(batch, seq, heads, HD, generator=g, device="cuda") * 0.5).half()
    k = (torch.randn(batch, seq, kv_heads, HD, generator=g, device="cuda") * 1.5).half()
    v = torch.randn(batch, seq, kv_heads, HD, generator=g, device="cuda").half()
    qt = torch.linalg.qr(torch.randn(HD, HD, generator=g, device="cuda"))[0].half().contiguous() if trans else None
    return q, k, v, qt


def _ref(q, k, v, qt=None):
    """dense causal attention in fp64: q [b, s, H, hd], k / v [b, s, KVH, hd]; query head h reads KV head h // (H // KVH); the launch rounds
    q . q_trans to fp16 as the reference's matmul does"""
    b, s, H, hd = q.shape
    grp = H // k.shape[2]
    qq = q.double() if qt is None else torch.matmul(q.float(), qt.float()).half().double()
    kk, vv = k.double().repeat_interleave(grp, dim=2), v.double().repeat_interleave(grp, dim=2)
    x = torch.einsum("bthd,bshd->bhts", qq, kk) / hd ** 0.5
    above = torch.arange(s, device=q.device)[None, :] > torch.arange(s, device=q.device)[:, None]
    x = x.masked_fill(above[None, None], float("-inf"))
    return torch.einsum("bhts,bshd->bthd", torch.softmax(x, dim=-1), vv)


def _close(o, ref, bar=1e-3):
    """the project's attention bar (tests/test_gpu_kv_extend.py::_close): per (token, head) row, max_d |o - ref| <= bar max_d |ref|, all finite"""
    err = (o.double() - ref).abs().amax(-1)
    scale = ref.abs().amax(-1)
    print("max relative row error", (err / scale).max().item())
    assert torch.isfinite(o.float()).all()
    assert (err <= bar * scale).all(), (err / scale).max().item()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)))


# ------------------------------------------------------------------------------------------------ 1. against fp64

GEOMS = [(1, 1, 1), (2, 4, 1), (3, 8, 2), (1, 8, 8), (2, 6, 2)]        # (batch, q_heads, kv_heads); a group of 3 on purpose
SEQS = [1, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 255, 257, 300, 513]
SHAPES = [(GEOMS[i % len(GEOMS)][0], s) + GEOMS[i % len(GEOMS)][1:] for i, s in enumerate(SEQS)] + [(2, 1024, 8, 2)]


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("batch,seq,heads,kv_heads", SHAPES)
def test_prompt_attention_matches_fp64(ops, batch, seq, heads, kv_heads, trans):
    q, k, v, qt = _inputs(batch, seq, heads, kv_heads, 1000 * seq + heads, trans)
    o = ops.prefill_attention(q, k, v, qt)
    assert o.shape == q.shape and o.dtype == torch.float16 and o.is_contiguous()
    _close(o, _ref(q, k, v, qt))


# ------------------------------------------------------------------------------------------------ 2. causality and isolation, bit for bit

@pytest.mark.parametrize("trans", [False, True])
def test_causality_and_isolation_bit_for_bit(ops, trans):
    batch, seq, heads, kv_heads = 2, 300, 4, 2
    q, k, v, qt = _inputs(batch, seq, heads, kv_heads, 7, trans)
    o = ops.prefill_attention(q, k, v, qt)
    assert _same(o, ops.prefill_attention(q, k, v, qt))                                # two runs
    grp = heads // kv_heads
    assert _same(o[:, 0], v[:, 0].repeat_interleave(grp, dim=1))                        # position 0 attends itself alone: its KV head's value row
    g = torch.Generator(device="cuda").manual_seed(8)
    for p in (1, 63, 64, 129, 256, 299):                                               # k / v at position p: nothing before p moves
        k2, v2 = k.clone(), v.clone()
        k2[:, p] = (torch.randn(batch, kv_heads, HD, generator=g, device="cuda") * 3).half()
        v2[:, p] = (torch.randn(batch, kv_heads, HD, generator=g, device="cuda") * 3).half()
        o2 = ops.prefill_attention(q, k2, v2, qt)
        assert _same(o2[:, :p], o[:, :p]), p
        assert not _same(o2[:, p:], o[:, p:]), p
    q2, k2, v2 = q.clone(), k.clone(), v.clone()                                        # request 1 rewritten: request 0 stays
    for t in (q2, k2, v2):
        t[1] = (torch.randn(t.shape[1:], generator=g, device="cuda") * 2).half()
    o2 = ops.prefill_attention(q2, k2, v2, qt)
    assert _same(o2[0], o[0]) and not _same(o2[1], o[1])
    k2, v2 = k.clone(), v.clone()                                                      # KV head 1 rewritten: the heads of KV head 0 stay
    k2[:, :, 1] = (torch.randn(batch, seq, HD, generator=g, device="cuda") * 2).half()
    v2[:, :, 1] = (torch.randn(batch, seq, HD, generator=g, device="cuda") * 2).half()
    o2 = ops.prefill_attention(q, k2, v2, qt)
    assert _same(o2[:, :, :grp], o[:, :, :grp]) and not _same(o2[:, :, grp:], o[:, :, grp:])


# ------------------------------------------------------------------------------------------------ 3. ranges

def _ranges(seq):
    """left-padded, right-padded, full, length-1 and length-0 rows"""
    left, right = seq - 37 if seq > 64 else seq // 2, seq - 1 if seq < 100 else 131
    return [(seq - left, left), (0, right), (0, seq), (seq // 3, 1), (seq // 2, 0)]


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("seq", [65, 300])
def test_ranges_equal_the_compacted_requests_and_pad_with_zeros(ops, seq, trans):
    heads, kv_heads = 4, 2
    rng = _ranges(seq)
    batch = len(rng)
    q, k, v, qt = _inputs(batch, seq, heads, kv_heads, 3 * seq, trans)
    start = torch.tensor([s for s, _ in rng], dtype=torch.int32, device="cuda")
    length = torch.tensor([n for _, n in rng], dtype=torch.int32, device="cuda")
    o = ops.prefill_attention(q, k, v, qt, start, length)
    inside = torch.zeros(batch, seq, dtype=torch.bool, device="cuda")
    for b, (s, n) in enumerate(rng):
        inside[b, s:s + n] = True
        if n:
            alone = ops.prefill_attention(q[b:b + 1, s:s + n], k[b:b + 1, s:s + n], v[b:b + 1, s:s + n], qt)
            assert _same(o[b:b + 1, s:s + n], alone), (b, s, n)
    assert bool((o[~inside].view(torch.int16) == 0).all())                              # exactly zero (+0.0) outside the ranges
    _close(o[2:3], _ref(q[2:3], k[2:3], v[2:3], qt))                                    # (the full row is the plain launch's answer)
    nan = float("nan")
    qn, kn, vn = q.clone(), k.clone(), v.clone()
    for t in (qn, kn, vn):
        t[~inside] = nan
    assert _same(ops.prefill_attention(qn, kn, vn, qt, start, length), o)


# ------------------------------------------------------------------------------------------------ 4. memory contract

@pytest.mark.parametrize("seq,ranged", [(257, False), (65, True)])
def test_memory_contract(ops, seq, ranged):
    """o allocated between both poisons, the inputs between NaN pads (the ranges between valid entries): the pads stay intact and the output is
    bit-identical under both poisons and equal to the plain run — every byte of o written by the launch, nothing read outside the inputs."""
    heads, kv_heads = 4, 2
    rng = _ranges(seq) if ranged else [(0, seq), (0, seq)]
    q, k, v, qt = _inputs(len(rng), seq, heads, kv_heads, 11 * seq, True)
    start = torch.tensor([s for s, _ in rng], dtype=torch.int32, device="cuda") if ranged else None
    length = torch.tensor([n for _, n in rng], dtype=torch.int32, device="cuda") if ranged else None
    want = ops.prefill_attention(q, k, v, qt, start, length)
    torch.cuda.synchronize()
    got = []
    for poison in guards.POISONS:
        g = guards.Guard(poison)
        with g.on(ops):
            gi = [None if t is None else g.guard_input(t) for t in (q, k, v, qt, start, length)]
            got.append(ops.prefill_attention(*gi))
            torch.cuda.synchronize()
        g.check()
        assert len(g.find("empty")) == 1                                               # o, and no workspace
    assert guards.same_raw(got[0], got[1]), "differs between the two poisons: not written completely, or a pad was read"
    assert guards.same_raw(got[0], want)


# ------------------------------------------------------------------------------------------------ 5. surface

def test_flash_attention_forward_with_a_mask_is_the_ranged_launch(ops):
    from flatquant_amd.deploy.functional import flash_attention_forward, mask_ranges
    seq, heads, kv_heads = 65, 4, 2
    rng = _ranges(seq)
    q, k, v, qt = _inputs(len(rng), seq, heads, kv_heads, 5, True)
    mask = torch.zeros(len(rng), seq, dtype=torch.int64, device="cuda")
    for b, (s, n) in enumerate(rng):
        mask[b, s:s + n] = 1
    start, length = mask_ranges(mask)
    assert length.tolist() == [n for _, n in rng]
    for t in (None, qt):
        o = flash_attention_forward(q, k, v, seq, attention_mask=mask, is_causal=True, q_trans=t)
        assert _same(o, ops.prefill_attention(q, k, v, t, start, length))
        assert _same(flash_attention_forward(q, k, v, seq, q_trans=t), ops.prefill_attention(q, k, v, t))
    assert _same(flash_attention_forward(q, k, v, seq, attention_mask=mask.cpu()), ops.prefill_attention(q, k, v, None, start, length))


@pytest.mark.parametrize("trans,disable_quant", [("matmul", False), ("had", False), ("none", True)])
def test_attention_core_on_a_real_prompt_call_and_the_following_decode_step(ops, trans, disable_quant):
    """MultiLayerPagedKVCache4Bit.update()'s prompt call returns the un-quantised transformed states: attention_core runs the prompt launch on
    them (fp64 attention over the returned states, the project's bar); the next step's closure goes through attention_core unchanged."""
    import flatquant_amd.deploy.transformers as TR
    g = torch.Generator(device="cuda").manual_seed(len(trans) + 17)
    bsz, prompt, kv_heads, group, layers = 2, 37, 2, 4, 2
    H = kv_heads * group
    # (two caches fed alike: a decode step's closure may append the step's row itself and runs once, so the direct call needs its own)
    cache, twin = (TR.MultiLayerPagedKVCache4Bit(bsz, 16, 64, "cuda", layers, H, HD, disable_quant=disable_quant, trans=trans, group_size=group)
                   for _ in range(2))
    kw = {}
    if trans == "matmul":
        tk = torch.linalg.qr(torch.randn(HD, HD, generator=g, device="cuda"))[0].half()
        kw = {"trans_matrix_k": tk, "trans_matrix_k_inv_t": torch.linalg.inv(tk.float()).T.contiguous().half()}
    for layer in range(layers):
        k = (torch.randn(bsz, prompt, kv_heads, HD, generator=g, device="cuda") * 1.5).half()
        v = torch.randn(bsz, prompt, kv_heads, HD, generator=g, device="cuda").half()
        q = (torch.randn(bsz, prompt, H, HD, generator=g, device="cuda") * 0.5).half()
        out = cache.update(k, v, layer, dict(kw))
        twin.update(k, v, layer, dict(kw))
        assert isinstance(out, tuple)
        o = TR.attention_core(out, q, dict(kw))
        assert o.shape == q.shape
        _close(o, _ref(q, out[0].half(), out[1].half(), kw.get("trans_matrix_k_inv_t")))
    for layer in range(layers):
        k = (torch.randn(bsz, 1, kv_heads, HD, generator=g, device="cuda") * 1.5).half()
        v = torch.randn(bsz, 1, kv_heads, HD, generator=g, device="cuda").half()
        q = (torch.randn(bsz, 1, H, HD, generator=g, device="cuda") * 0.5).half()
        attend = cache.update(k, v, layer, dict(kw))
        assert callable(attend) and not isinstance(attend, tuple)
        o = TR.attention_core(attend, q, dict(kw))
        assert o.shape == q.shape and bool(torch.isfinite(o.float()).all())
        assert _same(o, twin.update(k, v, layer, dict(kw))(q))


def test_attention_core_passes_the_attention_mask(ops):
    import flatquant_amd.deploy.transformers as TR
    q, k, v, _ = _inputs(2, 40, 4, 2, 23)
    mask = torch.ones(2, 40, dtype=torch.int64, device="cuda")
    mask[1, :9] = 0
    o = TR.attention_core((k, v), q, {"attention_mask": mask})
    start = torch.tensor([0, 9], dtype=torch.int32, device="cuda")
    length = torch.tensor([40, 31], dtype=torch.int32, device="cuda")
    assert _same(o, ops.prefill_attention(q, k, v, None, start, length))
    assert bool((o[1, :9] == 0).all())
    _close(o[1:, 9:], _ref(q[1:, 9:], k[1:, 9:], v[1:, 9:]))


# ------------------------------------------------------------------------------------------------ 6. errors

def test_errors(ops):
    from flatquant_amd._lib import FQ_EUNSUPPORTED, FqError
    from flatquant_amd.deploy.functional import flash_attention_forward
    q, k, v, _ = _inputs(1, 8, 6, 4, 1)
    with pytest.raises(ValueError, match="multiple"):
        ops.prefill_attention(q, k, v)                                                 # 6 query heads on 4 KV heads
    h64 = torch.zeros(1, 8, 2, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(FqError) as e:
        ops.prefill_attention(h64, h64, h64)
    assert e.value.code == FQ_EUNSUPPORTED
    q, k, v, _ = _inputs(1, 8, 4, 2, 2)
    hole = torch.tensor([[1, 1, 0, 1, 1, 1, 1, 1]], device="cuda")
    with pytest.raises(NotImplementedError):
        flash_attention_forward(q, k, v, 8, attention_mask=hole)
    with pytest.raises(NotImplementedError):
        flash_attention_forward(q, k, v, 8, is_causal=False)
    with pytest.raises(NotImplementedError):
        flash_attention_forward(q[:, :1], k, v, 1)
    with pytest.raises(TypeError):
        ops.prefill_attention(q.float(), k, v)
    with pytest.raises(TypeError):
        ops.prefill_attention(q.bfloat16(), k.bfloat16(), v.bfloat16())
    with pytest.raises(ValueError):
        ops.prefill_attention(q, k, v, None, torch.zeros(1, dtype=torch.int32, device="cuda"), None)
    with pytest.raises(ValueError):
        ops.prefill_attention(q, k[:, :4], v[:, :4])
