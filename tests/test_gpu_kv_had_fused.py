"""The Hadamard rotation of the cache's default configuration (trans="had") inside the decode launch: ops.kv_decode_append(had=True),
fq_kv_decode_append_had_i4. The launch rotates its queries and the step's new K row itself; what is asserted is BIT IDENTITY with the launches it
replaces — ops.hadamard on q and k followed by the launch without ``had`` — in cache bytes, (scale, zero) pairs and attention output, on every
launch geometry, on rows that expose a wrong stage order or a wrong rounding point, through the cache class (against HAD_IN_LAUNCH = False)
and under graph capture; plus one anchor that is not launch against launch: the appended row against the numpy oracle, the output against
dense float64 attention."""
import numpy as np
import pytest
import torch

from tests import guards
from tests.test_gpu_kv_decode_append import _cache
from tests.test_gpu_rope import FUSED

pytestmark = pytest.mark.gpu
F16 = torch.float16
HD = 128


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == F16 and bool(torch.equal(a.view(torch.int16), b.view(torch.int16)))


def both_ways(ops, q, k, v, data, param, indptr, indices, last, layer, **kw):
    """-> ((o, data, param) of the launch with had=True, ... of ops.hadamard on q and k followed by the launch without)"""
    d1, p1 = data.clone(), param.clone()
    o1 = ops.kv_decode_append(ops.hadamard(q), ops.hadamard(k), v, None, d1, p1, indptr, indices, last, layer, None, **kw)
    d2, p2 = data.clone(), param.clone()
    o2 = ops.kv_decode_append(q, k, v, None, d2, p2, indptr, indices, last, layer, None, had=True, **kw)
    return (o2, d2, p2), (o1, d1, p1)


# ------------------------------------------------------------------------------------------------ 1. the launch against the launches it replaces

GEOMETRIES = FUSED + [
    (2, [600, 90], 8, 8, 1, 32, False),                               # groups of EIGHT copies (64 query heads on 8 KV heads)
    (2, [600, 90], 8, 8, 1, 32, True),                                # ... read one copy per group
    (20, [200 + i for i in range(20)], 8, 1, 8, 64, False),           # ... on the shared cache: two workgroups of four heads per group
]


@pytest.mark.parametrize("bsz,lens,src_heads,copies,q_group,page,one_copy", GEOMETRIES)
@pytest.mark.parametrize("transpose_out", [False, True])
def test_had_launch_equals_hadamard_then_decode_append(ops, bsz, lens, src_heads, copies, q_group, page, one_copy, transpose_out):
    g = torch.Generator(device="cuda").manual_seed(bsz * 1000 + lens[0] + src_heads)
    layer = 1
    cache_heads, heads = src_heads * copies, src_heads * copies * q_group
    data, param, indptr, indices, last = _cache(g, bsz, lens, cache_heads, page)
    k = (torch.randn(bsz, src_heads, HD, generator=g, device="cuda") * 2).half()
    v = (torch.randn(bsz, src_heads, HD, generator=g, device="cuda") * 2).half()
    q = (torch.randn(bsz, heads, HD, generator=g, device="cuda") * 0.5).half()
    q0, k0, v0 = q.clone(), k.clone(), v.clone()
    for split in (True, False):
        kw = dict(transpose_out=transpose_out, seq_hint=max(lens), split=split, read_one_copy=one_copy)
        (o2, d2, p2), (o1, d1, p1) = both_ways(ops, q, k, v, data, param, indptr, indices, last, layer, **kw)
        assert not torch.equal(d1, data)                       # (the step did append something)
        assert torch.equal(d2, d1), "cache bytes"
        assert torch.equal(p2.view(torch.int16), p1.view(torch.int16)), "cache parameters"
        assert bits_equal(o2, o1), "attention output"
        assert bool(torch.isfinite(o2.float()).all())
        assert bits_equal(q, q0) and bits_equal(k, k0) and bits_equal(v, v0)      # the launch rotates in LDS, never in the caller's tensors
        # ... and the rotation does matter here: the launch without it leaves another row and another output
        d3, p3 = data.clone(), param.clone()
        o3 = ops.kv_decode_append(q, k, v, None, d3, p3, indptr, indices, last, layer, None, **kw)
        assert not torch.equal(d3, d1) and not bits_equal(o3, o1)


# ------------------------------------------------------------------------------------------------ 2. rows that expose a wrong order or rounding point

def _edge_rows():
    """name -> fp16 row of 128; each would come out differently under another stage order, another operand order or another rounding point"""
    gen = torch.Generator().manual_seed(77)
    j = torch.arange(HD)
    rows = {}
    # magnitudes over 2^-10 .. 2^10: the fp32 sums round, so their ORDER shows
    rows["spread"] = (torch.randn(HD, generator=gen) * torch.exp2(torch.randint(-10, 11, (HD,), generator=gen).float())).half()
    rows["one_hot_first"] = torch.zeros(HD).half()
    rows["one_hot_first"][0] = 3.0
    rows["one_hot_odd"] = torch.zeros(HD).half()
    rows["one_hot_odd"][77] = -1.75               # every stride bit of 77 = 0b1001101 set or clear: the sign pattern is the operand order
    rows["constant"] = torch.full((HD,), 0.3).half()
    rows["alternating"] = (torch.where(j % 2 == 0, 1.0, -1.0) * 1.37).half()
    rows["subnormal"] = (torch.randint(-40, 41, (HD,), generator=gen).float() * 2.0 ** -24).half()      # fp16 subnormals: nothing may flush
    rows["zero"] = torch.zeros(HD).half()
    # +-600 in a Walsh pattern: one rotated sum is 128 * 600 = 76800 in fp32, beyond fp16 — finite only if the scale comes BEFORE the rounding
    pop = sum(((j & 5) >> b) & 1 for b in range(3))
    rows["pm600"] = (torch.where(pop % 2 == 0, 1.0, -1.0) * 600.0).half()
    rows["nan"] = torch.randn(HD, generator=gen).half()
    rows["nan"][41] = float("nan")
    return rows


def test_edge_rows_between_ordinary_rows(ops):
    rows = _edge_rows()
    names = ["spread", "one_hot_first", "one_hot_odd", "constant", "alternating", "subnormal", "zero", "pm600"]
    lens = list(range(17, 25))
    bsz, src_heads, page, layer = len(lens), 3, 16, 0
    assert len(names) == bsz
    g = torch.Generator(device="cuda").manual_seed(21)
    data, param, indptr, indices, last = _cache(g, bsz, lens, src_heads, page)
    k = (torch.randn(bsz, src_heads, HD, generator=g, device="cuda") * 2).half()
    v = (torch.randn(bsz, src_heads, HD, generator=g, device="cuda") * 2).half()
    q = (torch.randn(bsz, src_heads, HD, generator=g, device="cuda") * 0.5).half()
    for b, name in enumerate(names):               # head 1 of every request: the edge row, between the ordinary rows of heads 0 and 2
        k[b, 1] = rows[name].cuda()
        if name == "zero":
            v[b, 1] = 0
        if name != "pm600":                        # (a query of +-600 would only overflow the scores)
            q[b, 1] = rows[name].cuda()
    # the standalone rotation of these rows is the oracle's, so the comparison below is against the pinned arithmetic
    from oracle import fq_oracle as O
    want_k = O.hadamard(k.reshape(-1, HD).cpu().numpy())
    assert np.array_equal(ops.hadamard(k).reshape(-1, HD).cpu().numpy().view(np.int16), want_k.view(np.int16))
    assert np.isfinite(want_k.astype(np.float32)).all() and np.abs(want_k.astype(np.float32)).max() > 6000      # (the +-600 row: 76800 / sqrt(128))
    for split in (True, False):
        (o2, d2, p2), (o1, d1, p1) = both_ways(ops, q, k, v, data, param, indptr, indices, last, layer, split=split, seq_hint=max(lens))
        assert torch.equal(d2, d1) and torch.equal(p2.view(torch.int16), p1.view(torch.int16)) and bits_equal(o2, o1)
        assert bool(torch.isfinite(o2.float()).all())
    # a NaN row: its own digits are not asserted, every row next to it is as without it
    kn = k.clone()
    kn[3, 1] = rows["nan"].cuda()
    (o2, d2, p2), (o1, d1, p1) = both_ways(ops, q, kn, v, data, param, indptr, indices, last, layer, seq_hint=max(lens))
    (oc, dc, pc), _ = both_ways(ops, q, k, v, data, param, indptr, indices, last, layer, seq_hint=max(lens))
    pg = int(indices[int(indptr[3]) + (lens[3] - 1) // page])
    keep_d = torch.ones(data.shape[:-1], dtype=torch.bool, device="cuda")
    keep_d[pg, layer, 0, 1, (lens[3] - 1) % page] = False
    keep_o = torch.ones(bsz, src_heads, dtype=torch.bool, device="cuda")
    keep_o[3, 1] = False
    for d, p, o in ((d2, p2, o2), (d1, p1, o1)):
        assert torch.equal(d[keep_d], dc[keep_d]) and torch.equal(p.view(torch.int16)[keep_d], pc.view(torch.int16)[keep_d])
        assert torch.equal(o.view(torch.int16)[keep_o], oc.view(torch.int16)[keep_o])


# ------------------------------------------------------------------------------------------------ 3. an anchor that is not launch against launch

def test_appended_row_is_the_oracles_and_the_output_is_dense_attention(ops):
    from oracle import fq_oracle as O
    lens, src_heads, page, layer = [1, 16, 17], 2, 16, 1
    bsz = len(lens)
    g = torch.Generator(device="cuda").manual_seed(31)
    data, param, indptr, indices, last = _cache(g, bsz, lens, src_heads, page)
    k = (torch.randn(bsz, src_heads, HD, generator=g, device="cuda") * 2).half()
    v = (torch.randn(bsz, src_heads, HD, generator=g, device="cuda") * 2).half()
    q = (torch.randn(bsz, src_heads, HD, generator=g, device="cuda") * 0.5).half()
    o = ops.kv_decode_append(q, k, v, None, data, param, indptr, indices, last, layer, had=True, seq_hint=max(lens))
    d, p, o = data.cpu().numpy(), param.cpu().numpy(), o.cpu().numpy().astype(np.float64)
    ip, ix = indptr.cpu().numpy(), indices.cpu().numpy()
    k_rot = O.hadamard(k.reshape(-1, HD).cpu().numpy())
    q_rot = O.hadamard(q.reshape(-1, HD).cpu().numpy()).astype(np.float64).reshape(bsz, src_heads, HD)
    packed, scale, zero, _ = O.kv_asym_quant(k_rot)
    packed_v, scale_v, zero_v, _ = O.kv_asym_quant(v.reshape(-1, HD).cpu().numpy())

    def deq(p8, par):
        n = np.stack((p8 & 15, p8 >> 4), axis=-1).reshape(p8.shape[0], -1).astype(np.float64)
        return n * par[:, :1].astype(np.float64) - par[:, 1:].astype(np.float64)

    for b, n in enumerate(lens):
        pages = ix[ip[b]:ip[b + 1]]
        pg, ent = pages[(n - 1) // page], (n - 1) % page
        for h in range(src_heads):
            r = b * src_heads + h
            assert np.array_equal(d[pg, layer, 0, h, ent], packed[r]), (b, h)
            assert np.array_equal(p[pg, layer, 0, h, ent].view(np.int16), np.array([scale[r, 0], zero[r, 0]], dtype=np.float16).view(np.int16)), (b, h)
            assert np.array_equal(d[pg, layer, 1, h, ent], packed_v[r]), (b, h)                          # V is never rotated
            assert np.array_equal(p[pg, layer, 1, h, ent].view(np.int16), np.array([scale_v[r, 0], zero_v[r, 0]], dtype=np.float16).view(np.int16)), (b, h)
            K = deq(d[pages, layer, 0, h].reshape(-1, HD // 2)[:n], p[pages, layer, 0, h].reshape(-1, 2)[:n])
            V = deq(d[pages, layer, 1, h].reshape(-1, HD // 2)[:n], p[pages, layer, 1, h].reshape(-1, 2)[:n])
            x = K @ q_rot[b, h] / np.sqrt(HD)
            w = np.exp(x - x.max())
            ref = (w / w.sum()) @ V
            err = np.abs(o[b, h] - ref).max() / np.abs(ref).max()
            assert err <= 3e-3, (b, h, err)


# ------------------------------------------------------------------------------------------------ 4. the cache class

VARIANTS = {
    # name: (requests, constructor options, HAD_FUSE_MAX_FOUR_HEAD_WGS for the test or None)
    "plain": (3, dict(), None),
    "shared_heads": (3, dict(share_kv_heads=True), None),
    "four_heads": (4, dict(), None),                 # 32 (request, KV head) pairs: the launch that serves four query heads per workgroup
    "four_heads_shared": (4, dict(share_kv_heads=True), None),
    "four_heads_beyond_the_bound": (4, dict(), 16),  # ... more such workgroups than the bound: the two launches in front of the fused append, as before
}
STAYS = {
    # routes that keep their ops.hadamard launches: name -> (constructor options, ragged mask, FUSE_APPEND_MAX_PAIRS for the test or None)
    "fuse_append_off": (dict(fuse_append=False), False, None),
    "too_many_pairs": (dict(), False, 8),
    "fp16_pages": (dict(disable_quant=True), False, None),
    "ragged_mask": (dict(), True, None),
}
STEPS = 3


def _run_cache(ops, bsz, opts, call_all, ragged=False):
    """a prompt of 13 tokens and three decode steps at trans="had" -> (outputs, pages, scales, ops.hadamard calls of the steps, had=True launches)"""
    import flatquant_amd.deploy.transformers as T
    heads, kv_heads, page, prompt = 32, 8, 16, 13
    g = torch.Generator(device="cuda").manual_seed(11)
    cache = T.MultiLayerPagedKVCache4Bit(bsz, page, 64, torch.device("cuda"), 1, heads, HD, trans="had", group_size=heads // kv_heads, **opts)
    cache._pages.fill_(0x11 if not cache.disable_quant else 0.5), cache._scales.fill_(0.25)       # (torch.empty: equal bytes wherever nothing is appended)
    valid = [prompt, prompt - 4, prompt - 9, prompt][:bsz] if ragged else [prompt] * bsz
    mask = torch.zeros(bsz, prompt, dtype=torch.int64, device="cuda")
    for i, n in enumerate(valid):
        mask[i, prompt - n:] = 1
    calls = {"hadamard": 0, "had_launch": 0}
    real_had, real_fused = ops.hadamard, ops.kv_decode_append

    def counted_had(*a, **k):
        calls["hadamard"] += 1
        return real_had(*a, **k)

    def counted_fused(*a, **k):
        calls["had_launch"] += bool(k.get("had"))
        return real_fused(*a, **k)

    outs = []
    with torch.no_grad():
        k = torch.randn(bsz, prompt, kv_heads, HD, generator=g, device="cuda").half()
        v = torch.randn(bsz, prompt, kv_heads, HD, generator=g, device="cuda").half()
        outs += list(cache.update(k, v, 0, {"attention_mask": mask} if ragged else {}))        # (the prompt's rotation is not counted)
        ops.hadamard, ops.kv_decode_append = counted_had, counted_fused
        try:
            for si in range(STEPS):
                if ragged:
                    mask = torch.cat([mask, torch.ones(bsz, 1, dtype=mask.dtype, device="cuda")], dim=1)
                k = torch.randn(bsz, 1, kv_heads, HD, generator=g, device="cuda").half()
                v = torch.randn(bsz, 1, kv_heads, HD, generator=g, device="cuda").half()
                q = (torch.randn(bsz, 1, heads, HD, generator=g, device="cuda") * 0.5).half()
                att = cache.update(k, v, 0, {"attention_mask": mask} if ragged else {})
                if call_all or si != 1:                    # (the middle step's closure is dropped: its row reaches the cache through _flush_pending)
                    outs.append(att(q, transposed=(si == 2)))
            pages, scales = cache.pages.clone(), cache.scales.clone()
        finally:
            ops.hadamard, ops.kv_decode_append = real_had, real_fused
    return outs, pages, scales, calls["hadamard"], calls["had_launch"]


def _same_run(a, b):
    assert len(a[0]) == len(b[0]) and len(a[0]) >= 4
    for x, y in zip(a[0], b[0]):
        assert x.shape == y.shape and torch.equal(x.view(torch.int16), y.view(torch.int16))
        assert bool(torch.isfinite(x.float()).all())
    assert guards.same_raw(a[1], b[1]) and guards.same_raw(a[2], b[2])


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("call_all", [True, False])
def test_cache_class_rotates_in_the_launch(ops, monkeypatch, variant, call_all):
    from flatquant_amd.deploy.transformers import kv_cache as kvc
    bsz, opts, bound = VARIANTS[variant]
    assert kvc.HAD_IN_LAUNCH is True and kvc.HAD_FUSE_MAX_FOUR_HEAD_WGS >= 32       # (the four-head variants here are 32 such workgroups)
    if bound is not None:
        monkeypatch.setattr(kvc, "HAD_FUSE_MAX_FOUR_HEAD_WGS", bound)
    got = _run_cache(ops, bsz, opts, call_all)
    monkeypatch.setattr(kvc, "HAD_IN_LAUNCH", False)
    want = _run_cache(ops, bsz, opts, call_all)
    _same_run(got, want)
    if bound is not None:                            # beyond the bound: the route of HAD_IN_LAUNCH = False, launch for launch
        assert got[3] == want[3] == (2 * STEPS if call_all else 2 * STEPS - 1) and got[4] == want[4] == 0
        return
    # no launch of its own for the rotation when every closure is called; an un-called closure's row is rotated once by _flush_pending
    assert got[3] == (0 if call_all else 1)
    assert got[4] == (STEPS if call_all else STEPS - 1)
    # ... where the two-launch form pays one for the keys in every update and one for the queries in every closure
    assert want[3] == (2 * STEPS if call_all else 2 * STEPS - 1) and want[4] == 0


@pytest.mark.parametrize("route", sorted(STAYS))
def test_other_routes_keep_their_hadamard_launches(ops, monkeypatch, route):
    from flatquant_amd.deploy.transformers import kv_cache as kvc
    opts, ragged, bound = STAYS[route]
    if bound is not None:
        monkeypatch.setattr(kvc, "FUSE_APPEND_MAX_PAIRS", bound)
    got = _run_cache(ops, 3, opts, True, ragged)
    monkeypatch.setattr(kvc, "HAD_IN_LAUNCH", False)
    want = _run_cache(ops, 3, opts, True, ragged)
    _same_run(got, want)
    assert got[3] == want[3] == 2 * STEPS and got[4] == want[4] == 0


# ------------------------------------------------------------------------------------------------ 5. the captured step

@pytest.mark.parametrize("bsz", [1, 3])
def test_graphed_decode_with_the_rotation_in_the_launch(ops, bsz):
    """two warm-ups, one capture, six replays of ``cache.update(k, v, 0, kw)(q)`` at trans="had", across a page boundary (lengths 11 .. 19, pages
    of 16): every output and every appended row equal the eager twin's — the graph reads k and q themselves, no rotated copy of them"""
    import flatquant_amd.deploy as deploy
    import flatquant_amd.deploy.transformers as T
    heads, kv_heads, page, prompt = 32, 8, 16, 10
    g = torch.Generator(device="cuda").manual_seed(60 + bsz)

    def new():
        c = T.MultiLayerPagedKVCache4Bit(bsz, page, 64, torch.device("cuda"), 1, heads, HD, trans="had", group_size=heads // kv_heads)
        c._pages.fill_(0x11), c._scales.fill_(0.25)
        return c

    def fn(q, k, v, cache):
        return cache.update(k, v, 0, {})(q)

    launches = []
    real = ops.kv_decode_append
    ops.kv_decode_append = lambda *a, **k: (launches.append(bool(k.get("had"))), real(*a, **k))[1]
    try:
        with torch.no_grad():
            cache, twin = new(), new()
            k0 = torch.randn(bsz, prompt, kv_heads, HD, generator=g, device="cuda").half()
            v0 = torch.randn(bsz, prompt, kv_heads, HD, generator=g, device="cuda").half()
            for c in (cache, twin):
                c.update(k0, v0, 0, {})
            gd = deploy.GraphedDecode(fn)
            for i in range(9):
                k = torch.randn(bsz, 1, kv_heads, HD, generator=g, device="cuda").half()
                v = torch.randn(bsz, 1, kv_heads, HD, generator=g, device="cuda").half()
                q = (torch.randn(bsz, 1, heads, HD, generator=g, device="cuda") * 0.5).half()
                got = gd(q, k, v, cache)
                want = fn(q, k, v, twin)
                assert cache.length == twin.length == prompt + i + 1
                assert torch.equal(got.view(torch.int16), want.view(torch.int16)), i
                assert guards.same_raw(cache.pages, twin.pages) and guards.same_raw(cache.scales, twin.scales), i
            assert gd.captures == 1 and gd.eager_calls == 2 and gd.replays >= 6
            assert (prompt + 9 - 1) // page > prompt // page      # (a page boundary was crossed)
    finally:
        ops.kv_decode_append = real
    assert launches and all(launches)                             # every step, captured or eager, ran the launch that rotates


# ------------------------------------------------------------------------------------------------ 6. refusals

def test_had_excludes_the_other_transforms_and_unsupported_geometries(ops):
    from flatquant_amd import _lib
    g = torch.Generator(device="cuda").manual_seed(3)
    data, param, indptr, indices, last = _cache(g, 2, [20, 21], 2, 16)
    q = torch.randn(2, 2, HD, generator=g, device="cuda").half()
    k = torch.randn(2, 2, HD, generator=g, device="cuda").half()
    T = (torch.randn(HD, HD, generator=g, device="cuda") / HD ** 0.5).half()
    cos = torch.rand(2, HD, generator=g, device="cuda").half()
    before = data.clone()
    with pytest.raises(ValueError):
        ops.kv_decode_append(q, k, k, T, data, param, indptr, indices, last, 0, had=True)
    with pytest.raises(ValueError):
        ops.kv_decode_append(q, k, k, None, data, param, indptr, indices, last, 0, T, had=True)
    with pytest.raises(ValueError):
        ops.kv_decode_append(q, k, k, None, data, param, indptr, indices, last, 0, rope=(cos, cos), had=True)
    assert torch.equal(data, before)
    d8, p8, ip8, ix8, la8 = _cache(g, 1, [20], 2, 8)                         # page_size 8: a wave's 16 rows straddle pages
    with pytest.raises(_lib.FqError) as e:
        ops.kv_decode_append(q[:1].contiguous(), k[:1].contiguous(), k[:1].contiguous(), None, d8, p8, ip8, ix8, la8, 0, had=True)
    assert e.value.code == _lib.FQ_EUNSUPPORTED
    d64, p64, ip64, ix64, la64 = _cache(g, 1, [20], 2, 16, hd=64)            # head_dim 64
    q64 = torch.randn(1, 2, 64, generator=g, device="cuda").half()
    with pytest.raises(_lib.FqError) as e:
        ops.kv_decode_append(q64, q64, q64, None, d64, p64, ip64, ix64, la64, 0, had=True)
    assert e.value.code == _lib.FQ_EUNSUPPORTED
    f16_pages = torch.zeros(2, 2, 2, 2, 16, HD, dtype=F16, device="cuda")    # the fp16 configuration
    assert not ops.kv_decode_append_supported(f16_pages, 2)
    refused = []
    for had in (False, True):                                                # refused as the plain launch refuses them: before anything is launched
        with pytest.raises((_lib.FqError, TypeError)) as e:
            ops.kv_decode_append(q[:1].contiguous(), k[:1].contiguous(), k[:1].contiguous(), None, f16_pages, p8, ip8, ix8, la8, 0, had=had)
        refused.append(type(e.value))
    assert refused[0] is refused[1]
