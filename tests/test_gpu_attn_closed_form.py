"""Every attention launch on inputs whose softmax is known exactly (tests/attn_closed_form.py): fq_prefill_attention_f16,
fq_kv_chunk_extend, fq_kv_batch_extend, the fq_kv_batch_decode* family, fq_kv_decode_append[_had]_i4 and MultiLayerPagedKVCache4Bit through
attention_core. The weights are exactly 0 or exactly equal, so token t must return the mean of V over a known set of rows: all finite, singleton
sets on fp16 values bit for bit, everything else within the derived bounds 3 / 4 of that module, two launches bit-identical. Nothing is
masked or left out."""
import functools

import numpy as np
import pytest
import torch

from tests import attn_closed_form as A
from tests import kv_edge_rows as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _tensors(cache):
    return tuple(_t(x) for x in (cache.data, cache.param, cache.indptr, cache.indices, cache.last))


def _hold(o, case, bits, what=""):
    o = o.cpu().numpy()
    bad = A.check(o, case) + (A.check_bits(o, case) if bits else [])
    assert not bad, f"{what}: " + "; ".join(bad)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)))


# ------------------------------------------------------------------------------------------------ the prompt launch

def _prefill(ops, c):
    return ops.prefill_attention(_t(c["q"]), _t(c["k"]), _t(c["v"]), _t(c["qt"]))


@pytest.mark.parametrize("name", [n for n, _ in A.PREFILL_CASES])
def test_prompt_launch(ops, name):
    c = A.prefill_case(**dict(A.PREFILL_CASES)[name])
    o = _prefill(ops, c)
    _hold(o, c, True, name)
    assert _same(o, _prefill(ops, c))


def test_prompt_launch_ranged(ops):
    """left padding, a full row, a length-1 and a length-0 request: inside a range the compacted request's closed form, outside it +0.0"""
    c = A.prefill_case(**A.PREFILL_RANGED)
    kw = A.PREFILL_RANGED
    run = lambda: ops.prefill_attention(_t(c["q"]), _t(c["k"]), _t(c["v"]), None, _t(np.array(kw["start"], np.int32)), _t(np.array(kw["seqs"], np.int32)))
    o = run()
    _hold(o, c, True, "ranged")
    assert bool((o.cpu()[torch.from_numpy(~c["inside"])].view(torch.int16) == 0).all())
    assert _same(o, run())


def test_prompt_launch_uniform_with_zero_queries_equals_level_0_keys(ops):
    a, b = A.prefill_case(**A.PREFILL_UNIFORM), A.prefill_case(**A.PREFILL_UNIFORM, level0=True)
    assert not np.array_equal(a["q"], b["q"]) and np.array_equal(a["e"], b["e"])
    assert _same(_prefill(ops, a), _prefill(ops, b))


# ------------------------------------------------------------------------------------------------ the two extend launches

@functools.lru_cache(maxsize=None)
def _extend_case(name):
    return A.paged_case(**(A.EXTEND_CASES.get(name) or A.RISER_EXTEND[name]))


# fq_kv_batch_extend and the decode's four-head launch put fp16(256 p s_v) on the matrix pipe, p relative to a reference 2^8 above the score that
# last moved it: finite while p s_v < 256 (their documented limit; the per-row power of two that lifts it costs more than the launches'
# run-to-run spread: profiles/attn_closed_form.txt). Every riser combination is a launch of its own there, and exactly the launches whose riser
# has p s_v >= 256 against row 0's reference are expected to fail.
_XFAIL = "fp16(256 p s_v) overflows on the matrix pipe: the launch's documented limit p s_v < 256"


def _riser_mark(route, name):
    k = int(name.split("riser")[1].split("-")[0])
    return [pytest.mark.xfail(strict=True, reason=_XFAIL)] if k in A.MARGIN_OVERFLOW[route] else []


def _extend_params():
    """every case on the chunk launch; on the extend launch every case but the two launches that mix riser combinations, which it meets one by one"""
    out = [pytest.param(n, r, id=f"{n}-{r}") for r in ("chunk", "extend", "extend-split") for n in A.EXTEND_CASES if r == "chunk" or "riser" not in n]
    return out + [pytest.param(n, r, id=f"{n}-{r}", marks=_riser_mark(r, n)) for r in ("extend", "extend-split") for n in A.RISER_EXTEND]


def _extend(ops, c, route, transpose_out=False):
    args = (_t(c["q"]), *_tensors(c["cache"]), c["cache"].layer, _t(c["qt"]), transpose_out)
    if route == "chunk":
        o = ops.kv_chunk_extend(*args, kv_copies=c["copies"])
    else:
        o = ops.kv_batch_extend(*args, seq_hint=max(c["cache"].lens), split=route == "extend-split", kv_copies=c["copies"])
    return o.transpose(-1, -2) if transpose_out else o


@pytest.mark.parametrize("name,route", _extend_params())
def test_extend_launches(ops, name, route):
    c = _extend_case(name)
    o = _extend(ops, c, route)
    _hold(o, c, True, f"{name} {route}")
    assert _same(o, _extend(ops, c, route))


@pytest.mark.parametrize("route", ["chunk", "extend"])
def test_extend_launches_transposed_output(ops, route):
    c = _extend_case("i4-L200-T71-g8-p16")
    o = _extend(ops, c, route, True)
    _hold(o, c, True, route)
    assert _same(o, _extend(ops, c, route, True))


@pytest.mark.parametrize("route", ["chunk", "extend", "extend-split"])
def test_extend_uniform_with_zero_queries_equals_level_0_keys(ops, route):
    a, b = A.paged_case(**A.EXTEND_UNIFORM), A.paged_case(**A.EXTEND_UNIFORM, level0=True)
    assert not np.array_equal(a["q"], b["q"]) and np.array_equal(a["e"], b["e"])
    assert _same(_extend(ops, a, route), _extend(ops, b, route))


# ------------------------------------------------------------------------------------------------ the decode launches

def _decode(ops, c, kw):
    return ops.kv_batch_decode(_t(c["q"][:, 0]), *_tensors(c["cache"]), c["cache"].layer, _t(c["qt"]), kv_copies=c["copies"], **kw)


@pytest.mark.parametrize("name", [pytest.param(n, id=n, marks=_riser_mark("g4", n) if n.endswith("-g4") and "riser" in n else []) for n in A.DECODE_CASES])
def test_decode_launches(ops, name):
    kw, run = A.DECODE_CASES[name]
    c = A.paged_case(**kw)
    o = _decode(ops, c, run)
    # (split and merged routes add their states in fp32: the bound, not bit equality)
    _hold(o[:, None], c, "per-head" in name or name.endswith("hd128-ends") or name.endswith("hd64-ends"), name)
    assert _same(o, _decode(ops, c, run))


def test_decode_uniform_with_zero_queries_equals_level_0_keys(ops):
    a, b = A.paged_case(**A.DECODE_UNIFORM), A.paged_case(**A.DECODE_UNIFORM, level0=True)
    assert not np.array_equal(a["q"], b["q"]) and np.array_equal(a["e"], b["e"])
    assert _same(_decode(ops, a, dict(split=False)), _decode(ops, b, dict(split=False)))


# ------------------------------------------------------------------------------------------------ rows the cache's own quantiser wrote

ROUND_TRIP = ["outlier_15000", "gauss_1e-3", "gauss_1e-6", "lone_subnormal", "const_7", "const_-8_one_7", "ties", "tiny_171", "tiny_-172",
              "const_1000_one_ulp", "one_plus_3e-5", "top_65504", "positive", "negative"]
# (the quantiser's row for top_65504 de-quantises to 65520.9 at the 65504: the one answer outside fp16's range, where the output must be 65504 or +Inf)


@functools.lru_cache(maxsize=None)
def _round_trip():
    """request b holds the ROUND_TRIP rows as V, appended by ops.kv_quant_append; its K rows are one_hot(b). The expectation is read from the
    bytes the quantiser wrote: token 0 (the one query) sees every row and attends row b alone."""
    from flatquant_amd import ops
    n, hd, page, heads = len(ROUND_TRIP), 128, 16, 2
    rows = E.edge_rows(hd)[[E.ROW[r] for r in ROUND_TRIP]]
    cache = A.Cache([n] * n, heads, page, hd, False, 70, layers=1, layer=0)
    k = np.zeros((n, n, heads, hd), A.F16)
    for b in range(n):
        k[b, b, :, A.FEATURES[hd][b % 3]] = A.K_F16
    v = np.broadcast_to(rows[None, :, None, :], k.shape).copy()
    data, param, indptr, indices, last = _tensors(cache)
    ops.kv_quant_append(_t(k), _t(v), None, data, param, indptr, indices, last, 0)
    wrote = A.Cache.view(data.cpu().numpy(), param.cpu().numpy(), cache.indptr, cache.indices, cache.last, 0)
    H = 4
    q = np.zeros((n, 1, H, hd), A.F16)
    e, tol, size = np.zeros((n, 1, H, hd)), np.zeros((n, 1, H, hd)), np.zeros((n, 1, H), np.int64)
    for b in range(n):
        q[b, 0, :, A.FEATURES[hd][b % 3]] = A.Q_F16
        for h in range(H):
            k64, _, _, _ = wrote.dense(b, h // 2, 0)
            v64, nib, s, z = wrote.dense(b, h // 2, 1)
            r = A.expect(q[b, :, h], k64, v64, np.array([n - 1]), hd, nib, s, z)
            assert r["S"][0].sum() == 1 and r["S"][0, b] and np.isfinite(r["e"]).all()
            e[b, :, h], tol[b, :, h], size[b, :, h] = r["e"], r["tol"], r["size"]
    over = np.abs(e) > 65504
    assert over.sum() == H and (e[over] > 0).all() and over[ROUND_TRIP.index("top_65504")].sum() == H      # (the one element, once per query head)
    return dict(q=q, e=e, tol=tol, size=size, over=over, f16=False, tensors=(data, param, indptr, indices, last))


@pytest.mark.parametrize("route", ["chunk", "extend", "extend-split", "decode", "decode-split"])
def test_round_trip_of_the_quantisers_edge_rows(ops, route):
    c = _round_trip()
    q = _t(c["q"])
    if route == "chunk":
        run = lambda: ops.kv_chunk_extend(q, *c["tensors"], 0)
    elif route.startswith("extend"):
        run = lambda: ops.kv_batch_extend(q, *c["tensors"], 0, split=route == "extend-split", seq_hint=len(ROUND_TRIP))
    else:
        run = lambda: ops.kv_batch_decode(q[:, 0], *c["tensors"], 0, split=route == "decode-split", seq_hint=2048)[:, None]
    o = run()
    got = o.cpu().numpy().copy()
    assert np.isin(got[c["over"]], [np.float16(65504), np.float16(np.inf)]).all(), got[c["over"]]
    got[c["over"]] = 65504                                       # (held above; everything else to its bound)
    bad = A.check(got, dict(c, e=np.where(c["over"], 65504.0, c["e"])))
    assert not bad, f"{route}: " + "; ".join(bad)
    assert _same(o, run())


# ------------------------------------------------------------------------------------------------ the decode launch that appends its own row

@pytest.mark.parametrize("had", [False, True], ids=["plain", "had"])
def test_decode_append_attends_its_own_row(ops, had):
    """Cached rows at level 0 (K = 0); the step's own row is the dominant one: K one-hot at c (had: the rotation's image of a one-hot row,
    which the launch rotates back), V integers 0 .. 15 times a power of two (quantised exactly). The expectation is read from the cache bytes
    after the launch, the sets from the fp64 scores of those bytes (GAP asserted)."""
    hd, page, kvh, G = 128, 16, 2, 4
    lens = [300, 17, 33, 64]
    rng = np.random.default_rng(90 + had)
    cache = A.Cache(lens, kvh, page, hd, False, 91, layers=1, layer=0)
    for b, L in enumerate(lens):
        for y in range(kvh):
            cache.put(b, y, 0, *A.keys_i4(np.zeros(L, np.int64), 0, hd, 0.0))
            cache.put(b, y, 1, *A.v_i4(rng, L, hd))
    k_new, q = np.zeros((len(lens), kvh, hd), A.F16), np.zeros((len(lens), kvh * G, hd), A.F16)
    v_new = (rng.integers(0, 16, (len(lens), kvh, hd)) * 2.0 ** rng.integers(-3, 4, (len(lens), kvh, 1))).astype(A.F16)
    for b in range(len(lens)):
        for y in range(kvh):
            c = A.FEATURES[hd][(b + y) % 3]
            k_new[b, y, c] = A.K_F16
            q[b, y * G:(y + 1) * G, c] = A.Q_F16
    qd, kd = _t(q), _t(k_new)
    if had:                                                       # H (H e_c) = e_c: the launch's rotation turns these back into one-hot rows
        qd, kd = ops.hadamard(qd), ops.hadamard(kd)
    data, param, indptr, indices, last = _tensors(cache)
    o = ops.kv_decode_append(qd, kd, _t(v_new), None, data, param, indptr, indices, last, 0, had=had)
    wrote = A.Cache.view(data.cpu().numpy(), param.cpu().numpy(), cache.indptr, cache.indices, cache.last, 0)
    q_seen = (ops.hadamard(qd) if had else qd).cpu().numpy()
    case = dict(e=np.zeros(q.shape), tol=np.zeros(q.shape), size=np.zeros(q.shape[:2], np.int64))
    for b, L in enumerate(lens):
        for h in range(kvh * G):
            k64, _, _, _ = wrote.dense(b, h // G, 0)
            v64, nib, s, z = wrote.dense(b, h // G, 1)
            r = A.expect(q_seen[b, h][None], k64, v64, np.array([L - 1]), hd, nib, s, z)
            assert r["S"][0].sum() == 1 and r["S"][0, L - 1]
            assert np.array_equal(v64[L - 1], v_new[b, h // G].astype(np.float64))        # (the payload's quantisation is exact)
            case["e"][b, h], case["tol"][b, h] = r["e"][0], r["tol"][0]
    _hold(o, case, False, "decode_append")


# ------------------------------------------------------------------------------------------------ the cache class

def test_cache_class_prompt_and_two_decode_steps(ops):
    """MultiLayerPagedKVCache4Bit(trans="none"): a prompt and two decode steps with sink (request 0) and staircase (request 1) keys through
    attention_core. The prompt call attends the un-quantised states (bit equality with the V rows); the decode steps' expectation is read from the
    cache bytes."""
    import flatquant_amd.deploy.transformers as TR
    hd, kvh, G, prompt, page = 128, 2, 4, 37, 16
    H = kvh * G
    rng = np.random.default_rng(95)
    cache = TR.MultiLayerPagedKVCache4Bit(2, page, 64, "cuda", 1, H, hd, trans="none", group_size=G)
    total = prompt + 2
    lev = [A.levels("sink", total), A.levels("staircase", total)]
    cs = [A.FEATURES[hd][0], A.FEATURES[hd][1]]
    k = np.stack([np.broadcast_to(A.keys_f16(lev[b], cs[b], hd)[:, None], (total, kvh, hd)) for b in range(2)]).copy()
    v = rng.integers(-8, 9, (2, total, kvh, hd)).astype(A.F16)
    q = np.zeros((2, total, H, hd), A.F16)
    for b in range(2):
        q[b, :, :, cs[b]] = A.Q_F16
    out = cache.update(_t(k[:, :prompt]), _t(v[:, :prompt]), 0)
    o = TR.attention_core(out, _t(q[:, :prompt]))
    case = dict(e=np.zeros((2, prompt, H, hd)), tol=np.zeros((2, prompt, H, hd)), size=np.zeros((2, prompt, H), np.int64))
    ks, vs = out[0].half().cpu().numpy(), out[1].half().cpu().numpy()
    for b in range(2):
        for h in range(H):
            r = A.expect(q[b, :prompt, h], ks[b, :, h // G].astype(np.float64), vs[b, :, h // G].astype(np.float64), np.arange(prompt), hd)
            case["e"][b, :, h], case["tol"][b, :, h], case["size"][b, :, h] = r["e"], r["tol"], r["size"]
    _hold(o, case, True, "prompt")
    assert _same(o, TR.attention_core(out, _t(q[:, :prompt])))
    for step in range(2):
        t = prompt + step
        attend = cache.update(_t(k[:, t:t + 1]), _t(v[:, t:t + 1]), 0)
        o = TR.attention_core(attend, _t(q[:, t:t + 1]))
        s = cache._specs
        wrote = A.Cache.view(cache.pages.cpu().numpy(), cache.scales.cpu().numpy(), s["kv_indptr"].cpu().numpy(), s["kv_indices"].cpu().numpy(),
                             s["last_page_offset"].cpu().numpy(), 0)
        assert wrote.lens == [t + 1, t + 1]
        case = dict(e=np.zeros((2, 1, H, hd)), tol=np.zeros((2, 1, H, hd)), size=np.zeros((2, 1, H), np.int64))
        for b in range(2):
            for h in range(H):
                k64, _, _, _ = wrote.dense(b, h, 0)
                v64, nib, sc, z = wrote.dense(b, h, 1)
                r = A.expect(q[b, t:t + 1, h], k64, v64, np.array([t]), hd, nib, sc, z)
                assert r["S"][0].sum() == 1 and r["S"][0, 0 if b == 0 else t]
                case["e"][b, :, h], case["tol"][b, :, h] = r["e"], r["tol"]
        _hold(o, case, False, f"decode step {step}")
