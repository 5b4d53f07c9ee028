"""deploy.GraphedDecode's host logic — "does this captured graph still belong to this cache?" — on real cache objects, without a GPU.

A replayed graph holds raw device pointers into a paged KV cache (pages, scales, index tensors). Which cache an entry belongs to is decided on the
host, by the signature (``_cache_token``), by ``_Entry.matches`` and by what happens to the wrapper's tables when a cache dies. Those pieces are
pure Python over attributes of the cache, and MultiLayerPagedKVCache4Bit(device="cpu") runs its host step without a device, so they are tested
here; the launches themselves are tests/test_gpu_graphed.py's."""
import gc

import pytest
import torch

from flatquant_amd import ops
from flatquant_amd.deploy import graphed
from flatquant_amd.deploy.transformers import MultiLayerPagedKVCache4Bit, kv_cache


def new_cache(bsz=2, max_len=64):
    """a cache after its prefill and one decode step's host side: generation 1, like every cache a serving loop hands to the wrapper"""
    c = MultiLayerPagedKVCache4Bit(bsz, 16, max_len, "cpu", 1, 4, 128, trans="none")
    c._needs_init = [False]
    c.length = 21
    c._host_step(0, 1)
    return c


def entry_for(*caches):
    """an entry as GraphedDecode._capture leaves it, minus the graph"""
    ent = graphed._Entry()
    ent.logs = [[(0, 1)] for _ in caches]
    ent.bind(list(caches), ops.cache_epoch())
    return ent


def sig_with(cache, extra=0):
    """a signature as _split builds it: (spec, one tensor's (shape, dtype, device), the cache's token, a scalar)"""
    return ("spec", ((2, 1, 64), torch.float16, 0), graphed._cache_token(cache), extra)


def test_a_new_cache_at_a_dropped_ones_address_is_another_cache():
    """Serving code builds a cache per generation run. CPython hands the next object of a size the block the last one of that size left, so
    after a plain ``del`` the new cache has the old one's id() — and, after its prefill, the same ``generation``. Keyed by id() + generation it
    would match the old cache's graph, whose launches write to the old (freed) pages."""
    seen_again = False
    for trial in range(40):
        a = new_cache(2, 64)
        id_a, gen_a, tok_a = id(a), a.generation, graphed._cache_token(a)
        ent = entry_for(a)
        assert ent.matches([a], ops.cache_epoch())
        del a
        b = new_cache(3, 256)
        tok_b = graphed._cache_token(b)
        assert tok_a != tok_b, "two cache objects share a signature token"
        assert not ent.matches([b], ops.cache_epoch()), "an entry captured over a dropped cache matches its successor"
        if id(b) == id_a:
            seen_again = True
            assert b.generation == gen_a          # what made the old staleness test blind
            break
    assert seen_again, "no id() came back in 40 trials: this test has not exercised the case it is for"


def test_cache_tokens_are_unique_among_live_and_dead_caches():
    toks = set()
    for _ in range(50):
        c = MultiLayerPagedKVCache4Bit(1, 16, 32, "cpu", 1, 2, 128)
        toks.add(graphed._cache_token(c))
    assert len(toks) == 50


def test_entry_goes_stale_when_the_epoch_or_the_storage_moves():
    a, b = new_cache(), new_cache()
    ent = entry_for(a)
    e = ops.cache_epoch()
    assert ent.matches([a], e)
    assert not ent.matches([a], e + 1)                                   # ops.invalidate_caches()
    assert not ent.matches([b], e) and not ent.matches([a, b], e) and not ent.matches([], e)
    # the pages re-allocated behind the cache's back (no generation bump): the baked address no longer holds
    a._pages = torch.empty_like(a._pages)
    assert not ent.matches([a], e)
    ent = entry_for(a)
    a._scales = torch.empty_like(a._scales)
    assert not ent.matches([a], e)
    ent = entry_for(a)
    a._st["last"] = torch.zeros_like(a._st["last"])                      # an index buffer replaced
    assert not ent.matches([a], e)
    ent = entry_for(a)
    g = a.generation
    a._ensure_page_cnt_per_batch(a.page_cnt_from_length(a.max_seq_len) + 1)   # page growth, as update() does it
    assert a.generation > g and not ent.matches([a], e)
    # two caches in one call: both must be the entry's, in order
    ent2 = entry_for(a, b)
    assert ent2.matches([a, b], e) and not ent2.matches([b, a], e)


def test_a_dead_cache_matches_nothing_and_leaves_no_record():
    gd = graphed.GraphedDecode(lambda *a: None)
    keep = new_cache()
    dead = new_cache()
    ent_dead = entry_for(dead)
    for c in (keep, dead):
        gd._watch([c])
        sig = sig_with(c)
        gd._keep_entry(sig, entry_for(c))
        gd._remember(sig, 2)
        gd._keep_logs(sig, [[(0, 1)]])
        gd._block(sig_with(c, extra=1))
    tok_dead, tok_keep = graphed._cache_token(dead), graphed._cache_token(keep)
    assert not isinstance(gd._entries[sig_with(dead)].refs[0], type(dead))       # a weak reference, not the object
    del dead, c
    gc.collect()
    assert ent_dead.refs[0]() is None
    assert not ent_dead.matches([keep], ops.cache_epoch())
    for table in (gd._entries, gd._seen, gd._logs, gd._blocked):
        assert not any(tok_dead in s for s in table), table
        assert sum(tok_keep in s for s in table) == 1                            # the live cache's records stay
    assert tok_dead not in gd._watched and tok_keep in gd._watched
    # the wrapper itself is not kept alive by the caches it has seen
    import weakref
    r = weakref.ref(gd)
    del gd
    gc.collect()
    assert r() is None


class Adapter:
    """what an integration may put around the cache: holds it as ``.inner`` and forwards ``update``"""

    def __init__(self, inner):
        self.inner = inner

    def update(self, *a, **k):
        return self.inner.update(*a, **k)


class Foreign:
    """some other cache-like object: the wrapper cannot run its host step outside a capture"""

    def __init__(self, hidden):
        self._hidden = hidden

    def update(self, *a, **k):
        return self._hidden.update(*a, **k)


def test_leaf_classification():
    c = new_cache()
    assert graphed._classify(c) == ("cache", c)
    kind, what = graphed._classify(Adapter(c))
    assert kind == "cache" and what is c                                 # one level of .inner / .cache is seen through

    class Holder:
        def __init__(self, cache):
            self.cache = cache
    kind, what = graphed._classify(Holder(c))
    assert kind == "cache" and what is c
    assert graphed._classify(Foreign(c)) == ("refuse", None)             # has update(), not recognised: the call is not captured
    assert graphed._classify(Adapter(Adapter(c))) == ("refuse", None)    # two levels: not seen through, and it has update()
    for v in (None, True, 3, 0.5, "x"):
        assert graphed._classify(v) == ("value", v)
    cfg = object()
    assert graphed._classify(cfg) == ("obj", cfg)
    m = torch.nn.Linear(2, 2)
    assert graphed._classify(m) == ("obj", m)


def test_tables_stay_bounded_under_a_thousand_signatures():
    gd = graphed.GraphedDecode(lambda *a: None)
    c = new_cache()
    for i in range(1000):
        sig = sig_with(c, extra=i)
        gd._remember(sig, 1)
        gd._keep_logs(sig, [[(0, 1)]])
        gd._block(sig)
        gd._keep_entry(sig, entry_for(c))
    n = gd.MAX_SIGNATURES
    assert len(gd._seen) <= n and len(gd._logs) <= n and len(gd._blocked) <= n and len(gd._entries) <= n
    assert sig_with(c, extra=999) in gd._blocked and sig_with(c, extra=0) not in gd._blocked     # the oldest go first
    assert len(gd._watched) == 0
    for _ in range(1000):                                                # a cache per generation run, each watched, each dropped
        k = new_cache()
        gd._watch([k])
        gd._remember(sig_with(k), 1)
        del k
    gc.collect()
    assert len(gd._watched) == 0 and len(gd._seen) <= n


def test_update_refuses_to_run_its_host_step_under_capture(monkeypatch):
    """A capture that reaches update() without the wrapper's ``_skip_host`` would bake the length and the index writes into the graph. (The
    stream's state is stubbed: the guard itself only ever asks a CUDA device.)"""
    c = new_cache()
    monkeypatch.setattr(kv_cache, "_capturing", lambda t: True)
    k = torch.zeros(2, 1, 4, 128, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="stream capture"):
        c.update(k, k, 0)
    with pytest.raises(RuntimeError, match="stream capture"):
        c._host_step(0, 1)
    with pytest.raises(RuntimeError, match="stream capture"):
        c.replay_host([(0, 1)])
    assert c.length == 22 and c._log is None                             # nothing happened
    with c.host_side_done():                                             # the wrapper's capture pass: the host side is left alone, no refusal
        c._refuse_capture()
    assert c._skip_host is False
    monkeypatch.undo()
    assert kv_cache._capturing(c._pages) is False                        # a CPU tensor: the device is never asked
    c._host_step(0, 1)
    assert c.length == 23


def test_linear4bit_image_keys_carry_the_cache_epoch():
    """An in-place reload of an inference tensor has no version counter to show (ops.ver is 0); the documented protocol is
    ops.invalidate_caches(), which moves the epoch — the module's own images must be keyed by it. (fp16 scales on the CPU; the operand
    images' keys are compared as the GPU test compares their results.)"""
    from flatquant_amd.deploy.nn import Linear4bit
    with torch.inference_mode():
        m = Linear4bit(128, 64, bias=True)
        m.weight_scales.fill_(0.5)
        s16, b16 = m._scales16()
        assert float(s16[0]) == 0.5
        m.weight_scales.fill_(0.25), m.bias.fill_(1.0)
        ops.invalidate_caches()
        s16, b16 = m._scales16()
    assert float(s16[0]) == 0.25 and float(b16[0]) == 1.0
