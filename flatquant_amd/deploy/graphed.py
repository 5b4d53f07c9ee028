"""Decode-sized calls served from captured HIP graphs — transparently.

The reference's decode table and layer benchmark are EAGER (README.md:300-310, benchmarks/layer_benchmark.py:131-143): a decoder layer's
one-token step is ~13 library launches of 3-30 us each, and from Python every launch costs 10-25 us of allocation, argument marshalling and
module plumbing — the step is host-bound (tools/bench_decode.py: 271 us eager against 73 us of kernels). The answer on this platform is a HIP
graph; this module supplies it WITHOUT caller-side graph code:

    deploy.fuse(model, capture=True)        # every decoder layer's forward is wrapped in a GraphedDecode

``GraphedDecode(fn)`` behaves like ``fn``. A call whose tensor arguments are decode-sized (<= ``max_rows`` rows) and which runs without
autograd is, per argument signature (shapes, dtypes, the other arguments by value or identity):
  1. run eagerly ``warmup`` times (default 2) — the library's caches (operand images, workspaces, launch plans) fill; the last of these runs
     on the wrapper's capture stream and RECORDS which host steps the paged KV caches among the arguments took (cache.update advances a length
     and rewrites its index tensors in place on the host: kv_cache.py ``_host_step``);
  2. captured: the tensor arguments are copied into static buffers, the caches' host steps are applied OUTSIDE the capture
     (``replay_host``), the callable runs once under ``torch.cuda.graph`` with the caches told to leave their host side alone;
  3. replayed from then on: copy the inputs in, apply the host steps, ``graph.replay()``, return the graph's output tensors.
Everything a step reads that changes between steps therefore sits in static device memory the replay sees: the inputs (copied), the cache's
pages (appended to in place by the captured launches through the index tensors), the index tensors (rewritten in place by the host step).
What makes an entry stale and sends the call back to the eager path for one call (then re-captured) — ``_Entry.matches``: the entry was
captured over ANOTHER cache object (caches are told apart by ``cache.serial``, a process-wide count, and by a weak reference the entry keeps —
never by ``id()``, which the next cache allocated after a ``del`` inherits); the cache's storage moved (page growth: ``cache.generation``, and
the addresses the graph holds as constants — pages, scales, index tensors — are compared as well: ``cache.graph_addresses()``); the library's
caches were invalidated (``ops.cache_epoch``). A prefill-sized or masked (ragged) call and a call under autograd are never captured.
A cache that dies takes its graphs with it: the wrapper holds no strong reference to a cache (an output that IS the cache is replaced by the
live argument on return), and a finalizer drops the entries, warm-up counts, recorded host steps and blocked signatures that name it.
A cache wrapped ONE level deep — an adapter with the cache as ``.inner`` or ``.cache`` that forwards ``update`` — is recognised and captured
like a bare one. A call with any other object that has an ``update`` method among its arguments is NOT captured (it may be a cache the wrapper
cannot drive from outside the capture); and a cache reached some other way refuses to run its host step under capture (RuntimeError in
``update``), so that capture fails, the signature is blocked and the call stays eager — correct, never a graph with a frozen length.

The returned tensors are the graph's OUTPUT BUFFERS: valid until the next call of the same wrapper with the same signature — a decoder
layer's output is consumed by the next layer within the step, which is the reference's usage; ``clone_outputs=True`` copies them out."""
import collections
import weakref

import torch
from torch.utils import _pytree

from .. import ops

DECODE_ROWS = 128


def _is_cache(a) -> bool:
    return hasattr(a, "replay_host") and hasattr(a, "generation") and hasattr(a, "_needs_init") and hasattr(a, "serial")


def _cache_token(cache):
    """A cache's place in a signature: its process-unique serial. (``id()`` comes back as soon as the object is dropped.)"""
    return ("cache", cache.serial)


def _classify(v):
    """What one non-tensor pytree leaf is to the wrapper -> (kind, payload):
    ("cache", the cache) — a paged KV cache, bare or ONE level inside an adapter (``.inner`` / ``.cache``);
    ("value", v) — None / bool / int / float / str, part of the signature by value;
    ("refuse", None) — an unrecognised object with an ``update`` attribute: possibly a cache behind a wrapper this module cannot see
    through, whose host step would be frozen into the graph — the call is not captured;
    ("obj", v) — anything else (a module, a config object): by identity, its CONTENT must not change between steps."""
    if _is_cache(v):
        return "cache", v
    if v is None or isinstance(v, (bool, int, float, str)):
        return "value", v
    for name in ("inner", "cache"):
        inner = getattr(v, name, None)
        if inner is not None and _is_cache(inner):
            return "cache", inner
    if hasattr(v, "update"):
        return "refuse", None
    return "obj", v


def _walk_out(o, fn):
    if isinstance(o, torch.Tensor):
        return fn(o)
    if isinstance(o, (list, tuple)):
        return type(o)(_walk_out(v, fn) for v in o)
    if isinstance(o, dict):
        return {k: _walk_out(v, fn) for k, v in o.items()}
    return o


class _ArgSlot:
    """Stands in a captured entry's output for an argument that came back as (part of) the result — the cache, or the adapter around it, as
    HF layers return ``past_key_value``: the entry must not keep that object alive; the LIVE argument is returned in its place.
    ``leaf`` >= 0: that leaf of the call's arguments; < 0: cache number ``-1 - leaf`` of the call (the cache inside an adapter)."""
    __slots__ = ("leaf",)

    def __init__(self, leaf):
        self.leaf = leaf


def _map_objects(o, fn):
    """``o`` with ``fn`` applied to every non-tensor, non-container leaf"""
    if isinstance(o, torch.Tensor):
        return o
    if isinstance(o, (list, tuple)):
        return type(o)(_map_objects(v, fn) for v in o)
    if isinstance(o, dict):
        return {k: _map_objects(v, fn) for k, v in o.items()}
    return fn(o)


class _Entry:
    __slots__ = ("graph", "static_in", "out", "slots", "logs", "gens", "epoch", "refs", "addrs")

    def bind(self, caches, epoch):
        """Record WHICH caches (weakly), in what state, the graph was captured over."""
        self.refs = [weakref.ref(c) for c in caches]
        self.gens = [c.generation for c in caches]
        self.addrs = [c.graph_addresses() for c in caches]
        self.epoch = epoch

    def matches(self, caches, epoch) -> bool:
        """May the graph be replayed for a call with these caches? Same library epoch, the very same cache objects (alive), whose storage has
        not moved since: the generation counts and every address the graph holds as a constant."""
        if self.epoch != epoch or len(caches) != len(self.refs):
            return False
        for c, r, g, a in zip(caches, self.refs, self.gens, self.addrs):
            if r() is not c or c.generation != g or c.graph_addresses() != a:
                return False
        return True


def _forget_cache(wrapper_ref, token):
    gd = wrapper_ref()
    if gd is not None:
        gd._forget(token)


class GraphedDecode:
    MAX_SIGNATURES = 64     # captured graphs, signatures still in warm-up and blocked signatures kept per wrapper (least recently created first out)

    def __init__(self, fn, max_rows: int = DECODE_ROWS, warmup: int = 2, clone_outputs: bool = False):
        self.fn, self.max_rows, self.warmup, self.clone_outputs = fn, max_rows, max(1, warmup), clone_outputs
        self._entries, self._seen, self._logs, self._blocked = {}, {}, {}, collections.OrderedDict()
        self._watched = {}      # cache token -> the finalizer that sweeps this wrapper's tables when that cache dies
        self._stream = None
        self.replays = self.captures = self.eager_calls = 0     # (counters: tests, tools/bench_decode.py)

    # -- argument handling ------------------------------------------------------------------------------------------------
    def _split(self, args, kwargs):
        """-> (leaves, spec, tensor positions, tensors, caches, signature, cache leaf positions) or None when the call is not one to capture.
        The arguments are flattened as a pytree, so tensors inside tuples / lists / dicts (HF's ``position_embeddings=(cos, sin)``) are graph
        inputs too. Every other leaf: ``_classify``."""
        leaves, spec = _pytree.tree_flatten((args, kwargs))
        pos, tensors, caches, cpos, sig = [], [], [], [], [spec]
        for i, v in enumerate(leaves):
            if isinstance(v, torch.Tensor):
                if not v.is_cuda or v.requires_grad:
                    return None
                pos.append(i), tensors.append(v)
                sig.append((tuple(v.shape), v.dtype, v.device.index))
                continue
            kind, what = _classify(v)
            if kind == "cache":
                caches.append(what), cpos.append(i)
                sig.append(_cache_token(what))
            elif kind == "value":
                sig.append(what)
            elif kind == "refuse":
                return None
            else:
                sig.append(("obj", id(v)))
        if not tensors:
            return None
        rows = 1
        for d in tensors[0].shape[:-1]:
            rows *= d
        if rows > self.max_rows or rows == 0:
            return None
        return leaves, spec, pos, tensors, caches, tuple(sig), cpos

    @staticmethod
    def _subst(leaves, spec, pos, tensors):
        leaves = list(leaves)
        for i, t in zip(pos, tensors):
            leaves[i] = t
        return _pytree.tree_unflatten(leaves, spec)

    # -- the tables: every one bounded by MAX_SIGNATURES, none holds a cache ------------------------------------------------------
    def _bounded_set(self, table, sig, value):
        if sig not in table and len(table) >= self.MAX_SIGNATURES:
            table.pop(next(iter(table)))
        table[sig] = value

    def _remember(self, sig, n):
        """warm-up counts per signature, bounded: a caller whose signature changes on every call (a growing attention mask, a fresh
        object per step) must not grow this table without limit — it simply stays eager."""
        self._bounded_set(self._seen, sig, n)

    def _keep_logs(self, sig, logs):
        self._bounded_set(self._logs, sig, logs)

    def _block(self, sig):
        """a signature whose capture failed: eager from now on. Bounded like the others — a forgotten one is simply tried (and blocked) again."""
        self._bounded_set(self._blocked, sig, True)

    def _keep_entry(self, sig, ent):
        self._bounded_set(self._entries, sig, ent)

    def _watch(self, caches):
        """When one of ``caches`` dies, every record of this wrapper that names it goes (``_forget``): its graphs (and their memory pools), its
        warm-up counts, its recorded host steps, its blocked signatures. The finalizer holds the wrapper weakly."""
        for c in caches:
            tok = _cache_token(c)
            if tok not in self._watched:
                fin = self._watched[tok] = weakref.finalize(c, _forget_cache, weakref.ref(self), tok)
                fin.atexit = False

    def _forget(self, token):
        self._watched.pop(token, None)
        for table in (self._entries, self._seen, self._logs, self._blocked):
            for sig in [s for s in table if token in s[1:]]:        # (s[0] is the pytree spec)
                del table[sig]

    # -- the call -----------------------------------------------------------------------------------------------------------
    def __call__(self, *args, **kwargs):
        if torch.is_grad_enabled() or torch.cuda.is_current_stream_capturing():
            return self.fn(*args, **kwargs)
        sp = self._split(args, kwargs)
        if sp is None:
            return self.fn(*args, **kwargs)
        leaves, spec, pos, tensors, caches, sig, cpos = sp
        if sig in self._blocked or any(any(c._needs_init) for c in caches):   # (capture failed once | a prompt has not been through this cache
            return self.fn(*args, **kwargs)                                    #  yet: the prefill branch of update())
        ent = self._entries.get(sig)
        if ent is not None:
            stale = not ent.matches(caches, ops.cache_epoch()) \
                or any(c.would_grow(sum(a for _, a in log)) for c, log in zip(caches, ent.logs))
            if stale:
                del self._entries[sig]
                self._remember(sig, self.warmup - 1)         # one eager call (it re-allocates / re-warms), then a new capture
                ent = None
        if ent is None:
            self._watch(caches)
            n = self._seen.get(sig, 0)
            if n + 1 < self.warmup:
                self._remember(sig, n + 1)
                self.eager_calls += 1
                return self.fn(*args, **kwargs)
            if n + 1 == self.warmup:                          # the last warm-up: on the capture stream, recording the caches' host steps
                self._remember(sig, n + 1)
                self.eager_calls += 1
                return self._recorded_eager(args, kwargs, caches, sig)
            ent = self._capture(leaves, spec, pos, tensors, caches, sig, cpos)
            if isinstance(ent, tuple):                        # (the capture failed; the step ran eagerly inside _capture)
                self.eager_calls += 1
                return ent[1]
            if ent is None:
                self.eager_calls += 1
                return self.fn(*args, **kwargs)
            self._keep_entry(sig, ent)
        else:
            for s, t in zip(ent.static_in, tensors):
                s.copy_(t)
            for c, log in zip(caches, ent.logs):
                c.replay_host(log, False)                     # (the stream is not capturing: looked at above)
        ent.graph.replay()
        self.replays += 1
        out = ent.out
        if ent.slots:                                         # (an argument came back in the result: the live one, not a kept one)
            out = _map_objects(out, lambda o: o if type(o) is not _ArgSlot else leaves[o.leaf] if o.leaf >= 0 else caches[-1 - o.leaf])
        return _walk_out(out, lambda t: t.clone()) if self.clone_outputs else out

    def _recorded_eager(self, args, kwargs, caches, sig):
        if self._stream is None:
            self._stream = torch.cuda.Stream()
        cur = torch.cuda.current_stream()
        self._stream.wait_stream(cur)
        for c in caches:
            c._log = []
        try:
            with torch.cuda.stream(self._stream):
                out = self.fn(*args, **kwargs)
        finally:
            logs = [c._log for c in caches]
            for c in caches:
                c._log = None
        cur.wait_stream(self._stream)
        self._keep_logs(sig, logs)
        return out

    def _capture(self, leaves, spec, pos, tensors, caches, sig, cpos=()):
        logs = self._logs.pop(sig, None)
        if logs is None or any(step is None for log in logs for step in log):
            return None                                       # (a masked / prefill update: not a replayable step)
        if any(c.would_grow(sum(a for _, a in log)) for c, log in zip(caches, logs)):
            return None
        ent = _Entry()
        cur = torch.cuda.current_stream()
        self._stream.wait_stream(cur)
        with torch.cuda.stream(self._stream):
            ent.static_in = [t.clone() for t in tensors]
        sargs, skwargs = self._subst(leaves, spec, pos, ent.static_in)
        for c, log in zip(caches, logs):
            c.replay_host(log)                                # the host side of THIS step, outside the capture (stream-ordered in front of it)
        self._stream.wait_stream(cur)
        ops.images_ready()                                    # fragment images prepared by the warm-up are complete: shared, not re-prepared in the graph
        ent.graph = torch.cuda.CUDAGraph()
        for c in caches:
            c._skip_host = True
        try:
            with torch.cuda.graph(ent.graph, stream=self._stream):
                out = self.fn(*sargs, **skwargs)
        except Exception:
            # The callable cannot be captured (an op that synchronises, allocates on the host, a cache this wrapper did not recognise refusing
            # its host step under capture, ...). The recognised caches' host steps of THIS call have been applied: run the step eagerly with
            # those caches still told to leave their host side alone, never try this signature again.
            self._block(sig)
            torch.cuda.synchronize()
            return ("eager", self.fn(*sargs, **skwargs))
        finally:
            for c in caches:
                c._skip_host = False
        cur.wait_stream(self._stream)
        # an argument that came back in the result (the cache itself, or the adapter around it) is not kept: its leaf position is
        # (>= 0), or for the cache inside an adapter its place among the caches (< 0)
        held = {id(leaves[i]): i for i in cpos}
        held.update((id(c), -1 - j) for j, c in enumerate(caches) if id(c) not in held)
        ent.slots = False

        def slot(o):
            i = held.get(id(o))
            if i is None:
                return o
            ent.slots = True
            return _ArgSlot(i)
        ent.out = _map_objects(out, slot)
        del out, sargs, skwargs
        ent.logs = logs
        ent.bind(caches, ops.cache_epoch())
        self.captures += 1
        return ent

    def release(self):
        """Drop every captured graph (and its private memory pool)."""
        self._entries.clear(), self._seen.clear(), self._logs.clear(), self._blocked.clear()
        for fin in self._watched.values():
            fin.detach()
        self._watched.clear()
