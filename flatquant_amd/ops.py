"""Tensor-level entry points: torch device memory + streams in, libfqhip C-ABI calls out.

PyTorch is plumbing here (allocation, current stream, device guard); all arithmetic happens in the HIP
kernels.  Inputs must be CUDA (ROCm) fp16 contiguous tensors — violations raise, as the reference's
``torch::check*`` / ``assert`` do (deploy/kernels/bindings.cpp:11-16,29-34; kron_matmul.py:195-199).
"""
from __future__ import annotations

import collections
import ctypes
import functools
import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (FQ_EUNSUPPORTED, FQ_GROUP128, FQ_MAX_CLIPS, FQ_NO_CLAMP0, FQ_OUT_FAKEQUANT, FQ_OUT_PACKED,
                   FQ_OUT_TRANSFORM, FQ_QUANT_F16, FQ_RATIO_POST, FQ_ROUND_Y_F16, FQ_SIG_F16, FQ_WS_PREPARED, check, lib)

Sig = Tuple[float, float]  # (sigmoid(clip_factor_a_max), sigmoid(clip_factor_a_min)); (1.0, 1.0) = no clip


@functools.lru_cache(maxsize=4096)
def _sigmoid_pair_cached(clip_max: float, clip_min: float) -> Sig:
    t = torch.sigmoid(torch.tensor([clip_max, clip_min], dtype=torch.float32))
    return float(t[0]), float(t[1])


def sigmoid_pair(clip_max, clip_min) -> Sig:
    """fp32 sigmoid of the raw (pre-sigmoid) learnable clipping factors, evaluated by torch on the host —
    the value the reference multiplies the row extrema with (quant_utils.py:96-97, kron_matmul.py:93-94)."""
    return _sigmoid_pair_cached(host_scalar(clip_max), host_scalar(clip_min))


def sigmoid_pair_f16(clip_max, clip_min) -> Sig:
    """sigmoid_pair rounded to fp16: what a DEVICE multiplies an fp16 tensor with when the other operand is a 0-dim fp32
    tensor (deploy/nn/quantization.py:21-22, deploy/functional/online_trans.py:97-98 move the 0-dim sigmoid to x's device;
    torch's device kernels cast a 0-dim operand to the result dtype on load — measured on MI355X,
    tools/microbench/sig_f16_probe.py: every finite fp16 extremum agrees with fp16(x * fp16(sigmoid)); the CPU keeps the fp32
    value). The product of two fp16 values is exact in fp32, so FQ_SIG_F16 then rounds once."""
    return _sig_f16_cached(*sigmoid_pair(clip_max, clip_min))


@functools.lru_cache(maxsize=4096)
def _sig_f16_cached(a: float, b: float) -> Sig:
    t = torch.tensor([a, b], dtype=torch.float32).to(torch.float16)   # (three tensor ops: ~6 us a call before the cache, round 4)
    return float(t[0]), float(t[1])


_SCALARS: "collections.OrderedDict" = collections.OrderedDict()


_CACHE_EPOCH = [0]


def ver(t: torch.Tensor) -> int:
    """``t._version`` for the cache keys of this package — 0 for an INFERENCE tensor, which has no version counter (reading it raises
    "Inference tensors do not track version counter"): the reference decorates its generation and benchmark entry points with
    ``@torch.inference_mode()`` (benchmarks/qlinear_benchmark.py builds its modules inside one), so buffers created and activations
    produced there are inference tensors. They cannot be written in place outside inference mode at all; a caller that rewrites one in
    place INSIDE inference mode (no counter to see it by) calls invalidate_caches(), as after a write through ``.data``."""
    return 0 if t.is_inference() else t._version


def cache_epoch() -> int:
    """Incremented by invalidate_caches(): part of the key of every cache a MODULE holds for itself."""
    return _CACHE_EPOCH[0]


class _CacheRegistry:
    """ONE object over every cache this module keeps (VERDICT r05 hygiene: seven caches keyed on data_ptr / version, each with its own
    rules). The protocol, for all of them:
      * KEY: (data_ptr, ver(tensor)) of the tensors a value was derived from (+ device / stream where the value is a device buffer) — an
        in-place write through the tensor bumps the version and misses; a write through ``.data`` does not: invalidate().
      * INVALIDATION: ``invalidate()`` (= ops.invalidate_caches()) clears every DERIVED cache and bumps the epoch the modules' own launch
        plans carry in their keys; load_state_dict of any mirror module calls it (invalidate_on_load).
      * PINNING: a value handed to a launch issued UNDER STREAM CAPTURE moves to its cache's pinned side and is never freed or cleared —
        the captured graph replays the raw pointer (fragment images: _WS_PINNED; split-decode workspaces: _KV_SPLIT_WS_PINNED).
      * BOUNDS: every unpinned cache is bounded by entries and, where entries are device buffers, by bytes (least recently used first).
    ``stats()`` reports entries and device bytes per cache (tests, tools/host_overhead.py)."""

    def __init__(self):
        self._derived, self._pinned, self._hooks = {}, {}, []

    def register(self, name, mapping, pinned=False):
        (self._pinned if pinned else self._derived)[name] = mapping
        return mapping

    def on_invalidate(self, fn):
        self._hooks.append(fn)
        return fn

    def invalidate(self):
        _CACHE_EPOCH[0] += 1    # (module-held launch plans carry the epoch in their key: deploy.nn.OnlineTrans / Quantizer / Linear4bit)
        for m in self._derived.values():
            m.clear()           # (the pinned sides stay: a captured graph replays the pointers it was given)
        for fn in self._hooks:
            fn()

    @staticmethod
    def _bytes(v):
        if isinstance(v, torch.Tensor):
            return v.numel() * v.element_size() if v.is_cuda else 0
        if isinstance(v, (tuple, list)):
            return _CacheRegistry._bytes(v[0]) if v else 0      # (entries are (buffer, the tensors it was derived from, ...): count the buffer)
        return 0

    def stats(self) -> dict:
        out = {}
        for side, maps in (("derived", self._derived), ("pinned", self._pinned)):
            for name, m in maps.items():
                out[name] = {"side": side, "entries": len(m), "device_bytes": sum(self._bytes(v) for v in m.values())}
        out["epoch"] = _CACHE_EPOCH[0]
        return out


CACHES = _CacheRegistry()
CACHES.register("host_scalars", _SCALARS)


def cache_stats() -> dict:
    """Entries and device bytes of every cache of this module, derived and pinned (see _CacheRegistry)."""
    return CACHES.stats()


def invalidate_caches() -> None:
    """Forget every value this module derived from tensors it does not own: host copies of clip scalars (host_scalar),
    fragment workspaces of factor matrices, Hadamard factor pairs, unpinned split-decode workspaces. The caches are keyed by
    (data_ptr, ver(tensor)): an in-place write through the tensor itself (``t.fill_()``, ``t.copy_()``) bumps the version and is seen, a write
    through ``t.data`` (``mod.clip_factor_a_max.data.fill_(..)``, ``weight.data.copy_(..)``) does NOT — call this after
    such an update (checkpoint loaders that assign ``.data`` should), or update in place on the tensor. One protocol for all of them:
    _CacheRegistry."""
    CACHES.invalidate()


@CACHES.on_invalidate
def _clear_function_caches():
    _sigmoid_pair_cached.cache_clear()
    _sig_f16_cached.cache_clear()
    from .flatquant.trans_utils import _Fp16Cache   # the modules' fp16 / bf16 copies of their (fp32) matrices
    _Fp16Cache.clear_all()


def invalidate_on_load(module: torch.nn.Module) -> None:
    """Mirror modules call this in their constructor: after ``load_state_dict`` (whose ``copy_`` goes through ``param.data``
    semantics for assign=True / ``.data`` loaders and may recycle addresses) every derived cache is dropped, so a module never
    runs on fragments or scalars of the matrices it held before the load."""
    module.register_load_state_dict_post_hook(lambda mod, incompatible: invalidate_caches())


def host_scalar(v) -> float:
    """float(v) for a Python number or a one-element tensor, WITHOUT a device synchronisation per call: a CUDA
    scalar (the deploy modules keep clip_factor_a_max/min as buffers; the reference's loader turns them into Python
    floats, modeling_llama.py:532-538) is read back once per (storage, version) and remembered. The entry holds the
    tensor, so its address cannot be recycled under it. Writes through ``.data`` do not bump the version: see
    invalidate_caches()."""
    if not isinstance(v, torch.Tensor):
        return float(v)
    if not v.is_cuda:
        return float(v)
    key = (v.data_ptr(), ver(v))
    hit = _SCALARS.get(key)
    if hit is not None:
        return hit[0]
    val = float(v.item())
    _SCALARS[key] = (val, v)
    if len(_SCALARS) > 4096:
        _SCALARS.popitem(last=False)
    return val


def _chk(t: torch.Tensor, name: str, dtype=torch.float16) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA/ROCm tensor (flatquant_amd has no CPU path); got {t.device}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


ACT_DTYPES = (torch.float16, torch.bfloat16)


def _chk_act(x: torch.Tensor, name: str = "x"):
    """The activation of a path-A entry point: fp16 or bf16 (the reference's eval pipeline feeds whatever the checkpoint
    declares, flatquant/model_utils.py:20 torch_dtype='auto'; main_dpskv3.py:395). Returns its dtype: every other fp tensor
    of the call must have it too, and the library's *_f16 / *_bf16 entry point is picked by it (_fn)."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if x.dtype not in ACT_DTYPES:
        raise TypeError(f"{name} must be torch.float16 or torch.bfloat16, got {x.dtype}")
    _chk(x, name, x.dtype)
    return x.dtype


def _fn(stem: str, dtype):
    """libfqhip entry point of a dtype: fq_<stem>_f16 / fq_<stem>_bf16."""
    return getattr(lib, f"fq_{stem}_bf16" if dtype == torch.bfloat16 else f"fq_{stem}_f16")


def _ptr(t: Optional[torch.Tensor]):
    """a tensor's address as ctypes takes it for a c_void_p argument: a plain int (None = NULL) — no c_void_p object per argument"""
    return None if t is None else t.data_ptr()


_NULL4 = (ctypes.c_void_p * FQ_MAX_CLIPS)()   # the output sets a launch does not write (read-only on the C side)


def _ptr_array(ts: Sequence[Optional[torch.Tensor]]):
    if not ts:
        return _NULL4
    arr = (ctypes.c_void_p * FQ_MAX_CLIPS)()
    for i, t in enumerate(ts):
        arr[i] = 0 if t is None else t.data_ptr()
    return arr


@functools.lru_cache(maxsize=1024)
def _sig_arrays_cached(key):
    smax = (ctypes.c_float * FQ_MAX_CLIPS)(*[s[0] for s in key])
    smin = (ctypes.c_float * FQ_MAX_CLIPS)(*[s[1] for s in key])
    return smax, smin, len(key)


def _sig_arrays(sigs: Sequence[Sig]):
    """-> (float[4] sig_max, float[4] sig_min, n): read-only on the C side, so the arrays of a clip-set tuple are built once"""
    n = len(sigs)
    if not 1 <= n <= FQ_MAX_CLIPS:
        raise ValueError(f"between 1 and {FQ_MAX_CLIPS} clip sets are supported, got {n}")
    return _sig_arrays_cached(tuple((float(s[0]), float(s[1])) for s in sigs))


class _on:
    """``with _on(t.device):`` — the launch's device made current for the library call (kernels go to the CURRENT device's stream
    handle; a multi-GPU process may hold tensors of several). ``torch.cuda.device`` does the same but exchanges the device on
    entry and exit unconditionally (~6 us of the ~30 us a module call spends on the host); the tensor's device almost always IS the
    current one, and then this is one cached look-up."""
    __slots__ = ("idx", "prev")

    def __init__(self, device: torch.device):
        self.idx = device.index
        self.prev = -1

    def __enter__(self):
        if self.idx is not None:
            cur = torch.cuda.current_device()
            if cur != self.idx:
                torch.cuda.set_device(self.idx)
                self.prev = cur
        return self

    def __exit__(self, *exc):
        if self.prev >= 0:
            torch.cuda.set_device(self.prev)
        return False


# The current stream's raw handle. torch.cuda.current_stream() builds a Stream object through two device-index helpers: ~4 us a call,
# twice per launch (the workspace key and the launch argument) — 8 of the ~19 us a library call spent on the host (round 4,
# tools/host_overhead.py). torch._C._cuda_getCurrentRawStream is the same look-up without the object.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_handle(device: torch.device) -> int:
    if _raw_stream is not None:
        return _raw_stream(device.index if device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(device).cuda_stream


def _stream(t: torch.Tensor):
    return ctypes.c_void_p(_stream_handle(t.device))


class FusedOutputs:
    """Outputs of one fused transform+quant launch (lists are indexed by clip set)."""

    def __init__(self):
        self.q: List[torch.Tensor] = []       # uint8 [..., d/2]
        self.scale: List[torch.Tensor] = []   # fp16 [rows]
        self.fq: List[torch.Tensor] = []      # fp16 [..., d]
        self.y: Optional[torch.Tensor] = None  # fp16 [..., d]


def _alloc_outputs(x: torch.Tensor, rows: int, d: int, n_clips: int, flags: int, q_shape, y_shape):
    o = FusedOutputs()
    for _ in range(n_clips if flags & (FQ_OUT_PACKED | FQ_OUT_FAKEQUANT) else 0):
        if flags & FQ_OUT_PACKED:
            o.q.append(torch.empty(q_shape, dtype=torch.uint8, device=x.device))
            o.scale.append(torch.empty((rows,), dtype=x.dtype, device=x.device))
        if flags & FQ_OUT_FAKEQUANT:
            o.fq.append(torch.empty(y_shape, dtype=x.dtype, device=x.device))
    if flags & FQ_OUT_TRANSFORM:
        o.y = torch.empty(y_shape, dtype=x.dtype, device=x.device)
    return o


# Fragment workspaces of the non-64x64 Kronecker kernels, one per (device, stream, left, right): the launch re-packs
# left/right into MFMA fragment order there (~5 us); a deployed layer passes the same two buffers every call, so the
# second call onwards skips the re-pack (FQ_WS_PREPARED). An entry keeps its tensors alive (their addresses cannot be
# recycled under it) and is keyed by torch's version counters (in-place updates miss). LRU-bounded.
_WS_LRU: "collections.OrderedDict" = CACHES.register("kron_images_by_stream", collections.OrderedDict())
_WS_LRU_MAX = 512
_WS_LRU_MAX_BYTES = 256 << 20   # and by bytes: a caller that re-stacks per-expert matrices on every call (keys never repeat) would
                                # otherwise pin hundreds of multi-megabyte images before the count bound evicts one


_WS_BYTES: dict = {}   # fq_kron_workspace_bytes(M, N): a pure function of the pair
_WS_ANY: dict = CACHES.register("kron_images_any_stream", {})     # the same images by (device, M, N, left, right) WITHOUT the stream: (ws, left, right, [complete], event of the preparing launch)
_WS_ANY_MAX_BYTES = _WS_LRU_MAX_BYTES
# Images handed to a launch issued UNDER STREAM CAPTURE: the graph holds the raw pointer (FQ_WS_PREPARED, no prepare kernel of its own)
# for as long as it is replayed, so the cache may never free them — not on an LRU / byte-bound eviction, not on invalidate_caches()
# (a load_state_dict hook of ANY module calls that). id(workspace) -> (workspace, left, right). Bounded by what graphs were captured.
_WS_PINNED: dict = CACHES.register("kron_images_pinned", {}, pinned=True)


def _pin_for_capture(ent) -> None:
    if torch.cuda.is_current_stream_capturing():
        _WS_PINNED.setdefault(id(ent[0]), (ent[0], ent[1], ent[2]))


def images_ready() -> int:
    """Ask the preparing launch of every cached fragment image whether it has completed (an event query each; no wait) -> how many are
    still pending. Call it after a device / stream synchronisation and BEFORE capturing a graph on another stream: inside a capture no
    event may be queried, so a captured launch only shares an image already known complete — otherwise it prepares its own image inside
    the graph (correct, and replayed with every step: the 240 prepare launches of round 4's C4 graph)."""
    pending = 0
    for ent in _WS_ANY.values():
        if not ent[3][0]:
            if ent[4].query():
                ent[3][0] = True
            else:
                pending += 1
    for ent in _KV_TIMG.values():          # (the K-transform images of kv_decode_append: same rule)
        if not ent[3]["done"]:
            if ent[2].query():
                ent[3]["done"] = True
            else:
                pending += 1
    return pending


def _kron_workspace(device: torch.device, M: int, N: int, left: torch.Tensor, right: torch.Tensor):
    """-> (workspace | None, bytes, prepared, key). Keyed by stream too: two streams must not share a buffer. The
    caller registers a fresh workspace (_kron_workspace_commit) once the launch that fills it has been accepted."""
    nbytes = _WS_BYTES.get((M, N))
    if nbytes is None:
        nbytes = _WS_BYTES[(M, N)] = int(lib.fq_kron_workspace_bytes(M, N))
    if nbytes < 0:
        raise _lib.FqError(nbytes, f"no kernel for Kronecker factors ({M}, {N}): need M, N <= 256 and M * N <= 32768")
    if nbytes == 0:   # (no pair has a zero-size workspace since round 3: 64 x 64 takes its optional 32 KB image)
        return None, 0, False, None
    key = (device.index, _stream_handle(device), M, N,
           left.data_ptr(), ver(left), right.data_ptr(), ver(right))
    ent = _WS_LRU.get(key)
    if ent is not None:
        _WS_LRU.move_to_end(key)
        _pin_for_capture(ent)
        return ent[0], nbytes, True, key
    # Another stream: an image of the same pair prepared on a DIFFERENT stream is read-only once its preparing launch has completed, and
    # may then be shared — otherwise every captured launch carried its own fq_kron_prepare_kernel into the graph and replayed it every
    # step (round 4: 240 of them in bench.py's C4 graph, 4 % of C5's step). Outside capture the preparing launch's event is asked; under
    # capture (no event may be queried there, and a raw CUDAGraph.capture_begin() does not synchronise the device as torch.cuda.graph
    # does) only an image ALREADY known complete is shared: ops.images_ready() after the warm-up's synchronise establishes that.
    other = _ws_shared(key)
    if other is not None:
        return other[0], nbytes, True, key
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes, False, key


def _ws_shared(key):
    """The image of this key's pair prepared on ANOTHER stream, if its preparing launch has completed (it is then registered under
    this stream as well); None otherwise."""
    other = _WS_ANY.get(key[:1] + key[2:])
    if other is None:
        return None
    done = other[3]
    if not done[0]:
        if torch.cuda.is_current_stream_capturing():
            return None          # (cannot ask inside a capture; the launch prepares its own image in the capture's pool)
        if other[4].query():
            done[0] = True
    if not done[0]:
        return None
    _WS_LRU[key] = other[:3]
    _pin_for_capture(other)
    return other[:3]


def _kron_workspace_commit(key, ws: torch.Tensor, left: torch.Tensor, right: torch.Tensor) -> None:
    _WS_LRU[key] = (ws, left, right)
    _pin_for_capture((ws, left, right))     # (prepared INSIDE a capture: the graph's later launches and its replays read it)
    if not torch.cuda.is_current_stream_capturing():      # (an event recorded inside a capture belongs to the graph)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(ws.device))
        _WS_ANY[key[:1] + key[2:]] = (ws, left, right, [False], ev)
        # the stream-less index keeps its tensors alive too: bounded by count AND by bytes like the LRU (an entry the LRU drops leaves
        # with it, below), so that re-stacked per-expert matrices — multi-megabyte images whose keys never repeat — cannot pin gigabytes
        any_total = sum(e[0].numel() for e in _WS_ANY.values()) if ws.numel() > (1 << 20) else 0
        while len(_WS_ANY) > 2 * _WS_LRU_MAX or (any_total > _WS_ANY_MAX_BYTES and len(_WS_ANY) > 1):
            any_total -= _WS_ANY.pop(next(iter(_WS_ANY)))[0].numel()
    total = sum(e[0].numel() for e in _WS_LRU.values()) if ws.numel() > (1 << 20) else 0   # (only big images can hit the byte bound)
    while len(_WS_LRU) > _WS_LRU_MAX or (total > _WS_LRU_MAX_BYTES and len(_WS_LRU) > 1):
        k_old, ent = _WS_LRU.popitem(last=False)
        total -= ent[0].numel()
        other = _WS_ANY.get(k_old[:1] + k_old[2:])
        if other is not None and other[0] is ent[0]:
            del _WS_ANY[k_old[:1] + k_old[2:]]


def _group_scales_shape(o: FusedOutputs, lead, groups_per_row: int) -> None:
    o.scale = [sc.reshape(lead + (groups_per_row,)) for sc in o.scale]


def _quant_groups_of(y: torch.Tensor, sigs: Sequence[Sig], flags: int, groupsize: int, o: FusedOutputs) -> FusedOutputs:
    """groupsize-element groups of an already transformed fp16 activation: the reference's own formulation,
    ``x.reshape(-1, groupsize)`` then the per-row quantiser (vllm_custom/.../fake_quant_utils.py:72-78)."""
    d = y.shape[-1]
    r = rowquant(y.reshape(-1, groupsize), sigs, flags & ~FQ_OUT_TRANSFORM)
    o.q = [q.reshape(y.shape[:-1] + (d // 2,)) for q in r.q]
    o.scale = [sc.reshape(y.shape[:-1] + (d // groupsize,)) for sc in r.scale]
    o.fq = [f.reshape(y.shape) for f in r.fq]
    return o


def kron_quant(x: torch.Tensor, left: torch.Tensor, right: torch.Tensor, sigs: Sequence[Sig] = ((1.0, 1.0),),
               flags: int = FQ_OUT_PACKED, diag: Optional[torch.Tensor] = None, groupsize: int = -1) -> FusedOutputs:
    """y = x @ kron(left, right) fused with per-token INT4 quantisation (fq_kron_quant_f16).

    groupsize = 128: one scale per 128 consecutive elements of the transformed token instead of one per token
    (ActivationQuantizer(groupsize=128)); scales come back as [..., d/128]. One launch (FQ_GROUP128) where the library
    fuses it — packed output at N = 64, and with FQ_ROUND_Y_F16 every output set of the listed pairs (64x112 = 7168,
    32x64 = 2048, 64x128, 112x128, ...), fp16 and bf16 — otherwise the transform launch followed by the row quantiser over
    the (-1, 128) view of its result: the reference's own order of operations.

    x fp16 or bf16 (left / right / diag of the same dtype): fq_kron_quant_f16 / fq_kron_quant_bf16; outputs in x's dtype."""
    dt = _chk_act(x)
    _chk(left, "left", dt), _chk(right, "right", dt)
    M, N = left.shape[0], right.shape[0]
    if left.shape != (M, M) or right.shape != (N, N):
        raise ValueError("left/right must be square")
    d = M * N
    if x.shape[-1] != d:
        raise ValueError(f"x.shape[-1]={x.shape[-1]} != {M}*{N}")
    if diag is not None:
        _chk(diag, "diag", dt)
        if diag.numel() != d:
            raise ValueError("diag must have M*N elements")
    if groupsize not in (-1, 128) or (groupsize == 128 and d % 128):
        raise ValueError("groupsize must be -1 (per token) or 128 with M*N % 128 == 0")
    rows = x.numel() // d
    smax, smin, n = _sig_arrays(sigs)
    # one launch (FQ_GROUP128): the packed fp32-arithmetic launch at N = 64 (wave-per-token kernels), or — with
    # FQ_ROUND_Y_F16, the transformed activation rounded to x's dtype as ActivationQuantizer(groupsize=128) sees it — any
    # output set of the pairs the workgroup-per-token kernel lists (group epilogue, round 3); otherwise two launches
    fused_acc = groupsize == 128 and (flags & (FQ_OUT_PACKED | FQ_OUT_FAKEQUANT | FQ_QUANT_F16)) == FQ_OUT_PACKED \
        and n == 1 and N == 64 and M % 2 == 0 and diag is None and dt == torch.float16
    fused_rnd = groupsize == 128 and n == 1 and bool(flags & FQ_ROUND_Y_F16) and bool(flags & (FQ_OUT_PACKED | FQ_OUT_FAKEQUANT))
    fused_g = fused_acc or fused_rnd

    def two_launches():
        o2 = kron_quant(x, left, right, flags=FQ_OUT_TRANSFORM | (flags & FQ_WS_PREPARED), diag=diag)
        return _quant_groups_of(o2.y, sigs, flags, 128, o2) if flags & (FQ_OUT_PACKED | FQ_OUT_FAKEQUANT) else o2

    if groupsize == 128 and not fused_g:
        return two_launches()
    o = _alloc_outputs(x, rows * (d // 128 if fused_g else 1), d, n, flags, x.shape[:-1] + (d // 2,), x.shape)
    if fused_g:
        _group_scales_shape(o, x.shape[:-1], d // 128)
        flags |= FQ_GROUP128
    if rows == 0:
        return o
    with _on(x.device):
        ws, ws_bytes, prepared, key = _kron_workspace(x.device, M, N, left, right)
        rc = _fn("kron_quant", dt)(_ptr(x), _ptr(left), _ptr(right), _ptr(diag), rows, M, N, smax, smin, n,
                                   flags | (FQ_WS_PREPARED if prepared else 0), _ptr_array(o.q), _ptr_array(o.scale),
                                   _ptr_array(o.fq), _ptr(o.y), _ptr(ws), ws_bytes, _stream(x))
        if rc == _lib.FQ_EUNSUPPORTED and fused_rnd:     # a pair without a group epilogue: the reference's own two steps
            return two_launches()
        check(rc)
        if key is not None and not prepared:
            _kron_workspace_commit(key, ws, left, right)
    return o


class LaunchPlan:
    """A prepared library call with STATIC outputs (round 4, the host path of VERDICT r03 item 4c): shapes, dtype, device, the factor pair /
    clip sets, the output tensors, the fragment image and the ctypes argument list are fixed at construction; ``run(x)`` swaps in x's
    address and the current stream and makes ONE foreign call — no allocation, no cache look-up, no argument conversion beyond ctypes'
    own (tools/host_overhead.py: ~5 us per call where the general entry point spends 14-17). The outputs are REUSED by every call, as
    under a captured graph: a caller that needs the previous result after the next call must copy it. Built by kron_plan() /
    rowquant_plan(); ``result`` is whatever the builder put there (a FusedOutputs, or a module's PackedQuantizedTensor)."""
    __slots__ = ("fn", "args", "shape", "dtype", "device", "dev_index", "keep", "result", "outputs")

    def run(self, x: torch.Tensor):
        if x.shape != self.shape or x.dtype != self.dtype or x.device != self.device or not x.is_contiguous():
            raise ValueError(f"LaunchPlan: built for a contiguous {self.dtype} tensor of shape {tuple(self.shape)} on {self.device}, "
                             f"got {x.dtype} {tuple(x.shape)} on {x.device}")
        a = self.args
        a[0] = x.data_ptr()
        a[-1] = _stream_handle(self.device)
        if torch.cuda.current_device() != self.dev_index:
            with _on(self.device):
                rc = self.fn(*a)
        else:
            rc = self.fn(*a)
        if rc:
            check(rc)
        return self.result

    def run2(self, x: torch.Tensor, x2: torch.Tensor):
        """run() for entry points with two per-call inputs (argument 1 = x2: the packed activations AND their scales of a linear)"""
        self.args[1] = x2.data_ptr()
        return self.run(x)


class FreshPlan:
    """A prepared library call whose arguments live on the C side (fq_plan_*, round 5 — the host path of VERDICT r04 item 6a): every
    ``run`` allocates FRESH outputs (no aliasing between calls, unlike LaunchPlan's static buffers) and makes one foreign call with five
    pointers — ~8 us of Python per module call where the general entry points spend 14-20 (tools/host_overhead.py), same bits out.
    Built for one input shape / dtype / device and one set of matrices / clip factors; the owner (a deploy.nn module) re-plans when any
    of them changes. Not used under stream capture (a captured graph must not hold pointers into a plan the owner may rebuild)."""
    __slots__ = ("handle", "shape", "dtype", "dev_index", "device", "keep", "q_shape", "s_shape", "s_dtype", "__weakref__")

    def __init__(self, handle, x_like: torch.Tensor, q_shape, s_shape, s_dtype, keep):
        if not handle:
            raise _lib.FqError(_lib.FQ_EINVAL, lib.fq_last_error().decode("utf-8", "replace"))
        self.handle = ctypes.c_void_p(handle)
        self.shape, self.dtype, self.device = x_like.shape, x_like.dtype, x_like.device
        self.dev_index = x_like.device.index if x_like.device.index is not None else torch.cuda.current_device()
        self.q_shape, self.s_shape, self.s_dtype, self.keep = q_shape, s_shape, s_dtype, keep

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and lib is not None:      # (at interpreter shutdown the module globals may already be gone)
            lib.fq_plan_free(h)

    def matches(self, x: torch.Tensor) -> bool:
        return x.shape == self.shape and x.dtype == self.dtype and x.device == self.device

    def run(self, x: torch.Tensor):
        """-> (q uint8 ``q_shape``, scales ``s_shape``): fresh tensors. x: contiguous, ``matches(x)`` (the caller has checked)."""
        q = torch.empty(self.q_shape, dtype=torch.uint8, device=self.device)
        sc = torch.empty(self.s_shape, dtype=self.s_dtype, device=self.device)
        if torch.cuda.current_device() != self.dev_index:
            with _on(self.device):
                rc = lib.fq_plan_run(self.handle, x.data_ptr(), None, q.data_ptr(), sc.data_ptr(), _stream_handle(self.device))
        else:
            rc = lib.fq_plan_run(self.handle, x.data_ptr(), None, q.data_ptr(), sc.data_ptr(), _stream_handle(self.device))
        if rc:
            check(rc)
        return q, sc

    def run_linear(self, xq: torch.Tensor, xs: torch.Tensor):
        """skinny linear plans: (packed x, its fp16 scales) -> fresh y of ``q_shape`` (fp16)"""
        y = torch.empty(self.q_shape, dtype=torch.float16, device=self.device)
        if torch.cuda.current_device() != self.dev_index:
            with _on(self.device):
                rc = lib.fq_plan_run(self.handle, xq.data_ptr(), xs.data_ptr(), y.data_ptr(), None, _stream_handle(self.device))
        else:
            rc = lib.fq_plan_run(self.handle, xq.data_ptr(), xs.data_ptr(), y.data_ptr(), None, _stream_handle(self.device))
        if rc:
            check(rc)
        return y


class FreshPlanSet:
    """The FreshPlans of ONE deploy.nn module: one per input (shape, dtype, device) — a server alternating prefill- and decode-sized
    calls keeps both instead of re-planning on every switch — at most ``KEEP``, all dropped when ``key`` (the owner's matrices / clip
    factors / cache epoch, as ids and versions) changes. ``refs`` keeps the objects whose ids are in the key alive."""
    __slots__ = ("key", "refs", "plans", "last")
    KEEP = 4

    def __init__(self):
        self.key, self.refs, self.plans, self.last = None, None, {}, None

    def lookup(self, key, x: torch.Tensor):
        if key != self.key:
            self.key, self.refs, self.last = key, None, None
            self.plans.clear()
            return None
        p = self.last
        if p is not None and p.matches(x):
            return p
        p = self.plans.get((x.shape, x.dtype, x.device))
        if p is not None:
            self.last = p
        return p

    def add(self, x: torch.Tensor, plan: "FreshPlan", refs=None):
        if len(self.plans) >= self.KEEP:
            self.plans.pop(next(iter(self.plans)))           # (insertion order: the oldest)
        self.plans[(x.shape, x.dtype, x.device)] = plan
        self.last, self.refs = plan, refs
        return plan


def kron_fresh_plan(x_like: torch.Tensor, left: torch.Tensor, right: torch.Tensor, sig: Sig, flags: int, q_shape, s_shape) -> FreshPlan:
    """deploy.nn.OnlineTrans(matmul, decompose).forward as a FreshPlan: one clip pair, packed output; the fragment image is prepared
    here and kept by the plan (as are left / right: their addresses cannot be recycled under it)."""
    dt = _chk_act(x_like)
    _chk(left, "left", dt), _chk(right, "right", dt)
    M, N = left.shape[0], right.shape[0]
    d = M * N
    if left.shape != (M, M) or right.shape != (N, N) or x_like.shape[-1] != d or x_like.numel() == 0:
        raise ValueError("kron_fresh_plan: x [..., M*N] (not empty), left [M, M], right [N, N]")
    rows = x_like.numel() // d
    with _on(x_like.device):
        nbytes = int(lib.fq_kron_workspace_bytes(M, N))
        if nbytes < 0:
            raise _lib.FqError(nbytes, f"no kernel for Kronecker factors ({M}, {N})")
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x_like.device)
        if nbytes:
            check(_fn("kron_prepare", dt)(_ptr(left), _ptr(right), M, N, _ptr(ws), nbytes, _stream(x_like)))
    h = lib.fq_plan_kron(int(dt == torch.bfloat16), left.data_ptr(), right.data_ptr(), rows, M, N, float(sig[0]), float(sig[1]),
                         (flags & ~FQ_WS_PREPARED) | (FQ_WS_PREPARED if nbytes else 0), ws.data_ptr() if nbytes else None, nbytes)
    return FreshPlan(h, x_like, q_shape, s_shape, dt, (left, right, ws))


def rowquant_fresh_plan(x_like: torch.Tensor, sig: Sig, flags: int, q_shape, s_shape) -> FreshPlan:
    """deploy.nn.Quantizer.forward as a FreshPlan (one clip pair, packed output)."""
    dt = _chk_act(x_like)
    cols = x_like.shape[-1]
    if x_like.numel() == 0:
        raise ValueError("rowquant_fresh_plan: empty input")
    h = lib.fq_plan_rowquant(int(dt == torch.bfloat16), x_like.numel() // cols, cols, float(sig[0]), float(sig[1]), flags)
    return FreshPlan(h, x_like, q_shape, s_shape, dt, ())


def skinny_linear_fresh_plan(x_like: torch.Tensor, w_image: torch.Tensor, w_scale: torch.Tensor, bias: Optional[torch.Tensor], N: int,
                             y_shape) -> FreshPlan:
    """the decode-sized Linear4bit.forward (fq_int4_skinny_linear_f16) as a FreshPlan: ``plan.run_linear(x_packed, x_scales)`` -> a fresh
    fp16 ``y_shape`` tensor. x_scales: contiguous fp16 of M elements (the caller checks)."""
    _chk(x_like, "x", torch.uint8), _chk(w_scale, "w_scale")
    if bias is not None:
        _chk(bias, "bias")
    K = x_like.shape[-1] * 2
    M = x_like.numel() // x_like.shape[-1] if x_like.numel() else 0
    if M == 0 or w_scale.numel() != N:
        raise ValueError("skinny_linear_fresh_plan: empty input or w_scale size")
    h = lib.fq_plan_skinny_linear(w_image.data_ptr(), w_scale.data_ptr(), None if bias is None else bias.data_ptr(), M, N, K)
    return FreshPlan(h, x_like, y_shape, None, None, (w_image, w_scale, bias))


def skinny_linear_plan(x_like: torch.Tensor, w_image: torch.Tensor, w_scale: torch.Tensor, bias: Optional[torch.Tensor], N: int) -> LaunchPlan:
    """int4_skinny_linear (M <= 128 rows against a decode weight image) as a LaunchPlan: ``plan.run2(x_packed, x_scale)`` -> the static
    fp16 [M, N] output. x_scale must be a contiguous fp16 tensor of M elements (not re-checked per call)."""
    _chk(x_like, "x", torch.uint8), _chk(w_scale, "w_scale")
    if bias is not None:
        _chk(bias, "bias")
    M, K = x_like.shape[0], x_like.shape[1] * 2
    if M == 0 or w_scale.numel() != N:
        raise ValueError("skinny_linear_plan: empty input or w_scale size")
    y = torch.empty((M, N), dtype=torch.float16, device=x_like.device)
    plan = LaunchPlan()
    plan.fn = lib.fq_int4_skinny_linear_f16
    plan.args = [0, 0, w_image.data_ptr(), w_scale.data_ptr(), None if bias is None else bias.data_ptr(), M, N, K, y.data_ptr(), 0]
    plan.shape, plan.dtype, plan.device = x_like.shape, torch.uint8, x_like.device
    plan.dev_index = x_like.device.index if x_like.device.index is not None else torch.cuda.current_device()
    plan.keep = (w_image, w_scale, bias, y)
    plan.outputs = plan.result = y
    return plan


def kron_plan(x_like: torch.Tensor, left: torch.Tensor, right: torch.Tensor, sigs: Sequence[Sig] = ((1.0, 1.0),),
              flags: int = FQ_OUT_PACKED) -> LaunchPlan:
    """kron_quant(x, left, right, sigs, flags) as a LaunchPlan for inputs shaped like ``x_like`` (per-token scales, no diag). The fragment
    image is prepared here; the plan keeps left / right alive and is only valid while they are not modified (the caller re-plans on a new
    ``_version``, as deploy.nn.OnlineTrans does)."""
    dt = _chk_act(x_like)
    _chk(left, "left", dt), _chk(right, "right", dt)
    M, N = left.shape[0], right.shape[0]
    d = M * N
    if left.shape != (M, M) or right.shape != (N, N) or x_like.shape[-1] != d:
        raise ValueError("kron_plan: x [..., M*N], left [M, M], right [N, N]")
    rows = x_like.numel() // d
    if rows == 0:
        raise ValueError("kron_plan: empty input")
    smax, smin, n = _sig_arrays(sigs)
    o = _alloc_outputs(x_like, rows, d, n, flags, x_like.shape[:-1] + (d // 2,), x_like.shape)
    plan = LaunchPlan()
    with _on(x_like.device):
        nbytes = int(lib.fq_kron_workspace_bytes(M, N))
        if nbytes < 0:
            raise _lib.FqError(nbytes, f"no kernel for Kronecker factors ({M}, {N})")
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x_like.device)
        if nbytes:
            check(_fn("kron_prepare", dt)(_ptr(left), _ptr(right), M, N, _ptr(ws), nbytes, _stream(x_like)))
    qa, sa, fa = _ptr_array(o.q), _ptr_array(o.scale), _ptr_array(o.fq)
    plan.fn = _fn("kron_quant", dt)
    plan.args = [0, left.data_ptr(), right.data_ptr(), None, rows, M, N, smax, smin, n, flags | (FQ_WS_PREPARED if nbytes else 0), qa, sa, fa,
                 _ptr(o.y), ws.data_ptr() if nbytes else None, nbytes, 0]
    plan.shape, plan.dtype, plan.device = x_like.shape, dt, x_like.device
    plan.dev_index = x_like.device.index if x_like.device.index is not None else torch.cuda.current_device()
    plan.keep = (left, right, ws, qa, sa, fa, smax, smin)
    plan.outputs = plan.result = o
    return plan


def rowquant_plan(x_like: torch.Tensor, sigs: Sequence[Sig] = ((1.0, 1.0),), flags: int = FQ_OUT_PACKED) -> LaunchPlan:
    """rowquant(x, sigs, flags) as a LaunchPlan for inputs shaped like ``x_like``."""
    dt = _chk_act(x_like)
    cols = x_like.shape[-1]
    rows = x_like.numel() // cols
    if rows == 0:
        raise ValueError("rowquant_plan: empty input")
    smax, smin, n = _sig_arrays(sigs)
    o = _alloc_outputs(x_like, rows, cols, n, flags, x_like.shape[:-1] + (cols // 2,), x_like.shape)
    qa, sa, fa = _ptr_array(o.q), _ptr_array(o.scale), _ptr_array(o.fq)
    plan = LaunchPlan()
    plan.fn = _fn("rowquant", dt)
    plan.args = [0, rows, cols, smax, smin, n, flags, qa, sa, fa, 0]
    plan.shape, plan.dtype, plan.device = x_like.shape, dt, x_like.device
    plan.dev_index = x_like.device.index if x_like.device.index is not None else torch.cuda.current_device()
    plan.keep = (qa, sa, fa, smax, smin)
    plan.outputs = plan.result = o
    return plan


class KronMultiPlan:
    """A prepared multi-job launch (fq_kron_quant_multi_{f16,bf16}): several independent 64 x 64 transform + quantisation jobs — a
    layer each — as ONE kernel launch. Build once (the device job table, the fragment images and the outputs are kept), call
    ``run()`` per step. ``xs[j]`` [rows_j, 4096] (fixed buffers: the table holds their addresses), ``lefts[j]`` / ``rights[j]``
    [64, 64]; one clip pair and one flag set (FQ_OUT_PACKED, optionally FQ_NO_CLAMP0) for all jobs. Bit for bit the results of
    ``kron_quant(xs[j], lefts[j], rights[j], [sig], flags)`` for every j."""

    def __init__(self, xs: Sequence[torch.Tensor], lefts: Sequence[torch.Tensor], rights: Sequence[torch.Tensor], sig: Sig = (1.0, 1.0),
                 flags: int = FQ_OUT_PACKED | FQ_NO_CLAMP0):
        if not (len(xs) == len(lefts) == len(rights)) or len(xs) == 0:
            raise ValueError("KronMultiPlan: xs, lefts, rights must be non-empty and of one length")
        self.dtype = _chk_act(xs[0])
        dev = xs[0].device
        for x, l, r in zip(xs, lefts, rights):
            _chk(x, "x", self.dtype), _chk(l, "left", self.dtype), _chk(r, "right", self.dtype)
            if x.shape[-1] != 4096 or l.shape != (64, 64) or r.shape != (64, 64) or x.device != dev:
                raise ValueError("KronMultiPlan: 64 x 64 factor pairs on d = 4096 activations of one device")
        self.sig, self.flags, self.n = sig, flags, len(xs)
        self.xs = list(xs)
        wsb = int(lib.fq_kron_workspace_bytes(64, 64))
        prep = _fn("kron_prepare", self.dtype)
        self.ws, self.q, self.scale = [], [], []
        jobs = (_lib.FqKronJob * self.n)()
        with _on(dev):
            st = _stream(xs[0])
            for j, (x, l, r) in enumerate(zip(xs, lefts, rights)):
                rows = x.numel() // 4096
                w = torch.empty(wsb, dtype=torch.uint8, device=dev)
                check(prep(_ptr(l), _ptr(r), 64, 64, _ptr(w), wsb, st))
                q = torch.empty(x.shape[:-1] + (2048,), dtype=torch.uint8, device=dev)
                s = torch.empty((rows,), dtype=self.dtype, device=dev)
                self.ws.append(w), self.q.append(q), self.scale.append(s)
                jobs[j] = _lib.FqKronJob(x.data_ptr(), w.data_ptr(), q.data_ptr(), s.data_ptr(), rows)
            tb = int(lib.fq_kron_multi_table_bytes(self.n))
            self.table = torch.empty(tb, dtype=torch.uint8, device=dev)
            rc = lib.fq_kron_multi_prepare(ctypes.cast(jobs, ctypes.c_void_p), self.n, _ptr(self.table), tb, st)
            if rc <= 0:
                check(rc if rc < 0 else _lib.FQ_EINVAL)
            self.wg_per_job = rc
        self._fn = _fn("kron_quant_multi", self.dtype)

    def run(self):
        """-> (q list, scale list): the kept output tensors, rewritten by this launch"""
        with _on(self.table.device):
            check(self._fn(_ptr(self.table), self.n, self.wg_per_job, ctypes.c_float(self.sig[0]), ctypes.c_float(self.sig[1]),
                           self.flags, _stream(self.table)))
        return self.q, self.scale


def kron_quant_ex(x: torch.Tensor, left: torch.Tensor, right: torch.Tensor, post_scale: float = 1.0,
                  sigs: Sequence[Sig] = ((1.0, 1.0),), flags: int = FQ_OUT_PACKED, up: Optional[torch.Tensor] = None) -> FusedOutputs:
    """fq_kron_quant_ex_f16: fq_kron_quant_f16 whose transformed activation is multiplied by ``post_scale`` (fp32) before
    rounding / quantisation, optionally with x = gate and the transform's input fp16(up * fp16(silu(gate)))."""
    _chk(x, "x"), _chk(left, "left"), _chk(right, "right")
    if up is not None:
        _chk(up, "up")
        if up.shape != x.shape:
            raise ValueError("up must have x's shape")
    M, N = left.shape[0], right.shape[0]
    d = M * N
    if x.shape[-1] != d or left.shape != (M, M) or right.shape != (N, N):
        raise ValueError("shape mismatch between x, left and right")
    rows = x.numel() // d
    smax, smin, n = _sig_arrays(sigs)
    o = _alloc_outputs(x, rows, d, n, flags, x.shape[:-1] + (d // 2,), x.shape)
    if rows == 0:
        return o
    with _on(x.device):
        ws, ws_bytes, prepared, key = _kron_workspace(x.device, M, N, left, right)
        check(lib.fq_kron_quant_ex_f16(_ptr(x), _ptr(up), _ptr(left), _ptr(right), rows, M, N, ctypes.c_float(post_scale), smax,
                                       smin, n, flags | (FQ_WS_PREPARED if prepared else 0), _ptr_array(o.q),
                                       _ptr_array(o.scale), _ptr_array(o.fq), _ptr(o.y), _ptr(ws), ws_bytes, _stream(x)))
        if key is not None and not prepared:
            _kron_workspace_commit(key, ws, left, right)
    return o


# The online Hadamard rotation of n = K * P (hadK (x) H_P, 1/sqrt(n)) in front of the deploy Quantizer as ONE Kronecker
# launch: x.view(K * P / N, N) -> left = kron(hadK, H_{P/N}) (+-1), right = H_N / 16, post_scale = 16 / sqrt(n). The
# factor pair is built once per (hadK, P) and kept (the fragment workspace cache is keyed by these tensors).
_HAD_KRON: "collections.OrderedDict" = CACHES.register("hadamard_factor_pairs", collections.OrderedDict())


def _sylvester(n: int) -> torch.Tensor:
    h = torch.ones(1, 1, dtype=torch.float32)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def _had_right_div(N: int) -> float:
    """The +-1 Sylvester factor is stored as +-1/div (sqrt(N) up to a power of two: the fp16 intermediate keeps the
    activation's range); the launch's post-scale carries the div back."""
    return 16.0 if N >= 128 else 8.0


def _hadamard_as_kron(K: int, P: int, hadK: Optional[torch.Tensor], device):
    """-> (left [M, M], right [N, N], post_scale) or None when the pair is not one the fused kernels take."""
    if K == 1 or hadK is None:
        return None
    for N in (128, 256, 64):
        M = K * (P // N) if P % N == 0 else 0
        # factor pairs with a packed-only kernel of their own: M in (64, 128] with N = 128 (three token groups per CU),
        # M in (96, 128] with N = 256 (workgroup per token), M in (64, 192] with N = 64 (a wave per row tile: 11008 = 172 x 64)
        if (N == 128 and 64 < M <= 128) or (N == 256 and 96 < M <= 128) or (N == 64 and 64 < M <= 192):
            key = (hadK.data_ptr(), ver(hadK), K, P, N, str(device))
            hit = _HAD_KRON.get(key)
            if hit is None:
                # out = hadK @ x.view(K, P): Y = L^T U contracts L's FIRST index, so L = kron(hadK, H)^T = kron(hadK^T, H)
                left = torch.kron(hadK.detach().float().cpu().T.contiguous(), _sylvester(P // N)).to(torch.float16).contiguous().to(device)
                right = (_sylvester(N) / _had_right_div(N)).to(torch.float16).contiguous().to(device)
                hit = (left, right, hadK)
                _HAD_KRON[key] = hit
                if len(_HAD_KRON) > 32:
                    _HAD_KRON.popitem(last=False)
            return hit[0], hit[1], N
    return None


def moe_group_rows(indices: torch.Tensor, n_groups: int):
    """(token, slot) pairs of a top-k routing table sorted by expert — the device-side form of the reference's
    ``counts = torch.bincount(indices.flatten(), minlength=E)`` + ``idx, top = torch.where(indices == i)`` loop
    (flatquant/model_tools/deepseekv3_utils.py:434-439), without the host round trip of ``.tolist()``.
    indices [T, k] integer -> (token_idx [T*k] int64: source row of every grouped row, in expert order and, inside an
    expert, in token order like torch.where; group_offsets [n_groups + 1] int64). Plumbing only (torch sort/bincount)."""
    flat = indices.reshape(-1).to(torch.int64)
    order = torch.sort(flat, stable=True).indices                   # stable: token order inside an expert
    counts = torch.bincount(flat, minlength=n_groups)
    offsets = torch.zeros(n_groups + 1, dtype=torch.int64, device=indices.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return order // indices.shape[-1], offsets


def kron_quant_grouped(x: torch.Tensor, left: torch.Tensor, right: torch.Tensor, group_offsets: torch.Tensor,
                       sig_max_g: torch.Tensor, sig_min_g: torch.Tensor, flags: int = FQ_OUT_PACKED,
                       groupsize: int = -1) -> FusedOutputs:
    """Grouped (per-expert) transform + quantisation (fq_kron_quant_grouped_f16): x [rows, d] sorted by group, group g
    owns rows [group_offsets[g], group_offsets[g+1]) and quantises with sigmoid factors (sig_max_g[g], sig_min_g[g])
    (fp32 device tensors; the reference shares ONE quantiser across the routed experts: expand it). One launch, nothing
    read back: 2-D left / right = the shared transform (deepseekv3_utils.py:470), fq_kron_quant_grouped_*; 3-D left / right
    [G, M, M] / [G, N, N] = the reference's ``routed_w2_trans[i]`` branch (:443-446), fq_kron_quant_grouped_mats_* (one
    fragment image per group in the cached workspace; the reference loops over the experts on the host with ``.tolist()``)."""
    dt = _chk_act(x)
    _chk(left, "left", dt), _chk(right, "right", dt)
    _chk(group_offsets, "group_offsets", torch.int64)
    _chk(sig_max_g, "sig_max_g", torch.float32), _chk(sig_min_g, "sig_min_g", torch.float32)
    G = group_offsets.numel() - 1
    if G < 1 or sig_max_g.numel() != G or sig_min_g.numel() != G:
        raise ValueError("group_offsets must have n_groups + 1 entries and sig_*_g n_groups")
    M, N = left.shape[-1], right.shape[-1]
    d = M * N
    if x.dim() != 2 or x.shape[1] != d:
        raise ValueError(f"x must be [rows, {M}*{N}]")
    if groupsize not in (-1, 128) or (groupsize == 128 and d % 128):
        raise ValueError("groupsize must be -1 (per token) or 128 with M*N % 128 == 0")
    rows = x.shape[0]
    if left.dim() == 3 or right.dim() == 3:                        # one transform per expert
        if left.shape[0] != G or right.shape[0] != G or left.dim() != 3 or right.dim() != 3:
            raise ValueError("per-group matrices must be [n_groups, M, M] and [n_groups, N, N]")
        if groupsize > 0:
            # 128-element scales next to per-expert matrices: the grouped transform launch, then the row quantiser over the
            # (-1, 128) view — the row quantiser takes one clip pair per launch, so the groups' pairs must agree (the reference
            # shares one quantiser across the routed experts: deepseekv3_utils.py:418-419)
            if not (bool((sig_max_g == sig_max_g[0]).all()) and bool((sig_min_g == sig_min_g[0]).all())):
                raise _lib.FqError(FQ_EUNSUPPORTED, "per-expert matrices with 128-element scales need one shared clip pair")
            o = kron_quant_grouped(x, left, right, group_offsets, sig_max_g, sig_min_g, FQ_OUT_TRANSFORM)
            sig = (float(sig_max_g[0]), float(sig_min_g[0]))
            return _quant_groups_of(o.y, [sig], flags, groupsize, o) if flags & (FQ_OUT_PACKED | FQ_OUT_FAKEQUANT) else o
        o = _alloc_outputs(x, rows, d, 1, flags, (rows, d // 2), x.shape)
        if rows == 0:
            return o
        with _on(x.device):
            per = _WS_BYTES.get((M, N))
            if per is None:
                per = _WS_BYTES[(M, N)] = int(lib.fq_kron_workspace_bytes(M, N))
            if per < 0:
                raise _lib.FqError(per, f"no kernel for Kronecker factors ({M}, {N})")
            key = (x.device.index, _stream_handle(x.device), M, N, G,
                   left.data_ptr(), ver(left), right.data_ptr(), ver(right))
            ent = _WS_LRU.get(key)
            if ent is None:
                ent = _ws_shared(key)      # (prepared on another stream: see _kron_workspace)
            else:
                _pin_for_capture(ent)
            prepared = ent is not None
            ws = ent[0] if prepared else torch.empty(per * G, dtype=torch.uint8, device=x.device)
            check(_fn("kron_quant_grouped_mats", dt)(
                _ptr(x), _ptr(left), _ptr(right), rows, M, N, _ptr(group_offsets), G, _ptr(sig_max_g), _ptr(sig_min_g),
                flags | (FQ_WS_PREPARED if prepared else 0), _ptr(o.q[0] if o.q else None), _ptr(o.scale[0] if o.scale else None),
                _ptr(o.fq[0] if o.fq else None), _ptr(o.y), _ptr(ws), per * G, _stream(x)))
            if not prepared:
                _kron_workspace_commit(key, ws, left, right)
            else:
                _WS_LRU.move_to_end(key)
        return o
    fused_g = groupsize == 128 and ((flags & (FQ_OUT_PACKED | FQ_OUT_FAKEQUANT)) == FQ_OUT_PACKED and N == 64
                                    and M % 2 == 0 and dt == torch.float16
                                    or bool(flags & FQ_ROUND_Y_F16) and bool(flags & (FQ_OUT_PACKED | FQ_OUT_FAKEQUANT)))
    if groupsize == 128 and not fused_g:
        raise _lib.FqError(FQ_EUNSUPPORTED, "grouped launch with 128-element scales: packed output at N = 64, or FQ_ROUND_Y_F16 "
                           "(the group epilogue quantises the transform rounded to x's dtype)")
    o = _alloc_outputs(x, rows * (d // 128 if fused_g else 1), d, 1, flags, (rows, d // 2), x.shape)
    if fused_g:
        _group_scales_shape(o, (rows,), d // 128)
        flags |= FQ_GROUP128
    if rows == 0:
        return o
    with _on(x.device):
        ws, ws_bytes, prepared, key = _kron_workspace(x.device, M, N, left, right)
        check(_fn("kron_quant_grouped", dt)(
            _ptr(x), _ptr(left), _ptr(right), rows, M, N, _ptr(group_offsets), G, _ptr(sig_max_g), _ptr(sig_min_g),
            flags | (FQ_WS_PREPARED if prepared else 0), _ptr(o.q[0] if o.q else None), _ptr(o.scale[0] if o.scale else None),
            _ptr(o.fq[0] if o.fq else None), _ptr(o.y), _ptr(ws), ws_bytes, _stream(x)))
        if key is not None and not prepared:
            _kron_workspace_commit(key, ws, left, right)
    return o


def rmsnorm(x: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """deploy.nn.RMSNorm (deploy/nn/normalization.py:16-23): fp16 in, fp16 out, no weight (fq_rmsnorm_f16)."""
    _chk(x, "x")
    cols = x.shape[-1]
    rows = x.numel() // cols
    y = torch.empty_like(x)
    if rows == 0:
        return y
    with _on(x.device):
        check(lib.fq_rmsnorm_f16(_ptr(x), _ptr(y), rows, cols, ctypes.c_float(eps), _stream(x)))
    return y


def rmsnorm_kron_quant(x: torch.Tensor, eps: float, left: torch.Tensor, right: torch.Tensor,
                       sigs: Sequence[Sig] = ((1.0, 1.0),), flags: int = FQ_OUT_PACKED) -> FusedOutputs:
    """RMSNorm + Kronecker transform + INT4 quantisation in one launch: fq_rmsnorm_kron_quant_f16 for the 64 x 64 factor
    pair, fq_rmsnorm_kron_quant_ws_f16 (packed output) for the wave-per-token pairs (64 x 128, 64 x 112, 56 x 64, 64 x 80,
    32 x 64); any other pair / output set runs rmsnorm() and kron_quant() one after the other (same arithmetic, one more
    round trip)."""
    _chk(x, "x"), _chk(left, "left"), _chk(right, "right")
    M, N = left.shape[0], right.shape[0]
    # (the wave kernel's one-row-tile instantiation exists for N = 64 only: 32 x 128, 32 x 112 ... take the two-launch route)
    wave_pair = M <= 64 and N in (64, 80, 112, 128) and (M, N) != (64, 64) and (M * (N // 8)) % 64 == 0 and (M > 32 or N == 64)
    if wave_pair and (flags & (FQ_OUT_PACKED | FQ_OUT_FAKEQUANT | FQ_OUT_TRANSFORM | FQ_QUANT_F16)) == FQ_OUT_PACKED:
        d = M * N
        if x.shape[-1] != d:
            raise ValueError(f"x.shape[-1]={x.shape[-1]} != {M}*{N}")
        rows = x.numel() // d
        smax, smin, n = _sig_arrays(sigs)
        o = _alloc_outputs(x, rows, d, n, flags, x.shape[:-1] + (d // 2,), x.shape)
        if rows == 0:
            return o
        with _on(x.device):
            ws, ws_bytes, prepared, key = _kron_workspace(x.device, M, N, left, right)
            check(lib.fq_rmsnorm_kron_quant_ws_f16(_ptr(x), ctypes.c_float(eps), _ptr(left), _ptr(right), rows, M, N, smax, smin,
                                                   n, flags | (FQ_WS_PREPARED if prepared else 0), _ptr_array(o.q),
                                                   _ptr_array(o.scale), _ptr_array(o.fq), _ptr(o.y), _ptr(ws), ws_bytes, _stream(x)))
            if key is not None and not prepared:
                _kron_workspace_commit(key, ws, left, right)
        return o
    if (M, N) != (64, 64) or (flags & (FQ_OUT_FAKEQUANT | FQ_QUANT_F16)):
        return kron_quant(rmsnorm(x, eps), left, right, sigs, flags)
    d = M * N
    if x.shape[-1] != d:
        raise ValueError(f"x.shape[-1]={x.shape[-1]} != {M}*{N}")
    rows = x.numel() // d
    smax, smin, n = _sig_arrays(sigs)
    o = _alloc_outputs(x, rows, d, n, flags, x.shape[:-1] + (d // 2,), x.shape)
    if rows == 0:
        return o
    with _on(x.device):
        check(lib.fq_rmsnorm_kron_quant_f16(_ptr(x), ctypes.c_float(eps), _ptr(left), _ptr(right), rows, M, N, smax, smin,
                                            n, flags, _ptr_array(o.q), _ptr_array(o.scale), _ptr_array(o.fq), _ptr(o.y),
                                            _stream(x)))
    return o


def silu_mul(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """x_up * act_fn(x_gate) with act_fn = SiLU on fp16 tensors (modeling_llama.py:277-278), one launch."""
    _chk(gate, "gate"), _chk(up, "up")
    if gate.shape != up.shape:
        raise ValueError("gate and up must have the same shape")
    y = torch.empty_like(gate)
    if gate.numel() == 0:
        return y
    with _on(gate.device):
        check(lib.fq_silu_mul_f16(_ptr(gate), _ptr(up), _ptr(y), gate.numel(), _stream(gate)))
    return y


def silu_mul_kron_quant(gate: torch.Tensor, up: torch.Tensor, left: torch.Tensor, right: torch.Tensor,
                        sigs: Sequence[Sig] = ((1.0, 1.0),), flags: int = FQ_OUT_PACKED) -> FusedOutputs:
    """kron_quant(up * silu(gate), ...) with the product formed inside the transform launch
    (fq_silu_mul_kron_quant_f16, factor pairs with M > 64); other pairs run silu_mul() + kron_quant()."""
    _chk(gate, "gate"), _chk(up, "up"), _chk(left, "left"), _chk(right, "right")
    if gate.shape != up.shape:
        raise ValueError("gate and up must have the same shape")
    M, N = left.shape[0], right.shape[0]
    if left.shape != (M, M) or right.shape != (N, N):
        raise ValueError("left/right must be square")
    d = M * N
    if gate.shape[-1] != d:
        raise ValueError(f"gate.shape[-1]={gate.shape[-1]} != {M}*{N}")
    rows = gate.numel() // d
    smax, smin, n = _sig_arrays(sigs)
    o = _alloc_outputs(gate, rows, d, n, flags, gate.shape[:-1] + (d // 2,), gate.shape)
    if rows == 0:
        return o
    with _on(gate.device):
        ws, ws_bytes, prepared, key = _kron_workspace(gate.device, M, N, left, right)
        rc = lib.fq_silu_mul_kron_quant_f16(_ptr(gate), _ptr(up), _ptr(left), _ptr(right), rows, M, N, smax, smin, n,
                                            flags | (FQ_WS_PREPARED if prepared else 0), _ptr_array(o.q),
                                            _ptr_array(o.scale), _ptr_array(o.fq), _ptr(o.y), _ptr(ws), ws_bytes,
                                            _stream(gate))
        if rc == _lib.FQ_EUNSUPPORTED:
            return kron_quant(silu_mul(gate, up), left, right, sigs, flags)
        check(rc)
        if key is not None and not prepared:
            _kron_workspace_commit(key, ws, left, right)
    return o


def block_quant(x: torch.Tensor, P: torch.Tensor, sigs: Sequence[Sig] = ((1.0, 1.0),),
                flags: int = FQ_OUT_PACKED | FQ_NO_CLAMP0, transpose_out: bool = True) -> FusedOutputs:
    """x [..., R, C] @ P [C, C], quantised per [R, C] block (fq_block_quant_f16 / _bf16 by x's dtype)."""
    dt = _chk_act(x)
    _chk(P, "P", dt)
    R, C = x.shape[-2], x.shape[-1]
    if P.shape != (C, C):
        raise ValueError("P must be [C, C] with C = x.shape[-1]")
    d = R * C
    rows = x.numel() // d
    smax, smin, n = _sig_arrays(sigs)
    yshape = x.shape[:-2] + ((C, R) if transpose_out else (R, C))
    o = _alloc_outputs(x, rows, d, n, flags, x.shape[:-2] + (d // 2,), yshape)
    if rows == 0:
        return o
    with _on(x.device):
        check(_fn("block_quant", dt)(_ptr(x), _ptr(P), rows, R, C, int(transpose_out), smax, smin, n, flags,
                                     _ptr_array(o.q), _ptr_array(o.scale), _ptr_array(o.fq), _ptr(o.y),
                                     _stream(x)))
    return o


def single_trans(x: torch.Tensor, matrix: torch.Tensor) -> torch.Tensor:
    """x.reshape(-1, n) @ matrix in x's dtype (fq_single_trans_{f16,bf16}): {SVD,Inv}SingleTransMatrix.forward at n = 64 / 128."""
    dt = _chk_act(x)
    _chk(matrix, "matrix", dt)
    n = matrix.shape[0]
    if matrix.shape != (n, n) or x.shape[-1] != n:
        raise ValueError("single_trans: matrix [n, n] and x [..., n]")
    rows = x.numel() // n
    y = torch.empty_like(x)
    if rows:
        with _on(x.device):
            check(_fn("single_trans", dt)(_ptr(x), _ptr(matrix), rows, n, _ptr(y), _stream(x)))
    return y


def rowquant(x: torch.Tensor, sigs: Sequence[Sig] = ((1.0, 1.0),), flags: int = FQ_OUT_PACKED) -> FusedOutputs:
    """Per-token scale + INT4 quantisation of x [..., cols] (fq_rowquant_f16 / _bf16 by x's dtype)."""
    dt = _chk_act(x)
    cols = x.shape[-1]
    rows = x.numel() // cols
    smax, smin, n = _sig_arrays(sigs)
    o = _alloc_outputs(x, rows, cols, n, flags, x.shape[:-1] + (cols // 2,), x.shape)
    if rows == 0:
        return o
    with _on(x.device):
        check(_fn("rowquant", dt)(_ptr(x), rows, cols, smax, smin, n, flags, _ptr_array(o.q),
                                  _ptr_array(o.scale), _ptr_array(o.fq), _stream(x)))
    return o


def fakequant_bits(x: torch.Tensor, sig: Sig, bits: int, flags: int = 0) -> torch.Tensor:
    """ActivationQuantizer.fake_quant with bits != 4 (fq_fakequant_bits_f16 / _bf16): x [..., cols] -> the fake-quantised tensor.
    flags: FQ_ASYM, FQ_QUANT_F16 (arithmetic in the activation dtype), FQ_SIG_F16. bits == 4 is served by rowquant() (same values)."""
    dt = _chk_act(x)
    if not 2 <= int(bits) <= 8:
        raise ValueError(f"fakequant_bits: bits={bits} outside [2, 8]")
    cols = x.shape[-1]
    rows = x.numel() // cols
    y = torch.empty_like(x)
    if rows == 0:
        return y
    with _on(x.device):
        check(_fn("fakequant_bits", dt)(_ptr(x), rows, cols, ctypes.c_float(sig[0]), ctypes.c_float(sig[1]), int(bits), flags, _ptr(y),
                                        _stream(x)))
    return y


def had_mfma_supported(n: int, K: int) -> bool:
    """Shapes of the structured matrix-pipe rotation (fq_had_mfma.hip): n = K * 512 (K <= 32) or K * 1024 (K <= 28), K % 4 == 0
    (14336 = 28 * 512: Llama-3-8B ffn; 28672 = 28 * 1024: Llama-2-70B ffn)."""
    return K % 4 == 0 and ((4 <= K <= 32 and n == K * 512) or (4 <= K <= 28 and n == K * 1024))


def hadamard_mfma(x: torch.Tensor, K: int, hadK: torch.Tensor, sig: Optional[Sig] = None, scale: Optional[float] = None,
                  want_y: bool = True, up: Optional[torch.Tensor] = None):
    """fq_hadamard_quant_mfma_f16: the rotation of n = K * 512 / K * 1024 with its structure on the matrix pipe. -> (y or None, q or None,
    scales or None); ``sig`` given: the deploy Quantizer's packed output as hadamard_quant; ``want_y``: the rotated activation.
    ``up`` (with ``sig``, ``want_y=False``): x is x_gate, the rotation's input is fp16(up * fp16(silu(x))) formed inside the launch
    (fq_silu_mul_hadamard_quant_mfma_f16) — the same bytes as this function on silu_mul(x, up)."""
    _chk(x, "x"), _chk(hadK, "hadK")
    n = x.shape[-1]
    if hadK.shape != (K, K) or not had_mfma_supported(n, K):
        raise ValueError("hadamard_mfma: n = K * 512 or K * 1024 with K <= 32, K % 4 == 0 and hadK [K, K]")
    if sig is None and not want_y:
        raise ValueError("hadamard_mfma: no output requested")
    if up is not None:
        _chk(up, "up")
        if up.shape != x.shape or sig is None or want_y:
            raise ValueError("hadamard_mfma(up=...): up of x's shape, sig given, want_y=False")
    if scale is None:
        scale = float(1.0 / torch.tensor(n).sqrt())
    rows = x.numel() // n
    y = torch.empty_like(x) if want_y else None
    q = torch.empty(x.shape[:-1] + (n // 2,), dtype=torch.uint8, device=x.device) if sig is not None else None
    s = torch.empty((rows,), dtype=torch.float16, device=x.device) if sig is not None else None
    if rows > 0 and up is not None:
        with _on(x.device):
            check(lib.fq_silu_mul_hadamard_quant_mfma_f16(_ptr(x), _ptr(up), rows, n, K, _ptr(hadK), ctypes.c_float(scale),
                                                          ctypes.c_float(sig[0]), ctypes.c_float(sig[1]), _ptr(q), _ptr(s), _stream(x)))
    elif rows > 0:
        with _on(x.device):
            check(lib.fq_hadamard_quant_mfma_f16(_ptr(x), rows, n, K, _ptr(hadK), ctypes.c_float(scale),
                                                 ctypes.c_float(sig[0] if sig is not None else 1.0),
                                                 ctypes.c_float(sig[1] if sig is not None else 1.0), _ptr(q), _ptr(s), _ptr(y), _stream(x)))
    return y, q, s


def hadamard_quantizer_mfma(x: torch.Tensor, K: int, hadK: torch.Tensor, input_clip_ratio: float = 1.0, scale: Optional[float] = None,
                            up: Optional[torch.Tensor] = None, want_y: bool = False):
    """fq_hadamard_quantizer_mfma_f16: the structured rotation (had_mfma_supported shapes) in front of deploy.nn.Quantizer(
    input_clip_ratio, lac=False) as ONE launch — scale = fp16(max|y| / 7) * ratio with no zero guard (deploy/nn/quantization.py:30), the
    down_proj input of the reference's ``options.trans == "had"`` model. -> (q [..., n/2] uint8, scales [rows] fp16, y or None).
    ``up``: x is x_gate, the rotation's input fp16(up * fp16(silu(x)))."""
    _chk(x, "x"), _chk(hadK, "hadK")
    n = x.shape[-1]
    if hadK.shape != (K, K) or not had_mfma_supported(n, K):
        raise ValueError("hadamard_quantizer_mfma: n = K * 512 (K <= 32) or K * 1024 (K <= 28), K % 4 == 0, hadK [K, K]")
    if up is not None:
        _chk(up, "up")
        if up.shape != x.shape or want_y:
            raise ValueError("hadamard_quantizer_mfma(up=...): up of x's shape, want_y=False")
    if scale is None:
        scale = float(1.0 / torch.tensor(n).sqrt())
    rows = x.numel() // n
    q = torch.empty(x.shape[:-1] + (n // 2,), dtype=torch.uint8, device=x.device)
    s = torch.empty((rows,), dtype=torch.float16, device=x.device)
    y = torch.empty_like(x) if want_y else None
    if rows > 0:
        with _on(x.device):
            check(lib.fq_hadamard_quantizer_mfma_f16(_ptr(x), _ptr(up), rows, n, K, _ptr(hadK), ctypes.c_float(scale),
                                                     ctypes.c_float(float(input_clip_ratio)), _ptr(q), _ptr(s), _ptr(y), _stream(x)))
    return q, s, y


def hadamard_quantizer(x: torch.Tensor, K: int, hadK: Optional[torch.Tensor], input_clip_ratio: float = 1.0,
                       up: Optional[torch.Tensor] = None):
    """The online Hadamard rotation in front of deploy.nn.Quantizer(input_clip_ratio, lac=False) as ONE launch where a fused route
    exists — the structured kernel (hadamard_quantizer_mfma: 14336, 28672, ...) or the tall Kronecker kernel with FQ_RATIO_POST
    (n = K' * 64 pairs: 11008 = 172 x 64, 8960, 5120 ...; ``up`` is multiplied in by its own launch there). -> (q, scales [rows])
    or None when the width has neither (the caller runs the rotation and the Quantizer one after the other)."""
    n = x.shape[-1]
    if K <= 1 or hadK is None or x.dtype != torch.float16 or not x.is_cuda or x.numel() == 0 or n % K:
        return None
    if had_mfma_supported(n, K):
        q, s, _ = hadamard_quantizer_mfma(x, K, hadK, input_clip_ratio, up=up)
        return q, s
    kr = _hadamard_as_kron(K, n // K, hadK, x.device)
    if kr is None or kr[2] != 64 or not 64 < kr[0].shape[0] <= 192:
        return None
    left, right, N = kr
    if up is not None:
        x = silu_mul(x, up)
    rows = x.numel() // n
    o = kron_quant_ex(x.reshape(rows, n), left, right, _had_right_div(N) * float(1.0 / torch.tensor(n).sqrt()),
                      [(float(input_clip_ratio), 1.0)], FQ_OUT_PACKED | FQ_QUANT_F16 | FQ_ROUND_Y_F16 | FQ_RATIO_POST)
    return o.q[0].reshape(x.shape[:-1] + (n // 2,)), o.scale[0].reshape(-1)


def hadamard(x: torch.Tensor, K: int = 1, hadK: Optional[torch.Tensor] = None,
             scale: Optional[float] = None, fwht_route: bool = False) -> torch.Tensor:
    """hadK @ FWHT(x.view(rows, K, n/K)) * scale. Routes: the register FWHT + K-factor kernel (fq_hadamard_f16; bit-exact for K = 1,
    the route of every K = 1 call); for K > 1 a matrix-pipe launch where one exists — the rotation as a dense Kronecker pair with the
    transform as its only output (11008 = 172 x 64, 8960, 5120), or the structured kernel (n = K * 512 / K * 1024: 14336, 28672). The
    matrix-pipe routes round the intermediate to fp16 at other points: within 1e-3 of the row maximum of the exact rotation, not
    bit-identical to the first route. ``fwht_route=True`` forces the first."""
    if K > 1 and hadK is not None and not fwht_route and x.numel() > 0 and x.shape[-1] % K == 0 and hadK.shape == (K, K):
        # (round 4) tall rotations — 11008 = 172 x 64 (Llama-2-7B), 8960 = 140 x 64, 5120 = 80 x 64 ... — as ONE dense Kronecker launch
        # with the transform as its only output (fq_kron_tall.hip: 464 -> ~200 us per 16384 tokens of 11008); tolerance parity
        # as the fused launch of the same pair (hadamard_quant), fwht_route=True keeps the bit-identical register FWHT
        # 14336 = 28 * 512: the structured matrix-pipe kernel (end to end through this function, 16384 tokens: 181 us against 244 for the
        # dense 112 x 128 pair with its post-scale and 238 for the FWHT route: profiles/r04_hadamard_standalone.txt, last block)
        if had_mfma_supported(x.shape[-1], K):
            return hadamard_mfma(x, K, hadK, None, scale, True)[0]
        kr = _hadamard_as_kron(K, x.shape[-1] // K, hadK, x.device)
        if kr is not None and kr[2] in (64, 128):
            _chk(x, "x"), _chk(hadK, "hadK")
            n = x.shape[-1]
            sc = float(1.0 / torch.tensor(n).sqrt()) if scale is None else scale
            o = kron_quant_ex(x.reshape(-1, n), kr[0], kr[1], _had_right_div(kr[2]) * sc, [(1.0, 1.0)], FQ_OUT_TRANSFORM | FQ_ROUND_Y_F16)
            return o.y.reshape(x.shape)
    _chk(x, "x")
    n = x.shape[-1]
    if K > 1:
        if hadK is None:
            raise ValueError("hadK required when K > 1")
        _chk(hadK, "hadK")
        if hadK.shape != (K, K):
            raise ValueError("hadK must be [K, K]")
    if scale is None:
        scale = float(1.0 / torch.tensor(n).sqrt())  # fp32 value, as hadamard_utils.py:135
    rows = x.numel() // n
    y = torch.empty_like(x)
    if rows == 0:
        return y
    with _on(x.device):
        check(lib.fq_hadamard_f16(_ptr(x), _ptr(y), rows, n, K, _ptr(hadK), ctypes.c_float(scale), _stream(x)))
    return y


def hadamard_fp32(x: torch.Tensor, K: int = 1, hadK: Optional[torch.Tensor] = None, scale: Optional[float] = None) -> torch.Tensor:
    """matmul_hadU_cuda on x.float() (OnlineTrans(force_fp32=True), deploy/nn/online_trans.py:55-59) -> fp32: the power-of-two
    transform with an fp32 result (fq_fwht_f32_f16: no fp16 rounding anywhere), then — K > 1 — the fp32 K x K factor as the
    reference's own plain GEMM (`hadK.to(input.dtype) @ input`, online_trans.py:148-150). x fp16 (its up-cast is exact)."""
    n = x.shape[-1]
    if n % K:
        raise ValueError("hadamard_fp32: n % K != 0")
    P = n // K
    if x.is_cuda and x.dtype == torch.bfloat16 and scale is None and 64 <= P <= 8192:
        return hadamard_wide(x.float(), K, hadK)            # (bf16 models: the up-cast is exact, the transform runs on fp16 pieces of it)
    _chk(x, "x")
    if P < 64 or P > 8192:
        # outside the fp32-result kernel's range (tiny test models: n / K = 32; n / K = 16384): the fp16-result kernel and an up-cast,
        # what this route was before round 4
        return hadamard(x, K, None if hadK is None else hadK.to(device=x.device, dtype=torch.float16).contiguous(), scale).float()
    if scale is None:
        scale = float(1.0 / torch.tensor(n).sqrt())
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    vecs = x.numel() // P
    if vecs:
        with _on(x.device):
            check(lib.fq_fwht_f32_f16(_ptr(x), _ptr(y), vecs, P, ctypes.c_float(scale), _stream(x)))
    if K == 1:
        return y
    if hadK is None or hadK.shape != (K, K):
        raise ValueError("hadK [K, K] required when K > 1")
    return (hadK.to(device=x.device, dtype=torch.float32) @ y.view(*x.shape[:-1], K, P)).reshape(x.shape)


def hadamard_wide(x: torch.Tensor, K: int = 1, hadK: Optional[torch.Tensor] = None) -> torch.Tensor:
    """matmul_hadU (hadamard_utils.py:89-110) for bf16 / fp32 ROCm tensors -> x's dtype, on the fp32-butterfly kernel
    (fq_fwht_f32_f16: fp16 in — exact up-cast — fp32 stages and result, nothing rounded in between). The transform is linear and
    power-of-two scaling is exact, so the input is handed over as fp16 PIECES of `x * 2^-e` (e: the tensor's largest exponent brought
    to 2^14): one piece for bf16 (8 mantissa bits fit fp16's 11 exactly), high + low for fp32 (22 of 24 mantissa bits; the residual is
    below 2^-22 of the largest element, inside the reference's own fp32 stage rounding ~log2(n) 2^-24). The K x K factor of
    n = K 2^p and the 1/sqrt(n) are the reference's own plain operations in fp32 (hadamard_utils.py:108-110). P = n / K in 64..8192."""
    if not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("hadamard_wide: bf16 / fp32 ROCm tensors")
    n = x.shape[-1]
    if n % K:
        raise ValueError("hadamard_wide: n % K != 0")
    P = n // K
    if P < 64 or P > 8192 or P & (P - 1):
        raise _lib.FqError(FQ_EUNSUPPORTED, f"hadamard_wide: n / K = {P} outside the register transform's range (64 .. 8192, a power of two)")
    xc = x.contiguous()
    amax = float(xc.abs().max()) if xc.numel() else 0.0
    if not math.isfinite(amax):
        raise ValueError("hadamard_wide: non-finite input")
    e = 0 if amax == 0.0 else math.frexp(amax)[1] - 15       # amax * 2^-e in [2^14, 2^15)
    xs = torch.ldexp(xc.float(), torch.tensor(-e, device=x.device))
    hi = xs.half()
    pieces = [hi] if x.dtype == torch.bfloat16 else [hi, (xs - hi.float()).half()]
    vecs = xc.numel() // P
    y = None
    for pc in pieces:
        yp = torch.empty(xc.shape, dtype=torch.float32, device=x.device)
        if vecs:
            with _on(x.device):
                check(lib.fq_fwht_f32_f16(_ptr(pc), _ptr(yp), vecs, P, ctypes.c_float(1.0), _stream(x)))
        y = yp if y is None else y + yp
    if K > 1:
        if hadK is None or hadK.shape != (K, K):
            raise ValueError("hadK [K, K] required when K > 1")
        y = (hadK.to(device=x.device, dtype=torch.float32) @ y.view(*xc.shape[:-1], K, P)).reshape(xc.shape)
    y = torch.ldexp(y, torch.tensor(e, device=x.device)) / torch.tensor(n, dtype=torch.float32, device=x.device).sqrt()
    return y.to(x.dtype)


def hadamard_quant(x: torch.Tensor, K: int = 1, hadK: Optional[torch.Tensor] = None, sig: Sig = (1.0, 1.0),
                   scale: Optional[float] = None, up: Optional[torch.Tensor] = None,
                   fwht_route: bool = False, route: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Hadamard rotation fused with the deploy Quantizer (fq_hadamard_quant_f16): -> (q uint8 [..., n/2], scales fp16
    [rows]); the Quantizer's arithmetic is deploy/nn/quantization.py:15-29. Two routes:
      * the register FWHT + K-factor kernel — bit-identical to rowquant(hadamard(x), [sig], FQ_OUT_PACKED | FQ_QUANT_F16 |
        FQ_SIG_F16); shapes the fused kernels do not cover take exactly that two-launch sequence;
      * n = K * 512 or K * 1024 with K <= 32 (14336 = 28 * 512, 28672 = 28 * 1024; round 4): the structured matrix-pipe kernel
        (hadamard_mfma) — H_512 / H_1024 as two register butterflies and two K = 32 contractions, 16 / 32 MFMAs per wave and token
        instead of the 60 / 128 of the dense pair below;
      * n = 11008 (K = 172) and every other n = K 2^p whose rotation is a factor pair with a
        packed-only kernel of its own (_hadamard_as_kron): the rotation runs as ONE Kronecker launch (112 x 128 / 112 x 256 /
        172 x 64, kron_quant_ex), 1.5-2x faster. It rounds the intermediate to fp16 at a different point: the rotated values agree with
        the FWHT route within 2e-3 of the row maximum (the reference's own tolerance class, tests/test_gpu_hadamard.py), so
        scales can differ by an fp16 step and digits by +-1 on ~1e-3 of elements — NOT bit for bit.
    ``fwht_route=True`` (= ``route="fwht"``) forces the first route for callers that need hadamard(fwht_route=True) + Quantizer ==
    hadamard_quant() exactly; ``route="kron"`` forces the dense Kronecker launch where it exists, ``route="mfma"`` the structured one.
    With ``up``: x is x_gate and the input of the rotation is up * silu(x), formed inside the launch (every route)."""
    if route not in (None, "fwht", "kron", "mfma"):
        raise ValueError("route: None, 'fwht', 'kron' or 'mfma'")
    fwht_route = fwht_route or route == "fwht"
    _chk(x, "x")
    if up is not None:
        _chk(up, "up")
        if up.shape != x.shape:
            raise ValueError("up must have x's shape")
    n = x.shape[-1]
    if K > 1:
        if hadK is None:
            raise ValueError("hadK required when K > 1")
        _chk(hadK, "hadK")
        if hadK.shape != (K, K):
            raise ValueError("hadK must be [K, K]")
    if scale is None:
        scale = float(1.0 / torch.tensor(n).sqrt())
    rows = x.numel() // n
    if route == "mfma" and not had_mfma_supported(n, K):
        raise _lib.FqError(FQ_EUNSUPPORTED, "hadamard_quant(route='mfma'): n = K * 512 (K <= 32) or K * 1024 (K <= 28), K % 4 == 0")
    if not fwht_route and route != "kron" and rows > 0 and had_mfma_supported(n, K):
        # the structured route (fq_had_mfma.hip): H_512 = H_4 (x) H_4 (x) H_32 (H_1024 = H_8 (x) H_4 (x) H_32) as two register butterflies +
        # two K = 32 contractions
        _, q, s = hadamard_mfma(x, K, hadK, sig, scale, want_y=False, up=up)
        return q, s
    kr = _hadamard_as_kron(K, n // K, hadK, x.device) if (n % K == 0 and not fwht_route) else None
    if kr is not None and rows > 0:
        # K > 1 shapes whose rotation is a Kronecker pair the fused MFMA kernels take (14336 = 112 x 128, 28672 = 112 x 256):
        # one launch of the transform + Quantizer kernel instead of the register FWHT + K-factor kernel (1.5x faster; the
        # two differ in where the intermediate is rounded to fp16, both within the 1e-3 tolerance of the reference)
        left, right, N = kr
        if up is not None and N == 64:     # the SiLU.mul input is fused for the down_proj pairs of N >= 128 only
            x, up = silu_mul(x, up), None
        o = kron_quant_ex(x.reshape(rows, n), left, right, _had_right_div(N) * scale, [sig],
                          FQ_OUT_PACKED | FQ_QUANT_F16 | FQ_SIG_F16 | FQ_ROUND_Y_F16,
                          up=None if up is None else up.reshape(rows, n))
        return o.q[0].reshape(x.shape[:-1] + (n // 2,)), o.scale[0]
    q = torch.empty(x.shape[:-1] + (n // 2,), dtype=torch.uint8, device=x.device)
    s = torch.empty((rows,), dtype=torch.float16, device=x.device)
    if rows == 0:
        return q, s
    with _on(x.device):
        if up is not None:
            rc = lib.fq_silu_mul_hadamard_quant_f16(_ptr(x), _ptr(up), rows, n, K, _ptr(hadK), ctypes.c_float(scale),
                                                    ctypes.c_float(sig[0]), ctypes.c_float(sig[1]), _ptr(q), _ptr(s),
                                                    _stream(x))
        else:
            rc = lib.fq_hadamard_quant_f16(_ptr(x), rows, n, K, _ptr(hadK), ctypes.c_float(scale), ctypes.c_float(sig[0]),
                                           ctypes.c_float(sig[1]), _ptr(q), _ptr(s), _stream(x))
    if rc == _lib.FQ_EUNSUPPORTED:
        if up is not None:
            x = silu_mul(x, up)
        o = rowquant(hadamard(x, K, hadK, scale, fwht_route=True), [sig], FQ_OUT_PACKED | FQ_QUANT_F16 | FQ_SIG_F16)
        return o.q[0], o.scale[0].reshape(-1)
    check(rc)
    return q, s


def int4_to_frag(w: torch.Tensor) -> torch.Tensor:
    """Linear4bit.weight [N, K/2] -> its image in MFMA fragment order for the decode-sized GEMM (fq_int4_to_frag)."""
    _chk(w, "w", torch.uint8)
    N, K = w.shape[0], w.shape[1] * 2
    nbytes = lib.fq_int4_frag_bytes(N, K)
    if nbytes < 0:
        raise _lib.FqError(_lib.FQ_EUNSUPPORTED, f"int4_to_frag: K={K} must be a multiple of 64")
    img = torch.empty((nbytes,), dtype=torch.uint8, device=w.device)
    with _on(w.device):
        check(lib.fq_int4_to_frag(_ptr(w), N, K, _ptr(img), _stream(w)))
    return img


SKINNY_K_LIMIT = 131072      # the weight-streaming kernel's accumulator carries 256 x the sum: all -8 x -8 would wrap at this K


def skinny_supported(M: int, K: int) -> bool:
    return 1 <= M <= 128 and K % 64 == 0 and K < SKINNY_K_LIMIT


def int4_skinny_matmul(x: torch.Tensor, w_image: torch.Tensor, N: int) -> torch.Tensor:
    """int4_matmul for M <= 128 rows against a weight image from int4_to_frag (fq_int4_skinny_gemm_i32)."""
    _chk(x, "x", torch.uint8)
    M, K = x.shape[0], x.shape[1] * 2
    c = torch.empty((M, N), dtype=torch.int32, device=x.device)
    if M:
        with _on(x.device):
            check(lib.fq_int4_skinny_gemm_i32(_ptr(x), _ptr(w_image), M, N, K, _ptr(c), _stream(x)))
    return c


_SKINNY_WS_BYTES: dict = {}      # (M tile count, N, K) -> fq_int4_skinny_split_workspace_bytes: a pure function


def skinny_split_workspace(M: int, N: int, K: int, device, stream=None):
    """-> (zeroed workspace | None, bytes) of the split weight-streaming launch for this geometry on the current stream (None: the geometry is
    not split, or the call is inside a stream capture that no eager call on this stream preceded — the plain launch runs then). The eager
    module path calls this too, so that a capture that follows its warm-up finds the workspace (deploy.nn.Linear4bit)."""
    key = ((M + 31) // 32, N, K)
    nbytes = _SKINNY_WS_BYTES.get(key)
    if nbytes is None:
        nbytes = _SKINNY_WS_BYTES[key] = int(lib.fq_int4_skinny_split_workspace_bytes(M, N, K))
    if nbytes <= 0:
        return None, 0
    if stream is None:
        stream = ctypes.c_void_p(_stream_handle(device))
    return _kv_split_workspace(("skinny", device.index, stream.value, nbytes), nbytes, device), nbytes


def int4_skinny_linear(x: torch.Tensor, x_scale: torch.Tensor, w_image: torch.Tensor, w_scale: torch.Tensor,
                       bias: Optional[torch.Tensor], N: int, split: bool = True) -> torch.Tensor:
    """int4_linear for M <= 128 rows against a weight image (fq_int4_skinny_linear_f16), bit-identical. ``split=False``: never the split launch."""
    _chk(x, "x", torch.uint8), _chk(x_scale, "x_scale"), _chk(w_scale, "w_scale")
    M, K = x.shape[0], x.shape[1] * 2
    if x_scale.numel() != M or w_scale.numel() != N:
        raise RuntimeError("int4_skinny_linear: x_scale must have M elements, w_scale N")
    if bias is not None:
        _chk(bias, "bias")
    y = torch.empty((M, N), dtype=torch.float16, device=x.device)
    if M:
        with _on(x.device):
            # (round 6) a lone narrow projection of 33 .. 128 rows: the K range of its feature tiles over 2 - 4 workgroups (fq_int4_skinny_linear_split_f16),
            # in a zeroed workspace kept per (device, stream, bytes) under the split-decode workspaces' protocol (never created inside a capture)
            stream = _stream(x)
            ws, nbytes = skinny_split_workspace(M, N, K, x.device, stream) if split else (None, 0)
            if ws is not None:
                check(lib.fq_int4_skinny_linear_split_f16(_ptr(x), _ptr(x_scale), _ptr(w_image), _ptr(w_scale), _ptr(bias), M, N, K,
                                                          _ptr(y), _ptr(ws), nbytes, stream))
            else:
                check(lib.fq_int4_skinny_linear_f16(_ptr(x), _ptr(x_scale), _ptr(w_image), _ptr(w_scale), _ptr(bias), M, N, K,
                                                    _ptr(y), stream))
    return y


def int4_skinny_linear_multi(problems) -> list:
    """Up to four decode-sized Linear4bit problems that share M (<= 128) and K — q / k / v, or up / gate of one layer — as ONE launch of the
    weight-streaming kernel (fq_int4_skinny_linear_multi_f16). ``problems``: a sequence of (x packed [M, K/2], x_scale [M], w_image
    (int4_to_frag), w_scale [N], bias [N] or None) -> a list of fp16 [M, N] tensors, each bit-identical to int4_skinny_linear()."""
    n = len(problems)
    if not 1 <= n <= 4:
        raise ValueError("int4_skinny_linear_multi: 1..4 problems")
    x0 = problems[0][0]
    M, K = x0.shape[0], x0.shape[1] * 2
    Ns = []
    for x, xs, wimg, ws, b in problems:
        _chk(x, "x", torch.uint8), _chk(xs, "x_scale"), _chk(ws, "w_scale")
        if b is not None:
            _chk(b, "bias")
        if x.dim() != 2 or x.shape != x0.shape:
            raise RuntimeError("int4_skinny_linear_multi: the problems must share M and K (x [M, K/2])")
        N = ws.numel()
        if xs.numel() != M or (b is not None and b.numel() != N) or wimg.numel() != int(lib.fq_int4_frag_bytes(N, K)):
            raise RuntimeError("int4_skinny_linear_multi: scale / bias / image sizes do not match M / N / K")
        Ns.append(N)
    ys = [torch.empty((M, N), dtype=torch.float16, device=x0.device) for N in Ns]
    if M == 0:
        return ys
    VP = ctypes.c_void_p * n
    tab = lambda k: VP(*[None if pr[k] is None else pr[k].data_ptr() for pr in problems])
    with _on(x0.device):
        check(lib.fq_int4_skinny_linear_multi_f16(n, tab(0), tab(1), tab(2), tab(3), tab(4), M, (ctypes.c_int * n)(*Ns), K,
                                                  VP(*[y.data_ptr() for y in ys]), _stream(x0)))
    return ys


FUSED_DECODE_MAX_ROWS = 16


def kron64_linear_multi(x: torch.Tensor, left: torch.Tensor, right: torch.Tensor, sigs: Sequence[Sig], problems, eps: Optional[float] = None,
                        flags: int = 0) -> Optional[list]:
    """The transform as the GEMM's prologue, decode regime (fq_kron64_linear_multi_f16): [RMSNorm(eps) +] the 64 x 64 Kronecker transform +
    per-token INT4 quantisation of x [..., 4096] (<= 16 tokens) + up to four Linear4bit problems — ``problems``: (w_image (int4_to_frag),
    w_scale [N], bias [N] or None), problem p quantised with sigs[p] — as ONE launch. -> a list of fp16 [M, N] tensors, bit-identical to
    [rmsnorm_]kron_quant(..., sigs, FQ_OUT_PACKED | flags) followed by int4_skinny_linear_multi; None when the shape is not covered
    (more than 16 tokens, a pair other than 64 x 64, N % 32 != 0): the caller runs the two launches."""
    n = len(problems)
    if not 1 <= n <= 4 or len(sigs) != n:
        raise ValueError("kron64_linear_multi: 1..4 problems, one clip pair each")
    if left.shape != (64, 64) or right.shape != (64, 64) or x.shape[-1] != 4096 or x.dtype != torch.float16:
        return None
    M = x.numel() // 4096
    Ns = [pr[1].numel() for pr in problems]
    if M > FUSED_DECODE_MAX_ROWS or any(N % 32 for N in Ns):
        return None
    _chk(x, "x"), _chk(left, "left"), _chk(right, "right")
    for (wimg, ws, b), N in zip(problems, Ns):
        _chk(ws, "w_scale")
        if b is not None:
            _chk(b, "bias")
        if (b is not None and b.numel() != N) or wimg.numel() != int(lib.fq_int4_frag_bytes(N, 4096)):
            raise RuntimeError("kron64_linear_multi: bias / image sizes do not match N / K")
    ys = [torch.empty((M, N), dtype=torch.float16, device=x.device) for N in Ns]
    if M == 0:
        return ys
    smax, smin, _ = _sig_arrays(sigs)
    VP = ctypes.c_void_p * n
    tab = lambda k: VP(*[None if pr[k] is None else pr[k].data_ptr() for pr in problems])
    with _on(x.device):
        ws, ws_bytes, prepared, key = _kron_workspace(x.device, 64, 64, left, right)
        check(lib.fq_kron64_linear_multi_f16(_ptr(x), 0 if eps is None else 1, ctypes.c_float(0.0 if eps is None else eps), _ptr(left),
                                             _ptr(right), M, n, smax, smin, flags | (FQ_WS_PREPARED if prepared else 0), tab(0), tab(1),
                                             tab(2), (ctypes.c_int * n)(*Ns), VP(*[y.data_ptr() for y in ys]), _ptr(ws), ws_bytes,
                                             _stream(x)))
        if key is not None and not prepared:
            _kron_workspace_commit(key, ws, left, right)
    return ys


def block_linear_supported(M: int, R: int, C: int, N: int) -> bool:
    """Does the fused o_proj launch (fq_block_linear_f16) cover M tokens of [R, C] blocks in front of an N-feature Linear4bit?
    R = head_dim = 128 and C = heads = 32 (hidden size 4096), 1..16 tokens, N a multiple of 32."""
    return R == 128 and C == 32 and 1 <= M <= FUSED_DECODE_MAX_ROWS and N >= 32 and N % 32 == 0


def block_linear(x: torch.Tensor, P: torch.Tensor, sig: Sig, w_image: torch.Tensor, w_scale: torch.Tensor, bias: Optional[torch.Tensor],
                 N: int, flags: int = FQ_NO_CLAMP0) -> Optional[torch.Tensor]:
    """The head transform as the GEMM's prologue, decode regime (fq_block_linear_f16): x [..., R, C] @ P [C, C], the per-token INT4 quantiser
    of the transposed block with the clip pair ``sig``, and the Linear4bit (w_image of int4_to_frag, w_scale [N], bias [N] or None) as ONE
    launch -> fp16 [M, N], bit-identical to block_quant(x, P, [sig], FQ_OUT_PACKED | flags, transpose_out=True) followed by
    int4_skinny_linear. None when the shape is not covered (block_linear_supported): the caller runs the two launches."""
    if x.dim() < 2 or x.dtype != torch.float16:
        return None
    R, C = x.shape[-2], x.shape[-1]
    M = x.numel() // (R * C) if R * C else 0
    if not block_linear_supported(M, R, C, N):
        return None
    _chk(x, "x"), _chk(P, "P"), _chk(w_scale, "w_scale"), _chk(w_image, "w_image", torch.uint8)
    if bias is not None:
        _chk(bias, "bias")
    if P.shape != (C, C):
        raise ValueError("P must be [C, C] with C = x.shape[-1]")
    if w_scale.numel() != N or (bias is not None and bias.numel() != N) or w_image.numel() != int(lib.fq_int4_frag_bytes(N, R * C)):
        raise RuntimeError("block_linear: scale / bias / image sizes do not match N / K")
    y = torch.empty((M, N), dtype=torch.float16, device=x.device)
    with _on(x.device):
        check(lib.fq_block_linear_f16(_ptr(x), _ptr(P), M, R, C, ctypes.c_float(sig[0]), ctypes.c_float(sig[1]), flags, _ptr(w_image),
                                      _ptr(w_scale), _ptr(bias), N, _ptr(y), _stream(x)))
    return y


def int4_to_bf6(q: torch.Tensor, weights: bool = False) -> torch.Tensor:
    """Packed INT4 [rows, K/2] -> the BF6 operand image of the FP6-path GEMM (fq_int4_to_bf6). ``weights``: the image of
    a Linear4bit.weight (convert once per layer); else of packed activations. K % 64 == 0."""
    _chk(q, "q", torch.uint8)
    if q.dim() != 2:
        raise RuntimeError("int4_to_bf6: expected [rows, K/2]")
    rows, K = q.shape[0], q.shape[1] * 2
    nbytes = lib.fq_bf6_blob_bytes(rows, K)
    if nbytes < 0:
        raise _lib.FqError(_lib.FQ_EUNSUPPORTED, f"int4_to_bf6: K={K} must be a multiple of 64")
    blob = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
    if rows:
        with _on(q.device):
            check(lib.fq_int4_to_bf6(_ptr(q), rows, K, 1 if weights else 0, _ptr(blob), _stream(q)))
    return blob


def bf6_supported(N: int, K: int) -> bool:
    return K % 128 == 0 and N % 16 == 0 and K <= (1 << 18)


def bf6_matmul(xblob: torch.Tensor, wblob: torch.Tensor, M: int, N: int, K: int) -> torch.Tensor:
    """int4_matmul on the FP6 matrix path: blobs from int4_to_bf6 -> int32 [M, N], bit-identical."""
    c = torch.empty((M, N), dtype=torch.int32, device=xblob.device)
    if M:
        with _on(xblob.device):
            check(lib.fq_bf6_gemm_i32(_ptr(xblob), _ptr(wblob), M, N, K, _ptr(c), _stream(xblob)))
    return c


def bf6_linear(xblob: torch.Tensor, x_scale: torch.Tensor, wblob: torch.Tensor, w_scale: torch.Tensor,
               bias: Optional[torch.Tensor], M: int, N: int, K: int) -> torch.Tensor:
    """int4_linear on the FP6 matrix path (fq_bf6_linear_f16), bit-identical."""
    _chk(x_scale, "x_scale"), _chk(w_scale, "w_scale")
    if x_scale.numel() != M or w_scale.numel() != N:
        raise RuntimeError("bf6_linear: x_scale must have M elements, w_scale N")
    if bias is not None:
        _chk(bias, "bias")
    y = torch.empty((M, N), dtype=torch.float16, device=xblob.device)
    if M:
        with _on(xblob.device):
            check(lib.fq_bf6_linear_f16(_ptr(xblob), _ptr(x_scale), _ptr(wblob), _ptr(w_scale), _ptr(bias), M, N, K, _ptr(y),
                                        _stream(xblob)))
    return y


def int4_linear_fp6(x: torch.Tensor, x_scale: torch.Tensor, w: torch.Tensor, w_image: Optional[torch.Tensor], w_scale: torch.Tensor,
                    bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Linear4bit.forward on the FP6 path as one library call (fq_int4_linear_fp6_f16): packed x [M, K/2], packed w [N, K/2] and,
    if the layer keeps one, its FP6 image (else the weights are converted for the call into the same scratch block as the
    activations) -> fp16 [M, N], the bits of int4_linear. One scratch allocation, one ctypes call, three launches."""
    _chk(x, "x", torch.uint8), _chk(w, "w", torch.uint8), _chk(x_scale, "x_scale"), _chk(w_scale, "w_scale")
    if bias is not None:
        _chk(bias, "bias")
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise RuntimeError(f"int4_linear_fp6: expected x [M, K/2] and w [N, K/2], got {tuple(x.shape)} and {tuple(w.shape)}")
    M, N, K = x.shape[0], w.shape[0], x.shape[1] * 2
    if x_scale.numel() != M or w_scale.numel() != N or (bias is not None and bias.numel() != N):
        raise RuntimeError("int4_linear_fp6: scale / bias sizes do not match M / N")
    if not bf6_supported(N, K):
        raise _lib.FqError(_lib.FQ_EUNSUPPORTED, f"int4_linear_fp6: N={N} K={K} not covered (K % 128, N % 16)")
    y = torch.empty((M, N), dtype=torch.float16, device=x.device)
    if M == 0:
        return y
    nbytes = int(lib.fq_bf6_blob_bytes(M, K)) + (0 if w_image is not None else int(lib.fq_bf6_blob_bytes(N, K)))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    with _on(x.device):
        check(lib.fq_int4_linear_fp6_f16(_ptr(x), _ptr(x_scale), _ptr(w), _ptr(w_image), _ptr(w_scale), _ptr(bias), M, N, K, _ptr(y),
                                         _ptr(scratch), nbytes, _stream(x)))
    return y


def int4_linear_fp6_multi(problems) -> list:
    """Up to four Linear4bit problems that share M and K (q / k / v, or up / gate of one layer) as ONE GEMM launch
    (fq_int4_linear_fp6_multi_f16). ``problems``: a sequence of (x packed [M, K/2], x_scale [M], w packed [N, K/2], w_image or None,
    w_scale [N], bias [N] or None) -> a list of fp16 [M, N] tensors, each bit-identical to int4_linear_fp6() of its problem."""
    n = len(problems)
    if not 1 <= n <= 4:
        raise ValueError("int4_linear_fp6_multi: 1..4 problems")
    x0 = problems[0][0]
    M, K = x0.shape[0], x0.shape[1] * 2
    Ns, nbytes, seen = [], 0, []
    for x, xs, w, wimg, ws, b in problems:
        _chk(x, "x", torch.uint8), _chk(w, "w", torch.uint8), _chk(xs, "x_scale"), _chk(ws, "w_scale")
        if b is not None:
            _chk(b, "bias")
        if x.dim() != 2 or w.dim() != 2 or x.shape != x0.shape or w.shape[1] != x.shape[1]:
            raise RuntimeError("int4_linear_fp6_multi: the problems must share M and K (x [M, K/2], w [N, K/2])")
        N = w.shape[0]
        if xs.numel() != M or ws.numel() != N or (b is not None and b.numel() != N):
            raise RuntimeError("int4_linear_fp6_multi: scale / bias sizes do not match M / N")
        if not bf6_supported(N, K):
            raise _lib.FqError(_lib.FQ_EUNSUPPORTED, f"int4_linear_fp6_multi: N={N} K={K} not covered (K % 128, N % 16)")
        Ns.append(N)
        if x.data_ptr() not in seen:
            seen.append(x.data_ptr())
            nbytes += int(lib.fq_bf6_blob_bytes(M, K))
        if wimg is None:
            nbytes += int(lib.fq_bf6_blob_bytes(N, K))
    ys = [torch.empty((M, N), dtype=torch.float16, device=x0.device) for N in Ns]
    if M == 0:
        return ys
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=x0.device)
    VP = ctypes.c_void_p * n
    tab = lambda k: VP(*[None if pr[k] is None else pr[k].data_ptr() for pr in problems])
    with _on(x0.device):
        check(lib.fq_int4_linear_fp6_multi_f16(n, tab(0), tab(1), tab(2), tab(3), tab(4), tab(5), M, (ctypes.c_int * n)(*Ns), K,
                                               VP(*[y.data_ptr() for y in ys]), _ptr(scratch), nbytes, _stream(x0)))
    return ys


def kv_quant(x: torch.Tensor, trans: Optional[torch.Tensor] = None, clip: Sig = (1.0, 1.0), lac: bool = False,
             return_transformed: bool = False):
    """K/V cache quantisation (fq_kv_quant_f16): x [..., head_dim] fp16 -> (q uint8 [..., head_dim/2], param fp16
    [..., 2] = (scale, zero)[, y fp16 [..., head_dim]]). ``trans`` [head_dim, head_dim]: y = x @ trans first (the K
    transform). ``clip`` = the sigmoid-ed clip factors, used with ``lac`` only (kv_cache.py:11-51)."""
    _chk(x, "x")
    hd = x.shape[-1]
    if trans is not None:
        _chk(trans, "trans")
        if trans.shape != (hd, hd):
            raise ValueError("trans must be [head_dim, head_dim]")
    elif return_transformed:
        raise ValueError("return_transformed needs trans")
    rows = x.numel() // hd
    q = torch.empty(x.shape[:-1] + (hd // 2,), dtype=torch.uint8, device=x.device)
    param = torch.empty(x.shape[:-1] + (2,), dtype=torch.float16, device=x.device)
    y = torch.empty_like(x) if return_transformed else None
    if rows == 0:
        return (q, param, y) if return_transformed else (q, param)
    with _on(x.device):
        check(lib.fq_kv_quant_f16(_ptr(x), _ptr(trans), rows, hd, ctypes.c_float(clip[0]), ctypes.c_float(clip[1]),
                                  _lib.FQ_KV_LAC if lac else 0, _ptr(q), _ptr(param), _ptr(y), _stream(x)))
    return (q, param, y) if return_transformed else (q, param)


def kv_dequant(q: torch.Tensor, param: torch.Tensor, lac: bool = False) -> torch.Tensor:
    """unpack_i4_and_asym_dequantize (kv_cache.py:54-61): q uint8 [..., hd/2], param fp16 [..., 2] -> fp16 [..., hd]."""
    _chk(q, "q", torch.uint8), _chk(param, "param")
    hd = q.shape[-1] * 2
    rows = q.numel() // q.shape[-1]
    if param.numel() != rows * 2:
        raise ValueError("param must be [..., 2] with q's leading shape")
    y = torch.empty(q.shape[:-1] + (hd,), dtype=torch.float16, device=q.device)
    with _on(q.device):
        check(lib.fq_kv_dequant_f16(_ptr(q), _ptr(param), rows, hd, _lib.FQ_KV_LAC if lac else 0, _ptr(y), _stream(q)))
    return y


def _chk_kv_index(kv_indptr: torch.Tensor, kv_indices: torch.Tensor, last_page_offset: torch.Tensor) -> int:
    """The paged-cache index tensors as the kernels read them: int32, contiguous, on the device; kv_indptr has batch + 1
    entries (torch's default int64, or the reference's stride-0 expanded last_page_offset, would be read as garbage)."""
    for t, n in ((kv_indptr, "kv_indptr"), (kv_indices, "kv_indices"), (last_page_offset, "last_page_offset")):
        _chk(t, n, torch.int32)
    batch = last_page_offset.numel()
    if kv_indptr.numel() != batch + 1:
        raise ValueError(f"kv_indptr must have batch + 1 = {batch + 1} entries, got {kv_indptr.numel()}")
    return batch


def _kv_geometry(kv_data: torch.Tensor):
    """-> (layers, heads, page_size, head_dim) of a paged cache: uint8 pages hold head_dim / 2 bytes per row (INT4), float16
    pages head_dim values (the ``disable_quant`` configuration, kv_cache.py:177-190)."""
    pages, n_layers, two, heads, page_size, last = kv_data.shape
    if two != 2 or kv_data.dtype not in (torch.uint8, torch.float16):
        raise ValueError("kv_data must be [pages, layers, 2, heads, page_size, head_dim/2] uint8 or [..., head_dim] float16")
    return n_layers, heads, page_size, last * 2 if kv_data.dtype == torch.uint8 else last


def kv_append(kv_data: torch.Tensor, kv_param: torch.Tensor, kv_indptr: torch.Tensor, kv_indices: torch.Tensor,
              last_page_offset: torch.Tensor, k: torch.Tensor, v: torch.Tensor, k_param: torch.Tensor, v_param: torch.Tensor,
              layer_idx: int, seqlen_indptr: Optional[torch.Tensor] = None, group_size: int = 1) -> None:
    """init_kv_i4 (with ``seqlen_indptr``) / append_kv_i4 (without) of deploy/transformers/kv_cache.py:69-95: scatter
    packed keys / values [tokens, heads, head_dim/2] uint8 and their (scale, zero) [tokens, heads, 2] fp16 into the paged
    cache (fq_kv_append_i4). The index tensors are int32 on the cache's device. ``group_size`` g: k / v hold heads / g
    heads and every cache head h receives head h // g (the GQA repeat of kv_cache.py:286-296, done by the scatter)."""
    f16c = kv_data.dtype == torch.float16            # init_kv_f16 / append_kv_f16 (kv_cache.py:107-129): fp16 rows
    _chk(kv_data, "kv_data", kv_data.dtype), _chk(kv_param, "kv_param"), _chk(k, "k", kv_data.dtype), _chk(v, "v", kv_data.dtype)
    _chk(k_param, "k_param"), _chk(v_param, "v_param")
    batch = _chk_kv_index(kv_indptr, kv_indices, last_page_offset)
    if seqlen_indptr is not None:
        _chk(seqlen_indptr, "seqlen_indptr", torch.int32)
    n_layers, heads, page_size, hd = _kv_geometry(kv_data)
    src_heads = heads // group_size
    tokens = k.numel() // (src_heads * (hd if f16c else hd // 2))
    if k.shape != v.shape or k_param.numel() != tokens * src_heads * 2 or v_param.numel() != tokens * src_heads * 2:
        raise ValueError("k / v / k_param / v_param shapes do not agree")
    with _on(kv_data.device):
        check((lib.fq_kv_append_f16 if f16c else lib.fq_kv_append_i4)(_ptr(kv_data), _ptr(kv_param), _ptr(kv_indptr), _ptr(kv_indices), _ptr(last_page_offset),
            _ptr(k), _ptr(v), _ptr(k_param), _ptr(v_param), _ptr(seqlen_indptr), tokens, n_layers,
            layer_idx, heads, page_size, hd, batch, group_size, _stream(kv_data)))


def kv_quant_append(k: torch.Tensor, v: torch.Tensor, trans: Optional[torch.Tensor], kv_data: torch.Tensor,
                    kv_param: torch.Tensor, kv_indptr: torch.Tensor, kv_indices: torch.Tensor, last_page_offset: torch.Tensor,
                    layer_idx: int, group_size: int = 1, clip=None, lac: bool = False) -> None:
    """kv_quant(k, trans) + kv_quant(v) + kv_append in ONE launch (fq_kv_quant_append_i4): k, v [bsz, added, kv_heads,
    head_dim] fp16, every request appends ``added`` tokens at the end of its current length."""
    _chk(k, "k"), _chk(v, "v"), _chk(kv_data, "kv_data", torch.uint8), _chk(kv_param, "kv_param")
    if trans is not None:
        _chk(trans, "trans")
    n_layers, heads, page_size, hd = _kv_geometry(kv_data)
    batch = _chk_kv_index(kv_indptr, kv_indices, last_page_offset)
    if k.shape != v.shape or k.shape[-1] != hd or k.shape[0] != batch:
        raise ValueError("k / v must be [batch, added, kv_heads, head_dim]")
    src_heads = k.shape[-2]
    tokens = k.numel() // (src_heads * hd)
    if tokens == 0:
        return
    c4 = None if clip is None else (ctypes.c_float * 4)(*[float(t) for t in clip])
    with _on(k.device):
        check(lib.fq_kv_quant_append_i4(_ptr(k), _ptr(v), _ptr(trans), tokens, src_heads, hd, c4, _lib.FQ_KV_LAC if lac else 0,
                                        _ptr(kv_data), _ptr(kv_param), _ptr(kv_indptr), _ptr(kv_indices),
                                        _ptr(last_page_offset), n_layers, layer_idx, heads, page_size, batch, group_size,
                                        _stream(k)))


# Workspaces of the split decode launches: (device index, stream handle, pairs, head_dim) -> a buffer ZEROED EAGERLY once (the launches leave its
# counters as they found them), used by one launch at a time in stream order. ADVICE r05: never created inside a stream capture — a torch.zeros
# there is a memset NODE of that graph in that graph's private pool: a second graph captured on the same stream would find the cached buffer, record
# no memset, and replayed first would read garbage counters. A capture that finds no workspace runs the unsplit launch (same results up to
# the order of fp32 additions); warm the shape up eagerly on the capture stream first (tools/bench_decode.py does; torch.cuda.graph's own
# warm-up convention). An entry a capture HAS used is pinned (the graph replays its address); the others are bounded, least recently used first.
_KV_SPLIT_WS: "collections.OrderedDict" = CACHES.register("kv_split_workspaces", collections.OrderedDict())
_KV_SPLIT_WS_PINNED: dict = CACHES.register("kv_split_workspaces_pinned", {}, pinned=True)
_KV_SPLIT_WS_MAX = 16


def _kv_split_workspace(key, nbytes: int, device) -> Optional[torch.Tensor]:
    capturing = torch.cuda.is_current_stream_capturing()
    ws = _KV_SPLIT_WS_PINNED.get(key)
    if ws is not None:
        return ws
    ws = _KV_SPLIT_WS.get(key)
    if ws is None:
        if capturing:
            return None
        ws = torch.zeros((nbytes,), dtype=torch.uint8, device=device)
        _KV_SPLIT_WS[key] = ws
        while len(_KV_SPLIT_WS) > _KV_SPLIT_WS_MAX:
            _KV_SPLIT_WS.popitem(last=False)
    else:
        _KV_SPLIT_WS.move_to_end(key)
    if capturing:
        _KV_SPLIT_WS_PINNED[key] = _KV_SPLIT_WS.pop(key)
    return ws


def _kv_attn_front(q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, q_trans, transpose_out, tokens_dim: bool, kv_copies: int = 1,
                   append: bool = False, k_new=None, v_new=None):
    """What the attention wrappers over the paged cache do before they launch: the tensor checks, the cache geometry, the index tensors, q's
    shape ([batch, heads, head_dim]; with ``tokens_dim`` [batch, q_len, heads, head_dim]), the ``kv_copies`` and ``q_trans`` rules and the
    output (q's shape, its last two dimensions swapped with ``transpose_out``). ``append``: ``k_new`` / ``v_new`` are the new row of
    kv_decode_append (INT4 pages only), checked along.
    -> (o, q's device, layers, cache heads, page_size, head_dim, batch, query heads, q_group = query heads per cache head, share = query
    heads that read one set of rows, 1 if the pages are fp16, the five cache pointers as the entry points take them).
    Every tensor attribute is read once: these wrappers are the host side of a 15 us call."""
    _chk(q, "q")
    cache_dtype = kv_data.dtype
    if append:
        _chk(k_new, "k_new"), _chk(v_new, "v_new"), _chk(kv_data, "kv_data", torch.uint8)
    else:
        _chk(kv_data, "kv_data", cache_dtype)
    _chk(kv_param, "kv_param")
    n_layers, kv_heads, page_size, hd = _kv_geometry(kv_data)
    batch = _chk_kv_index(kv_indptr, kv_indices, last_page_offset)
    shape = q.shape
    if tokens_dim:
        if len(shape) != 4 or shape[0] != batch or shape[3] != hd or shape[1] < 1 or shape[2] % kv_heads:
            raise ValueError(f"q must be [{batch}, q_len >= 1, a multiple of {kv_heads}, {hd}]")
    elif len(shape) != 3 or shape[0] != batch or shape[2] != hd or shape[1] % kv_heads:
        # (round 6) a cache that holds the KV heads once: q carries q_group query heads per cache head (fq_kv_batch_decode_gqa)
        raise ValueError(f"q must be [{batch}, a multiple of {kv_heads}, {hd}]")
    if append and (k_new.shape != v_new.shape or k_new.dim() != 3 or k_new.shape[0] != batch or k_new.shape[2] != hd
                   or kv_heads % k_new.shape[1]):
        raise ValueError(f"k_new / v_new must be [{batch}, a divisor of {kv_heads}, {hd}]")
    heads = shape[-2]
    q_group = heads // kv_heads
    if kv_copies > 1 and (q_group != 1 or kv_heads % kv_copies or kv_copies > 8):
        raise ValueError(f"kv_copies={kv_copies}: needs a replicated cache (query heads == cache heads == {kv_heads}) in groups of at most 8")
    if q_trans is not None:
        _chk(q_trans, "q_trans")
        if q_trans.shape != (hd, hd):
            raise ValueError("q_trans must be [head_dim, head_dim]")
    dev = q.device
    o = torch.empty(shape[:-2] + (hd, heads) if transpose_out else shape, dtype=torch.float16, device=dev)
    return (o, dev, n_layers, kv_heads, page_size, hd, batch, heads, q_group, kv_copies if kv_copies > 1 else q_group,
            1 if cache_dtype == torch.float16 else 0,
            (kv_data.data_ptr(), kv_param.data_ptr(), kv_indptr.data_ptr(), kv_indices.data_ptr(), last_page_offset.data_ptr()))


def kv_batch_decode(q: torch.Tensor, kv_data: torch.Tensor, kv_param: torch.Tensor, kv_indptr: torch.Tensor,
                    kv_indices: torch.Tensor, last_page_offset: torch.Tensor, layer_idx: int,
                    q_trans: Optional[torch.Tensor] = None, transpose_out: bool = False, seq_hint: int = 0, split: bool = True,
                    kv_copies: int = 1) -> torch.Tensor:
    """batch_decode_i4 (kv_cache.py:98-105): q [batch, heads, head_dim] fp16 -> o of the same shape, attention over each
    request's cached rows (fq_kv_batch_decode_i4[_ex]). ``q_trans`` [head_dim, head_dim]: the query is multiplied by it
    inside the launch; ``transpose_out``: o comes back as [batch, head_dim, heads]. With at most 128 (request, head) pairs the rows
    of a request are split over several workgroups (fq_kv_batch_decode_split, round 5; ``seq_hint``: the longest request, 0 = unknown;
    ``split=False``: never) — same results up to the order of fp32 additions. ``kv_copies`` = g > 1 (round 6): the cache is the reference's
    REPLICATED layout whose g consecutive heads per KV head hold identical rows (kv_cache.py:286-296; the appends of this package write them so)
    and the launch reads one copy per group (fq_kv_batch_decode_copies): the same values from 1 / g of the bytes (the same output bit for bit
    below 32 (request, KV head) pairs; from there one workgroup serves a group: another order of the fp32 additions, as with split launches)."""
    o, dev, n_layers, kv_heads, page_size, hd, batch, heads, q_group, share, f16_cache, cache = _kv_attn_front(
        q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, q_trans, transpose_out, False, kv_copies)
    if batch == 0:
        return o
    with _on(dev):
        if not split:
            nbytes = 0
        elif share > 1:
            nbytes = int(lib.fq_kv_decode_workspace_bytes_gqa(batch, heads // share, share, hd))
        else:
            nbytes = int(lib.fq_kv_decode_workspace_bytes(batch, heads, hd))
        stream = ctypes.c_void_p(_stream_handle(dev))
        ws = _kv_split_workspace((dev.index, stream.value, batch * heads, hd), nbytes, dev) if nbytes > 0 else None
        tail = (int(seq_hint), _ptr(ws), nbytes if ws is not None else 0, stream)
        if kv_copies > 1:
            entry, lead, group = lib.fq_kv_batch_decode_copies, (f16_cache,), (heads, kv_copies)
        elif q_group > 1:
            entry, lead, group = lib.fq_kv_batch_decode_gqa, (f16_cache,), (kv_heads, q_group)
        elif ws is not None:
            entry, lead, group = lib.fq_kv_batch_decode_split, (f16_cache,), (heads,)
        else:
            entry, lead, group, tail = lib.fq_kv_batch_decode_f16_ex if f16_cache else lib.fq_kv_batch_decode_i4_ex, (), (heads,), (stream,)
        check(entry(*lead, o.data_ptr(), q.data_ptr(), _ptr(q_trans), 1 if transpose_out else 0, *cache, n_layers, layer_idx, *group, page_size, hd,
                    batch, *tail))
    return o


def kv_batch_extend(q: torch.Tensor, kv_data: torch.Tensor, kv_param: torch.Tensor, kv_indptr: torch.Tensor,
                    kv_indices: torch.Tensor, last_page_offset: torch.Tensor, layer_idx: int,
                    q_trans: Optional[torch.Tensor] = None, transpose_out: bool = False, seq_hint: int = 0, split: bool = True,
                    kv_copies: int = 1) -> torch.Tensor:
    """Causal attention of the T tokens a step appended to every request (fq_kv_batch_extend, round 7): q [batch, T, heads, head_dim]
    fp16 -> o of the same shape ([batch, T, head_dim, heads] with ``transpose_out``). The lengths already count the T new rows; token t
    attends rows 0 .. length - T + t. Heads, ``q_trans``, ``seq_hint``, ``split`` and ``kv_copies`` as kv_batch_decode: heads = cache heads
    x q_group (a cache that holds the KV heads once) or, with ``kv_copies`` = g > 1, the replicated layout read one copy per group.
    head_dim 128."""
    o, dev, n_layers, kv_heads, page_size, hd, batch, heads, _, share, f16_cache, cache = _kv_attn_front(
        q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, q_trans, transpose_out, True, kv_copies)
    q_len = q.shape[1]
    if batch == 0:
        return o
    with _on(dev):
        nbytes = int(lib.fq_kv_extend_workspace_bytes(batch, heads, q_len, hd)) if split else 0
        stream = ctypes.c_void_p(_stream_handle(dev))
        ws = _kv_split_workspace(("extend", dev.index, stream.value, batch, heads, q_len, hd), nbytes, dev) if nbytes > 0 else None
        check(lib.fq_kv_batch_extend(f16_cache, o.data_ptr(), q.data_ptr(), _ptr(q_trans), 1 if transpose_out else 0, *cache, n_layers, layer_idx,
                                     kv_heads, share, kv_copies, q_len, page_size, hd, batch, int(seq_hint), _ptr(ws),
                                     nbytes if ws is not None else 0, stream))
    return o


def kv_chunk_extend(q: torch.Tensor, kv_data: torch.Tensor, kv_param: torch.Tensor, kv_indptr: torch.Tensor,
                    kv_indices: torch.Tensor, last_page_offset: torch.Tensor, layer_idx: int,
                    q_trans: Optional[torch.Tensor] = None, transpose_out: bool = False, kv_copies: int = 1) -> torch.Tensor:
    """kv_batch_extend's attention for prompt-sized steps (fq_kv_chunk_extend): the same tensors, lengths, causal mask, heads, ``q_trans``,
    ``transpose_out`` and ``kv_copies``, computed by a launch in the prompt attention's shape — a workgroup per (request, set of cached rows,
    128 (token, head) rows of q), every 64-row tile of the cache unpacked once for all of them. No workspace and no split: two calls are
    bit-identical, and a step fed as two consecutive calls equals the one call bit for bit. head_dim 128; 1, 2, 4 or 8 query heads per set of
    cached rows (anything else: FqError, kv_batch_extend takes it)."""
    o, dev, n_layers, kv_heads, page_size, hd, batch, _, _, share, f16_cache, cache = _kv_attn_front(
        q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, q_trans, transpose_out, True, kv_copies)
    if batch == 0:
        return o
    with _on(dev):
        check(lib.fq_kv_chunk_extend(f16_cache, o.data_ptr(), q.data_ptr(), _ptr(q_trans), 1 if transpose_out else 0, *cache, n_layers, layer_idx,
                                     kv_heads, share, kv_copies, q.shape[1], page_size, hd, batch, ctypes.c_void_p(_stream_handle(dev))))
    return o


def kv_chunk_extend_supported(q_group: int, head_dim: int) -> bool:
    """Does fq_kv_chunk_extend take ``q_group`` query heads per set of cached rows at this head_dim? (What the cache class asks before it routes.)"""
    return head_dim == 128 and q_group in (1, 2, 4, 8)


def prefill_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_trans: Optional[torch.Tensor] = None,
                      seq_start: Optional[torch.Tensor] = None, seq_len: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal self-attention of a prompt (fq_prefill_attention_f16): q [batch, seq, q_heads, 128], k / v [batch, seq, kv_heads, 128] fp16 -> o
    like q. Query head h reads KV head h // (q_heads // kv_heads); scores / sqrt(head_dim), fp32 softmax, o rounded to fp16 once.
    ``q_trans`` [128, 128]: the query is fp16(q . q_trans) inside the launch. ``seq_start`` / ``seq_len`` (int32 [batch], both or neither):
    request b's tokens are positions seq_start[b] .. seq_start[b] + seq_len[b] - 1, causal within them; o outside the range is zeros and
    q / k / v outside it never change a result. Non-contiguous inputs are copied. head_dim 128."""
    q, k, v = (t.contiguous() if isinstance(t, torch.Tensor) else t for t in (q, k, v))
    _chk(q, "q"), _chk(k, "k"), _chk(v, "v")
    if k.device != q.device or v.device != q.device:
        raise ValueError(f"q, k, v must be on one device, got {q.device}, {k.device}, {v.device}")
    if q.dim() != 4 or k.dim() != 4 or k.shape != v.shape or q.shape[:2] != k.shape[:2] or q.shape[3] != k.shape[3]:
        raise ValueError(f"q [batch, seq, q_heads, head_dim] and k / v [batch, seq, kv_heads, head_dim] expected, got {tuple(q.shape)}, "
                         f"{tuple(k.shape)}, {tuple(v.shape)}")
    batch, seq, heads, hd = q.shape
    kv_heads = k.shape[2]
    if kv_heads < 1 or heads < 1 or heads % kv_heads:
        raise ValueError(f"q_heads={heads} must be a multiple of kv_heads={kv_heads} (both >= 1)")
    if q_trans is not None:
        q_trans = q_trans.contiguous() if isinstance(q_trans, torch.Tensor) else q_trans
        _chk(q_trans, "q_trans")
        if q_trans.shape != (hd, hd) or q_trans.device != q.device:
            raise ValueError("q_trans must be [head_dim, head_dim] on q's device")
    if (seq_start is None) != (seq_len is None):
        raise ValueError("seq_start and seq_len go together (both or neither)")
    if seq_start is not None:
        seq_start, seq_len = seq_start.contiguous(), seq_len.contiguous()
        for t, n in ((seq_start, "seq_start"), (seq_len, "seq_len")):
            _chk(t, n, torch.int32)
            if t.shape != (batch,):
                raise ValueError(f"{n} must be [batch] = [{batch}], got {tuple(t.shape)}")
            if t.device != q.device:
                raise ValueError(f"{n} is on {t.device}, q on {q.device}: the launch reads it on q's device")
        if seq_start.data_ptr() % 16:
            seq_start = seq_start.clone()
        if seq_len.data_ptr() % 16:
            seq_len = seq_len.clone()
    o = torch.empty((batch, seq, heads, hd), dtype=torch.float16, device=q.device)
    if batch == 0 or seq == 0:
        return o
    with _on(q.device):
        check(lib.fq_prefill_attention_f16(_ptr(o), _ptr(q), _ptr(q_trans), _ptr(k), _ptr(v), _ptr(seq_start), _ptr(seq_len), batch, seq,
                                           heads, kv_heads, hd, _stream(q)))
    return o


# Fragment images of the K transform for kv_decode_append (fq_kv_transform_image_f16: 32 KB per layer at head_dim 128), by (device, transform):
# [image, transform, event of the preparing launch, {"done", "streams"}]. Same protocol as the Kronecker images: the entry keeps the transform alive,
# in-place updates miss (ver), another stream waits for the preparing launch once; under capture only an image known complete (images_ready())
# or prepared on the capturing stream is shared — otherwise the capture prepares a private one — and whatever a captured launch was handed is pinned.
_KV_TIMG: "collections.OrderedDict" = CACHES.register("kv_transform_images", collections.OrderedDict())
_KV_TIMG_PINNED: dict = CACHES.register("kv_transform_images_pinned", {}, pinned=True)
_KV_TIMG_MAX = 1024


def kv_transform_image(trans: torch.Tensor) -> torch.Tensor:
    """The K transform [head_dim, head_dim] fp16 as the MFMA fragment image kv_decode_append reads (cached per transform tensor)."""
    _chk(trans, "trans")
    hd = trans.shape[-1]
    if trans.dim() != 2 or trans.shape[0] != hd:
        raise ValueError("trans must be [head_dim, head_dim]")
    dev = trans.device
    sh = _stream_handle(dev)
    capturing = torch.cuda.is_current_stream_capturing()
    key = (dev.index, trans.data_ptr(), ver(trans))
    ent = _KV_TIMG.get(key)
    if ent is not None:
        state = ent[3]
        if not (state["done"] or sh in state["streams"]):
            if capturing:
                ent = None                                  # (no event may be asked or waited for here: a private image inside the capture)
            elif ent[2].query():
                state["done"] = True
            else:
                torch.cuda.current_stream(dev).wait_event(ent[2])
                state["streams"].add(sh)
    if ent is not None:
        _KV_TIMG.move_to_end(key)
        img = ent[0]
    else:
        nbytes = int(lib.fq_kv_transform_image_bytes(hd))
        if nbytes <= 0:
            raise _lib.FqError(_lib.FQ_EUNSUPPORTED, f"kv_transform_image: head_dim={hd} must be 64 or 128")
        img = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with _on(dev):
            check(lib.fq_kv_transform_image_f16(_ptr(trans), hd, _ptr(img), _stream(trans)))
        if not capturing:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            _KV_TIMG[key] = [img, trans, ev, {"done": False, "streams": {sh}}]
            while len(_KV_TIMG) > _KV_TIMG_MAX:
                _KV_TIMG.popitem(last=False)
    if capturing:
        _KV_TIMG_PINNED.setdefault(id(img), (img, trans))
    return img


def kv_decode_append(q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, trans: Optional[torch.Tensor], kv_data: torch.Tensor,
                     kv_param: torch.Tensor, kv_indptr: torch.Tensor, kv_indices: torch.Tensor, last_page_offset: torch.Tensor,
                     layer_idx: int, q_trans: Optional[torch.Tensor] = None, transpose_out: bool = False, seq_hint: int = 0,
                     split: bool = True, read_one_copy: bool = False, rope=None, had: bool = False) -> torch.Tensor:
    """kv_quant_append(k_new, v_new, trans, ...) + kv_batch_decode(q, ...) of a decode step as ONE launch (fq_kv_decode_append_i4, round 6): the
    index tensors already count the new token (as for kv_quant_append), k_new / v_new [batch, kv_heads, head_dim] fp16 are its keys / values
    (the cache's heads are a multiple of kv_heads: the reference's replicated layout, or the shared one), q [batch, heads, head_dim]. The
    cache contents and the attention output are bit-identical to the two calls. INT4 cache, head_dim 128, page_size % 16 == 0
    (``kv_decode_append_supported``). ``read_one_copy``: on the replicated layout (cache heads = query heads = kv_heads x copies) the launch
    reads the first copy of every group (as kv_batch_decode(kv_copies=...)) and writes the new row to all of them.
    ``rope`` = (cos, sin), each [batch, head_dim] fp16 (round 8, fq_kv_decode_append_rope_i4): q and k_new are the UN-rotated projections and the
    launch applies the step's rotary embedding to them itself — the queries before ``q_trans``, the new K row before ``trans``, never V: cache
    contents and output bit-identical to ``rope(q, k_new, cos, sin)`` followed by this call without the argument.
    ``had=True`` (fq_kv_decode_append_had_i4; the cache's default ``trans="had"``): q and k_new are the UN-rotated projections and the launch applies
    the normalised Hadamard rotation over head_dim to them itself, never to V: cache contents and output bit-identical to
    ``kv_decode_append(hadamard(q), hadamard(k_new), v_new, None, ...)``. It excludes ``trans``, ``q_trans`` and ``rope`` (ValueError)."""
    if had and (trans is not None or q_trans is not None or rope is not None):
        raise ValueError("kv_decode_append(had=True): the launch's own Hadamard rotation excludes trans, q_trans and rope")
    o, dev, n_layers, cache_heads, page_size, hd, batch, heads, q_group, _, _, cache = _kv_attn_front(
        q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, q_trans, transpose_out, False, 1, True, k_new, v_new)
    src_heads = k_new.shape[1]
    cos = sin = None
    if rope is not None:
        cos, sin = rope
        _chk(cos, "cos"), _chk(sin, "sin")
        if cos.numel() != batch * hd or sin.numel() != batch * hd or cos.shape[-1] != hd or sin.shape[-1] != hd:
            raise ValueError(f"rope = (cos, sin) must each be [{batch}, {hd}] (the step's row of the tables per request)")
    img = kv_transform_image(trans) if trans is not None else None
    if batch == 0:
        return o
    with _on(dev):
        one = bool(read_one_copy) and q_group == 1 and cache_heads // src_heads > 1
        share = cache_heads // src_heads if one else q_group           # query heads that share one set of rows
        nbytes = int(lib.fq_kv_decode_workspace_bytes_gqa(batch, heads // share, share, hd)) if split else 0
        stream = ctypes.c_void_p(_stream_handle(dev))
        ws = _kv_split_workspace((dev.index, stream.value, batch * heads, hd), nbytes, dev) if nbytes > 0 else None
        args = (o.data_ptr(), q.data_ptr(), _ptr(q_trans), 1 if transpose_out else 0, k_new.data_ptr(), v_new.data_ptr(), _ptr(img), src_heads,
                *cache, n_layers, layer_idx, cache_heads, q_group, page_size, hd, batch, int(seq_hint), 1 if one else 0, _ptr(ws),
                nbytes if ws is not None else 0, stream)
        if had:
            had_scale = float(1.0 / torch.tensor(hd).sqrt())  # the fp32 value ops.hadamard passes for rows of head_dim
            check(lib.fq_kv_decode_append_had_i4(*args[:2], *args[3:6], *args[7:], ctypes.c_float(had_scale)))
        elif cos is None:
            check(lib.fq_kv_decode_append_i4(*args))
        else:
            check(lib.fq_kv_decode_append_rope_i4(*args, _ptr(cos), _ptr(sin)))
    return o


def rope(q: Optional[torch.Tensor], k: Optional[torch.Tensor], cos: torch.Tensor, sin: torch.Tensor, out=None):
    """Rotary position embedding of queries and keys in ONE launch (fq_rope_f16, round 8): transformers' ``apply_rotary_pos_emb(q, k, cos, sin,
    unsqueeze_dim=2)`` on fp16 tensors, bit for bit — ``(x * cos) + (rotate_half(x) * sin)`` with its three fp16 roundings. q [..., q_heads,
    head_dim] and k [..., k_heads, head_dim] over the same leading (token) dimensions, cos / sin [..., head_dim] with one row per token, taken
    as given. Either of q, k may be None. ``out`` = (q_out, k_out): where the results go — each may be its own input (in place); default: new
    tensors. -> (q_out, k_out), None for a tensor that was not given. head_dim 64 or 128."""
    if q is None and k is None:
        raise ValueError("rope: q and k are both None")
    _chk(cos, "cos"), _chk(sin, "sin")
    hd = cos.shape[-1]
    tokens = cos.numel() // hd if hd else 0
    if cos.shape != sin.shape:
        raise ValueError("rope: cos and sin must have the same shape [..., head_dim]")
    q_out, k_out = out if out is not None else (None, None)
    heads = []
    outs = []
    for t, o, name in ((q, q_out, "q"), (k, k_out, "k")):
        if t is None:
            heads.append(0), outs.append(None)
            continue
        _chk(t, name)
        if t.dim() < 2 or t.shape[-1] != hd or t.numel() != tokens * t.shape[-2] * hd:
            raise ValueError(f"rope: {name} must be [..., heads, {hd}] with {tokens} tokens (cos / sin hold one row per token), got {tuple(t.shape)}")
        if o is None:
            o = torch.empty_like(t)
        else:
            _chk(o, name + "_out")
            if o.shape != t.shape:
                raise ValueError(f"rope: {name}_out must have the shape of {name}")
        heads.append(t.shape[-2]), outs.append(o)
    if tokens == 0:
        return outs[0], outs[1]
    with _on(cos.device):
        check(lib.fq_rope_f16(_ptr(outs[0]), _ptr(outs[1]), _ptr(q), _ptr(k), _ptr(cos), _ptr(sin), tokens, heads[0], heads[1], hd, hd, _stream(cos)))
    return outs[0], outs[1]


def kv_decode_append_supported(kv_data: torch.Tensor, src_heads: int) -> bool:
    """Does fq_kv_decode_append_i4 take this cache? (INT4 pages, head_dim 128, a wave's 16 rows never straddle a page, at most 8 copies per head)"""
    if kv_data.dtype != torch.uint8:
        return False
    _, cache_heads, page_size, hd = _kv_geometry(kv_data)
    return hd == 128 and page_size % 16 == 0 and src_heads > 0 and cache_heads % src_heads == 0 and cache_heads // src_heads <= 8


def int4_matmul(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """_CUDA.matmul (bindings.cpp:9-25 -> gemm.cu): x uint8 [M, K/2], w uint8 [N, K/2], packed nibbles -> int32 [M, N]."""
    _chk(x, "x", torch.uint8), _chk(w, "w", torch.uint8)
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise RuntimeError(f"int4_matmul: expected x [M, K/2] and w [N, K/2], got {tuple(x.shape)} and {tuple(w.shape)}")
    M, N, K = x.shape[0], w.shape[0], x.shape[1] * 2
    c = torch.empty((M, N), dtype=torch.int32, device=x.device)
    if M == 0:
        return c
    with _on(x.device):
        check(lib.fq_int4_gemm_i32(_ptr(x), _ptr(w), M, N, K, _ptr(c), _stream(x)))
    return c


def int4_linear(x: torch.Tensor, x_scale: torch.Tensor, w: torch.Tensor, w_scale: torch.Tensor,
                bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Linear4bit.forward in one launch (fq_int4_linear_f16): packed x [M, K/2] with fp16 scales [M], packed w [N, K/2]
    with fp16 scales [N], optional fp16 bias [N] -> fp16 [M, N]; == sym_dequant(int4_matmul(x, w), ...) (+ bias)."""
    _chk(x, "x", torch.uint8), _chk(w, "w", torch.uint8), _chk(x_scale, "x_scale"), _chk(w_scale, "w_scale")
    if bias is not None:
        _chk(bias, "bias")
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise RuntimeError(f"int4_linear: expected x [M, K/2] and w [N, K/2], got {tuple(x.shape)} and {tuple(w.shape)}")
    M, N, K = x.shape[0], w.shape[0], x.shape[1] * 2
    if x_scale.numel() != M or w_scale.numel() != N or (bias is not None and bias.numel() != N):
        raise RuntimeError("int4_linear: scale / bias sizes do not match M / N")
    y = torch.empty((M, N), dtype=torch.float16, device=x.device)
    if M == 0:
        return y
    with _on(x.device):
        check(lib.fq_int4_linear_f16(_ptr(x), _ptr(x_scale), _ptr(w), _ptr(w_scale), _ptr(bias), M, N, K, _ptr(y),
                                     _stream(x)))
    return y


def _chk_grouped_gemm(what: str, x: torch.Tensor, w_g: torch.Tensor, group_offsets: torch.Tensor):
    """The operands every grouped GEMM shares -> (rows, n_groups, N, K). Nothing here reads a tensor's contents."""
    _chk(x, "x", torch.uint8), _chk(w_g, "w_g", torch.uint8), _chk(group_offsets, "group_offsets", torch.int64)
    if x.dim() != 2 or w_g.dim() != 3 or x.shape[1] != w_g.shape[2]:
        raise RuntimeError(f"{what}: expected x [rows, K/2] and w_g [n_groups, N, K/2], got {tuple(x.shape)} and {tuple(w_g.shape)}")
    G = w_g.shape[0]
    if group_offsets.dim() != 1 or group_offsets.numel() != G + 1:
        raise RuntimeError(f"{what}: group_offsets must have n_groups + 1 = {G + 1} entries, got {tuple(group_offsets.shape)}")
    if group_offsets.device != x.device or w_g.device != x.device:
        raise RuntimeError(f"{what}: x, w_g and group_offsets must be on one device")
    return x.shape[0], G, w_g.shape[1], x.shape[1] * 2


def int4_matmul_grouped(x: torch.Tensor, w_g: torch.Tensor, group_offsets: torch.Tensor) -> torch.Tensor:
    """int4_matmul of every group (expert) in one launch (fq_int4_gemm_grouped_i32): x uint8 [rows, K/2] sorted by group, group g owns rows
    [group_offsets[g], group_offsets[g+1]) and multiplies with w_g[g] (uint8 [n_groups, N, K/2]) -> int32 [rows, N]. group_offsets is the int64
    device tensor of moe_group_rows / kron_quant_grouped; nothing is read back (capturable). Bit-identical to int4_matmul per row slice."""
    rows, G, N, K = _chk_grouped_gemm("int4_matmul_grouped", x, w_g, group_offsets)
    c = torch.empty((rows, N), dtype=torch.int32, device=x.device)
    if rows == 0:
        return c
    with _on(x.device):
        check(lib.fq_int4_gemm_grouped_i32(_ptr(x), _ptr(w_g), rows, N, K, _ptr(group_offsets), G, _ptr(c), _stream(x)))
    return c


def int4_linear_grouped(x: torch.Tensor, x_scale: torch.Tensor, w_g: torch.Tensor, w_scale_g: torch.Tensor, group_offsets: torch.Tensor,
                        bias_g: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Linear4bit.forward of every group (expert) in one launch (fq_int4_linear_grouped_f16): the packed rows and per-token fp16 scales
    [rows] of kron_quant_grouped(FQ_OUT_PACKED), w_g uint8 [n_groups, N, K/2], w_scale_g fp16 [n_groups, N], optional bias_g fp16
    [n_groups, N] -> fp16 [rows, N]. An extension (the reference's MoE path is fake-quant only); bit-identical to int4_linear on each
    group's row slice, without the host loop and the ``offsets.tolist()`` it needs."""
    rows, G, N, K = _chk_grouped_gemm("int4_linear_grouped", x, w_g, group_offsets)
    _chk(x_scale, "x_scale"), _chk(w_scale_g, "w_scale_g")
    if bias_g is not None:
        _chk(bias_g, "bias_g")
    if x_scale.numel() != rows or w_scale_g.numel() != G * N or (bias_g is not None and bias_g.numel() != G * N):
        raise RuntimeError("int4_linear_grouped: scale / bias sizes do not match rows / n_groups x N")
    y = torch.empty((rows, N), dtype=torch.float16, device=x.device)
    if rows == 0:
        return y
    with _on(x.device):
        check(lib.fq_int4_linear_grouped_f16(_ptr(x), _ptr(x_scale), _ptr(w_g), _ptr(w_scale_g), _ptr(bias_g), rows, N, K,
                                             _ptr(group_offsets), G, _ptr(y), _stream(x)))
    return y


def sym_quant(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """_CUDA.sym_quant (bindings.cpp:27-44): x fp16 [rows, cols], scale fp16 [rows] -> uint8 [rows, ceil(cols/2)]."""
    _chk(x, "x"), _chk(scale, "scale")
    if x.dim() != 2:
        raise RuntimeError("sym_quant: x must be 2-D")
    rows, cols = x.shape
    if scale.numel() != rows:
        raise RuntimeError(f"sym_quant: expected scale to have {rows} elements, got {scale.numel()}")
    q = torch.empty((rows, (cols + 1) // 2), dtype=torch.uint8, device=x.device)
    if rows == 0:
        return q
    with _on(x.device):
        check(lib.fq_sym_quant_f16(_ptr(x), _ptr(scale), rows, cols, _ptr(q), _stream(x)))
    return q


def sym_dequant(q: torch.Tensor, scale_row: torch.Tensor, scale_col: torch.Tensor) -> torch.Tensor:
    """_CUDA.sym_dequant (bindings.cpp:47-87), bits = 32."""
    _chk(q, "q", torch.int32), _chk(scale_row, "scale_row"), _chk(scale_col, "scale_col")
    if q.dim() != 2:
        raise RuntimeError("sym_dequant: q must be 2-D")
    rows, cols = q.shape
    if scale_row.numel() != rows or scale_col.numel() != cols:
        raise RuntimeError("sym_dequant: scale sizes do not match q")
    x = torch.empty((rows, cols), dtype=torch.float16, device=q.device)
    if rows == 0:
        return x
    with _on(q.device):
        check(lib.fq_sym_dequant_i32_f16(_ptr(q), _ptr(scale_row), _ptr(scale_col), rows, cols, _ptr(x),
                                         _stream(q)))
    return x
