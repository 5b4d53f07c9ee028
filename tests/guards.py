"""Guard bands around the buffers the code under test allocates for itself, without changing that code.

The product modules (``flatquant_amd/ops.py``, ``deploy/transformers/kv_cache.py``, ``deploy/nn/linear.py``) reach the allocator only
through their module-level name ``torch``. ``Guard(poison).on(module)`` replaces that name, in that module only, with a proxy that forwards
every attribute to the real ``torch`` except ``empty``, ``empty_like``, ``zeros``, ``zeros_like`` and ``full`` (the product uses no
``new_*`` form). Those return a contiguous view into the middle of a larger uint8 buffer:

    [ front pad: poison ][ payload: poison (empty*) / zeros (zeros*) / the value (full) ][ back pad: poison ]

so that a kernel that writes before or behind its output hits memory the TEST owns, where ``check()`` sees it, and an element a kernel
forgets to write holds the poison, not the previous launch's correct result. Objects that allocate at construction (LaunchPlan,
FreshPlan, KronMultiPlan, the paged cache) are built while the proxy is installed.

Geometry
  * front pad: a multiple of 256 bytes — the allocators hand out blocks aligned to at least 64 bytes, so the payload keeps the 16-byte
    alignment the library checks (FQ_NEED_ALIGN16) and every element type stays naturally aligned;
  * back pad: starts at the payload's last byte + 1, NOT rounded up to 16 — a full 16-byte store on a 74-byte packed row lands in it;
  * size of each pad: 256 further rows of the tensor's own last dimension (the widest tile that writes rows is the FP6 GEMM's 256 x 256,
    the decode GEMM's is 128; a Kronecker launch's unit is one token = one row, so 256 rows cover it many times over), at least
    PAD_FLOOR = 64 KiB (a whole stray 128 x 256 int16 tile, and every 1-D scale / counter vector) and at most PAD_CAP = 2 MiB (a
    16384-row, 16 KiB-per-row case then pays 4 MiB, not twice its footprint; the cap still holds 16 rows of the widest 64 Ki-element
    token, and one row is all a token-per-workgroup kernel can overrun by).

Poison: ``0x5A`` or ``0xA5``, chosen per Guard. Neither byte makes an inf or NaN in fp16 (0x5A5A = 203.25, 0xA5A5 = -0.0222) or bf16, both are
legal INT4 pairs, and they differ in every bit: an output that is bit-identical under both was written completely by the launch.

Inputs: ``guard_input`` copies a tensor into a guarded buffer whose pads would CHANGE A RESULT if they were read: NaN for floating point
(fp16 0x7E7E / 0xFFFF for the two poisons), 0xFF / 0x88 for packed bytes. Tensors of indices, offsets or pointers (kv_indptr, kv_indices,
last_page_offset, seqlen_indptr, group_offsets, job tables) are padded with entries that are VALID for the call — a repeat of the last
entry, or zeros — never with garbage: an over-read of an index must not be able to become a wild address. Asking for a NaN / 0xFF pad
around an integer tensor raises. The same rule for what the PRODUCT allocates: an int16 / int32 / int64 tensor made with zeros / full (the
paged cache's own indptr / indices / last_page_offset, group offsets) gets pads of zeros, checked against zeros. Limits, stated: a zero pad
cannot show a stray store of zeros; integer tensors made with ``empty`` are compute outputs (the int32 GEMM results) and keep poison pads;
and a BYTE buffer that holds pointers (KronMultiPlan's job table) cannot be told from any other byte buffer and keeps poison pads — its
cases here are direct launches on tables the library itself sized, not the module-level cases.

The proxy implements shape, dtype and device only: any other keyword, and any *_like of a non-contiguous tensor, raises, so that a product
call that starts to rely on one cannot silently behave differently under the guard.

No fault is provoked by any of this. The guards only make an overrun land in memory the test owns. A correct kernel touches exactly the
bytes it would touch without them, and no test built on this module may index, size or align anything so that a correct kernel would
leave its allocations."""
import contextlib

import torch as _torch

POISONS = (0x5A, 0xA5)
PAD_FLOOR = 64 << 10
PAD_CAP = 2 << 20
_NAN_BITS = {_torch.float16: (0x7E7E, -1), _torch.bfloat16: (0x7FFE, -1), _torch.float32: (0x7FC07E7E, -1), _torch.float64: (0x7FF8007E7E7E7E7E, -1)}
_INT_VIEW = {2: _torch.int16, 4: _torch.int32, 8: _torch.int64}
_BYTE_PADS = (0xFF, 0x88)


def pad_bytes(shape, itemsize: int) -> int:
    """Size of each pad of a tensor: 256 rows of its last dimension, within [PAD_FLOOR, PAD_CAP], a multiple of 256."""
    row = (int(shape[-1]) if len(shape) else 1) * itemsize
    n = min(max(256 * row, PAD_FLOOR), PAD_CAP)
    return (n + 255) // 256 * 256


class GuardError(AssertionError):
    pass


class _Record:
    __slots__ = ("buf", "front", "nbytes", "shape", "dtype", "what", "fill")

    def __init__(self, buf, front, nbytes, shape, dtype, what, fill):
        self.buf, self.front, self.nbytes, self.shape, self.dtype, self.what, self.fill = buf, front, nbytes, tuple(shape), dtype, what, fill

    def pads(self):
        return (("front", self.buf[:self.front], -self.front), ("back", self.buf[self.front + self.nbytes:], self.nbytes))


def _fill_pad(pad, fill):
    """fill: an int byte, or (int dtype, bit pattern) for multi-byte patterns (the pads are multiples of 256 bytes, 256-aligned)"""
    if isinstance(fill, tuple):
        pad.view(fill[0]).fill_(fill[1])
    else:
        pad.fill_(fill)


def _pad_damage(pad, fill):
    """-> a boolean tensor over the pad's BYTES, true where the byte no longer holds the fill"""
    if isinstance(fill, tuple):
        ref = _torch.empty_like(pad)
        _fill_pad(ref, fill)
        return pad != ref
    return pad != fill


class _Proxy:
    """Stands in for the ``torch`` name of ONE product module. Everything but the allocating factories is the real thing."""

    def __init__(self, guard):
        object.__setattr__(self, "_guard", guard)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the torch proxy is read-only")

    @staticmethod
    def _size(size):
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        return tuple(int(s) for s in size)

    @staticmethod
    def _only(kw, like=None):
        """The proxy implements shape, dtype and device. Any other keyword (pin_memory, memory_format, layout, out, requires_grad=True ...)
        and any *_like of a tensor that is not contiguous would behave differently under the guard than in the product: refuse them."""
        kw = {k: v for k, v in kw.items() if not (k == "requires_grad" and v is False)}
        if kw:
            raise TypeError(f"the torch proxy of tests/guards.py does not implement {sorted(kw)}: extend it before the product relies on them")
        if like is not None and not like.is_contiguous():
            raise TypeError("the torch proxy of tests/guards.py hands out contiguous tensors only: *_like of a strided tensor")

    def empty(self, *size, dtype=None, device=None, **kw):
        self._only(kw)
        return self._guard.alloc(self._size(size), dtype, device, "empty")

    def zeros(self, *size, dtype=None, device=None, **kw):
        self._only(kw)
        return self._guard.alloc(self._size(size), dtype, device, "zeros")

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        self._only(kw)
        if dtype is None:
            dtype = _torch.get_default_dtype() if isinstance(fill_value, float) else _torch.int64
        t = self._guard.alloc(self._size((size,)), dtype, device, "full")
        return t.fill_(fill_value)

    def empty_like(self, t, dtype=None, device=None, **kw):
        self._only(kw, t)
        return self._guard.alloc(tuple(t.shape), dtype or t.dtype, device or t.device, "empty")

    def zeros_like(self, t, dtype=None, device=None, **kw):
        self._only(kw, t)
        return self._guard.alloc(tuple(t.shape), dtype or t.dtype, device or t.device, "zeros")


class Guard:
    """One poison byte, one registry. ``with guard.on(ops): ...`` (or ``monkeypatch.setattr(ops, "torch", guard.proxy)``), then
    ``guard.check()``."""

    def __init__(self, poison: int):
        if poison not in POISONS:
            raise ValueError(f"poison must be one of {[hex(p) for p in POISONS]}")
        self.poison = poison
        self.variant = POISONS.index(poison)
        self.records = []
        self.proxy = _Proxy(self)

    @contextlib.contextmanager
    def on(self, *modules):
        saved = [(m, m.__dict__["torch"]) for m in modules]      # (KeyError: the module does not allocate through the name ``torch``)
        try:
            for m in modules:
                m.torch = self.proxy
            yield self
        finally:
            for m, t in saved:
                m.torch = t

    def _carve(self, shape, dtype, device, what, pad_fill, payload_fill):
        dtype = dtype or _torch.get_default_dtype()
        itemsize = _torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * itemsize
        pad = pad_bytes(shape, itemsize)
        buf = _torch.empty(pad + nbytes + pad, dtype=_torch.uint8, device=device)
        assert buf.data_ptr() % 16 == 0, "allocator returned a block that is not 16-byte aligned"
        rec = _Record(buf, pad, nbytes, shape, dtype, what, pad_fill)
        for _, p, _ in rec.pads():
            _fill_pad(p, pad_fill)
        payload = buf[pad:pad + nbytes]
        if payload_fill is not None:
            payload.fill_(payload_fill)
        self.records.append(rec)
        return payload.view(dtype).view(shape)

    def alloc(self, shape, dtype, device, what):
        dt = dtype or _torch.get_default_dtype()
        index_like = what in ("zeros", "full") and not dt.is_floating_point and dt != _torch.bool and _torch.empty((), dtype=dt).element_size() > 1
        # int16 / int32 / int64 tensors the product creates with zeros / full are index, offset and length tensors (the paged cache's indptr /
        # indices / last_page_offset, MoE group offsets): their pads hold zeros, a VALID entry, and are checked against zeros
        return self._carve(shape, dtype, device, what, 0 if index_like else self.poison, 0 if what == "zeros" else self.poison)

    def guard_input(self, t, pad="auto"):
        """A copy of ``t`` between pads. pad: "auto" (floating point: NaN; uint8 / int8: 0xFF-class bytes; wider integers: "repeat"),
        "nan", "ff", "zeros", "repeat" (the last entry of ``t``, zeros for an empty tensor)."""
        t = t.contiguous()
        integer = not t.dtype.is_floating_point
        wide_int = integer and t.element_size() > 1
        if pad == "auto":
            pad = "nan" if not integer else ("repeat" if wide_int else "ff")
        if pad == "nan":
            if integer:
                raise TypeError(f"guard_input: a {t.dtype} tensor cannot be NaN-padded; index tensors take 'zeros' or 'repeat'")
            fill = (_INT_VIEW[t.element_size()], _NAN_BITS[t.dtype][self.variant])
        elif pad == "ff":
            if wide_int:
                raise TypeError(f"guard_input: a {t.dtype} tensor holds indices / offsets: pad it with 'zeros' or 'repeat', never garbage")
            fill = _BYTE_PADS[self.variant]
        elif pad == "zeros" or (pad == "repeat" and t.numel() == 0):
            fill = 0
        elif pad == "repeat":
            last = t.reshape(-1)[-1:].clone()
            if t.element_size() == 1:
                fill = int(last.view(_torch.uint8).item())
            else:
                fill = (_INT_VIEW[t.element_size()], int(last.view(_INT_VIEW[t.element_size()]).item()))
        else:
            raise ValueError(f"guard_input: unknown pad {pad!r}")
        v = self._carve(tuple(t.shape), t.dtype, t.device, "input", fill, None)
        v.copy_(t)
        return v

    def check(self, what=("empty", "zeros", "full", "input")):
        """Every pad of every buffer handed out still holds its fill: one reduction per pad on the tensor's device, one flag read back per
        check. On damage: which tensor (shape, dtype), which pad, first and last damaged byte offset relative to the payload's start."""
        recs = [r for r in self.records if r.what in what]
        flags = [_pad_damage(p, r.fill).any() for r in recs for _, p, _ in r.pads()]
        if not flags or not bool(_torch.stack([f.to(flags[0].device) for f in flags]).any()):
            return
        lines = []
        for r in recs:
            for side, p, base in r.pads():
                bad = _pad_damage(p, r.fill).nonzero()
                if bad.numel():
                    first, last = int(bad[0]) + base, int(bad[-1]) + base
                    lines.append(f"{side} pad of {r.what} tensor shape={r.shape} dtype={r.dtype} ({r.nbytes} payload bytes) damaged: "
                                 f"{bad.numel()} bytes, first at payload offset {first}, last at {last}")
        raise GuardError("write outside an allocation:\n  " + "\n  ".join(lines))

    def payload_bytes(self, view):
        """The uint8 payload of a tensor this guard handed out (by address)."""
        for r in self.records:
            if r.buf.data_ptr() + r.front == view.data_ptr():
                return r.buf[r.front:r.front + r.nbytes]
        raise KeyError("not a tensor of this guard")

    def find(self, what, nbytes=None):
        """Records of one kind (and payload size): the way to a workspace the product keeps to itself."""
        return [r for r in self.records if r.what == what and (nbytes is None or r.nbytes == nbytes)]


def raw(t):
    """The tensor's bytes, for bit comparisons (``same_bits`` on the device)."""
    return t.detach().contiguous().reshape(-1).view(_torch.uint8)


def same_raw(a, b) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and bool(_torch.equal(raw(a), raw(b)))


# A stand-in "op" module for the helper's own tests (CPU and device): exec'd into a fresh module whose ``torch`` is then proxied.
STANDIN_SOURCE = '''
import torch


def scale_rows(x):                      # a correct op: writes every element of a fresh output
    y = torch.empty_like(x)
    y.copy_(x * 2)
    return y


def skips_last_row(x):                  # forgets the last row
    y = torch.empty_like(x)
    y[:-1].copy_(x[:-1] * 2)
    return y


def counters(n):
    return torch.zeros((n,), dtype=torch.int32, device="cpu")


def flags(n):
    return torch.zeros((n,), dtype=torch.uint8)


def filled(n):
    return torch.full((n,), 3.0, dtype=torch.float16)


def sized(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8)


def pinned(n):
    return torch.empty(n, dtype=torch.uint8, pin_memory=True)
'''


def standin_module(name="guards_standin_ops"):
    import types
    mod = types.ModuleType(name)
    exec(compile(STANDIN_SOURCE, name, "exec"), mod.__dict__)
    return mod
