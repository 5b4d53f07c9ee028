"""The prompt attention launch (fq_prefill_attention_f16) without a GPU: the symbol and its declaration, the argument checks of the C entry
(they return before any HIP call, the pointers are never dereferenced), the host helper that turns an attention mask into ranges, and the
compiler's resource report of the new file's kernels."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_with_thirteen_arguments():
    from flatquant_amd import _lib
    assert "fq_prefill_attention_f16" in _lib.SYMBOLS
    restype, argtypes = _lib.SYMBOLS["fq_prefill_attention_f16"]
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert argtypes[:7] == [ctypes.c_void_p] * 7 and argtypes[7:12] == [ctypes.c_int] * 5 and argtypes[12] is ctypes.c_void_p
    header = open(os.path.join(ROOT, "include", "fqhip.h")).read()
    m = re.search(r"\bint\s+fq_prefill_attention_f16\s*\(([^)]*)\)\s*;", header)
    assert m, "not declared in include/fqhip.h"
    assert len(m.group(1).split(",")) == 13
    assert hasattr(_lib.lib, "fq_prefill_attention_f16")


def test_argument_checks_return_before_any_launch():
    from flatquant_amd._lib import FQ_EINVAL, FQ_EUNSUPPORTED, lib
    vp, odd = 0x1000, 0x1008

    def call(o=vp, q=vp, qt=None, k=vp, v=vp, start=None, length=None, batch=1, seq=16, q_heads=8, kv_heads=2, head_dim=128):
        return lib.fq_prefill_attention_f16(o, q, qt, k, v, start, length, batch, seq, q_heads, kv_heads, head_dim, None)
    assert call(head_dim=64) == FQ_EUNSUPPORTED and b"head_dim" in lib.fq_last_error()
    assert call(head_dim=96) == FQ_EINVAL
    assert call(head_dim=256) == FQ_EINVAL
    assert call(batch=0) == FQ_EINVAL
    assert call(seq=0) == FQ_EINVAL
    assert call(q_heads=0) == FQ_EINVAL
    assert call(kv_heads=0) == FQ_EINVAL
    assert call(q_heads=6, kv_heads=4) == FQ_EINVAL and b"multiple" in lib.fq_last_error()
    assert call(start=vp) == FQ_EINVAL and b"seq_start" in lib.fq_last_error()         # exactly one of the two
    assert call(length=vp) == FQ_EINVAL
    assert call(o=None) == FQ_EINVAL and call(q=None) == FQ_EINVAL and call(k=None) == FQ_EINVAL and call(v=None) == FQ_EINVAL
    for name in ("o", "q", "qt", "k", "v"):                                            # every tensor starts on a 16-byte boundary
        assert call(**{name: odd}) == FQ_EINVAL, name
        assert b"16-byte aligned" in lib.fq_last_error(), name
    assert call(start=odd, length=vp) == FQ_EINVAL and b"16-byte aligned" in lib.fq_last_error()
    assert call(start=vp, length=odd) == FQ_EINVAL and b"16-byte aligned" in lib.fq_last_error()


def test_mask_ranges_on_cpu_tensors():
    from flatquant_amd.deploy.functional import mask_ranges
    mask = torch.tensor([[0, 0, 1, 1, 1, 1],       # left-padded
                         [1, 1, 1, 0, 0, 0],       # right-padded
                         [1, 1, 1, 1, 1, 1],       # full
                         [0, 0, 0, 0, 0, 0],       # empty
                         [0, 0, 0, 1, 0, 0],       # one token
                         [0, 0, 0, 0, 0, 1]])
    start, length = mask_ranges(mask)
    assert start.dtype == torch.int32 and length.dtype == torch.int32 and start.shape == (6,) and length.shape == (6,)
    assert length.tolist() == [4, 3, 6, 0, 1, 1]
    assert [s for s, n in zip(start.tolist(), length.tolist()) if n] == [2, 0, 0, 3, 5]
    assert 0 <= start.tolist()[3] <= 6                                                 # (an empty row's start is any position of the tensor)
    start, length = mask_ranges(mask.bool())
    assert length.tolist() == [4, 3, 6, 0, 1, 1]
    for hole in ([1, 0, 1, 1, 1, 1], [1, 1, 0, 0, 0, 1], [0, 1, 0, 1, 0, 0]):
        bad = mask.clone()
        bad[2] = torch.tensor(hole)
        with pytest.raises(NotImplementedError):
            mask_ranges(bad)
    with pytest.raises(ValueError):
        mask_ranges(torch.ones(6))


def test_surface_refuses_what_it_does_not_compute_without_a_gpu():
    from flatquant_amd import ops
    from flatquant_amd.deploy.functional import flash_attention_forward
    from flatquant_amd.deploy.transformers import attention_core
    q = torch.zeros(1, 4, 2, 128, dtype=torch.float16)
    with pytest.raises(NotImplementedError):
        flash_attention_forward(q, q, q, 4, is_causal=False)
    with pytest.raises(NotImplementedError):
        flash_attention_forward(q[:, :1], q, q, 1)                                     # a query shorter than the keys
    with pytest.raises(NotImplementedError):
        flash_attention_forward(q, q, q, 4, attention_mask=torch.tensor([[1, 0, 1, 1]]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.prefill_attention(q, q, q)
    assert attention_core(lambda x: x + 1, torch.zeros(2), None).tolist() == [1.0, 1.0]   # a closure is called with the queries


def test_new_kernels_do_not_spill_and_keep_two_waves_per_simd():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import parse
    res = {k: r for k, r in parse().items() if r["file"] == "fq_prefill_attn"}
    if not res:
        pytest.skip("no build/fq_prefill_attn.res next to the sources (library built elsewhere)")
    assert set(res) == {"fq_prefill_attn_kernel<0>", "fq_prefill_attn_kernel<1>"}, sorted(res)
    for name, r in res.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        # 2 waves per SIMD: the occupancy the kernel was written for and built at — __launch_bounds__(256, 2) with the 64 KB two-deep K / V ring
        # (two workgroups of four waves per CU); the first build reported 249 VGPRs, occupancy 2, no spill (build/fq_prefill_attn.res)
        assert r["occupancy"] >= 2, (name, r)
