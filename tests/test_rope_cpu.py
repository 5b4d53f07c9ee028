"""Rotary position embedding, the parts that need no GPU: the CPU restatement the GPU tests compare against is torch's fp16 expression bit
for bit (and is NOT the single-rounding form), the new entry points are declared and exported, and bad arguments are refused with their
codes before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

from tests.conftest import same_bits
from tests.rope_ref import llama3_tables, rope_ref, rope_single_rounding, rope_torch


def _random_case(seed, tokens, heads, hd):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(tokens, heads, hd, generator=g) * 1.5).half()
    cos = (torch.rand(tokens, hd, generator=g) * 2 - 1).half()          # (halves NOT equal: the tables are taken as given)
    sin = (torch.rand(tokens, hd, generator=g) * 2 - 1).half()
    return x, cos, sin


def _llama_case(seed, heads, hd):
    g = torch.Generator().manual_seed(seed)
    pos = torch.cat([torch.arange(0, 64), torch.randint(0, 8192, (448,), generator=g), torch.tensor([8191])])
    cos, sin = llama3_tables(pos, hd)
    x = (torch.randn(pos.numel(), heads, hd, generator=g) * 2).half()
    return x, cos, sin


CASES = [lambda: _random_case(0, 257, 8, 128), lambda: _random_case(1, 130, 3, 64), lambda: _llama_case(2, 8, 128), lambda: _llama_case(3, 4, 64)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_rope_ref_is_the_torch_fp16_expression(case):
    x, cos, sin = CASES[case]()
    assert not torch.equal(cos[:, :cos.shape[1] // 2], cos[:, cos.shape[1] // 2:]) or case >= 2
    want = rope_torch(x, cos, sin)
    assert want.dtype == torch.float16
    assert same_bits(rope_ref(x, cos, sin).numpy(), want.numpy())


@pytest.mark.parametrize("case", range(len(CASES)))
def test_rope_ref_is_not_the_single_rounding_form(case):
    """the power of the bit-identity tests: a fused multiply-add implementation would not pass them"""
    x, cos, sin = CASES[case]()
    a, b = rope_ref(x, cos, sin), rope_single_rounding(x, cos, sin)
    differ = float((a.view(torch.int16) != b.view(torch.int16)).float().mean())
    assert differ > 0.05, differ
    assert float((a.float() - b.float()).abs().max()) <= float(x.float().abs().max()) * 2.0 ** -8      # (... while being the same function)


def test_new_symbols_are_declared_and_exported():
    import os
    import re
    from flatquant_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fqhip.h")).read()
    for name, nargs in (("fq_rope_f16", 12), ("fq_kv_decode_append_rope_i4", 27)):
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and m.group(1).count(",") + 1 == nargs, name
        assert getattr(_lib.lib, name) is not None
    from flatquant_amd import ops
    from flatquant_amd.deploy import functional
    assert callable(ops.rope) and callable(functional.apply_rotary_pos_emb)


def test_bad_arguments_are_refused_before_any_launch():
    """(the pointers are never dereferenced: every refusal comes before the first HIP call)"""
    from flatquant_amd._lib import FQ_EINVAL, FQ_EUNSUPPORTED, lib
    vp, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008)

    def rope(q_out=vp, k_out=vp, q=vp, k=vp, cos=vp, sin=vp, tokens=4, qh=8, kh=2, hd=128, rot=None):
        return lib.fq_rope_f16(q_out, k_out, q, k, cos, sin, tokens, qh, kh, hd, hd if rot is None else rot, None)

    for hd in (32, 96, 256, 0):
        assert rope(hd=hd) == FQ_EUNSUPPORTED and b"head_dim" in lib.fq_last_error()
    assert rope(rot=64) == FQ_EUNSUPPORTED and b"partial" in lib.fq_last_error()          # partial rotary
    assert rope(hd=64, rot=32) == FQ_EUNSUPPORTED
    assert rope(q=None, k=None) == FQ_EINVAL and b"both NULL" in lib.fq_last_error()
    for name in ("q_out", "k_out", "q", "k", "cos", "sin"):
        assert rope(**{name: odd}) == FQ_EINVAL and b"aligned" in lib.fq_last_error(), name
    assert rope(cos=None) == FQ_EINVAL and rope(sin=None) == FQ_EINVAL
    assert rope(q_out=None) == FQ_EINVAL and rope(k_out=None) == FQ_EINVAL               # an input without its output
    assert rope(qh=0) == FQ_EINVAL and rope(kh=-1) == FQ_EINVAL and rope(tokens=-1) == FQ_EINVAL
    assert rope(tokens=0) == 0                                                            # nothing to do is not an error

    def fused(cos=vp, sin=vp, hd=128, page=16, k_new=vp):
        return lib.fq_kv_decode_append_rope_i4(vp, vp, None, 0, k_new, vp, None, 2, vp, vp, vp, vp, vp, 1, 0, 2, 1, page, hd, 1, 0, 0, None, 0, None, cos, sin)

    assert fused(hd=64) == FQ_EUNSUPPORTED and fused(page=24) == FQ_EUNSUPPORTED
    assert fused(cos=None) == FQ_EINVAL and b"cos and sin" in lib.fq_last_error()
    assert fused(sin=None) == FQ_EINVAL
    assert fused(cos=odd) == FQ_EINVAL and fused(sin=odd) == FQ_EINVAL
    assert fused(k_new=None) == FQ_EINVAL
