"""fq_kv_decode_append_had_i4 without a device: the header, the binding table and the library agree on the new entry point, and every refusal
that needs no GPU comes before the first HIP call."""
import ctypes
import os
import re

import pytest
import torch


def test_the_new_symbol_is_declared_bound_and_exported():
    from flatquant_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fqhip.h")).read()
    name, nargs = "fq_kv_decode_append_had_i4", 24
    assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
    assert m and m.group(1).count(",") + 1 == nargs
    assert m.group(1).rstrip().endswith("float had_scale") and "q_trans" not in m.group(1) and "k_trans_image" not in m.group(1)
    assert _lib.SYMBOLS[name][1][-1] is ctypes.c_float
    # fq_kv_decode_append_i4's arguments without q_trans / k_trans_image, plus the scale
    plain = list(_lib.SYMBOLS["fq_kv_decode_append_i4"][1])
    assert _lib.SYMBOLS[name][1] == plain[:2] + plain[3:6] + plain[7:] + [ctypes.c_float]
    assert getattr(_lib.lib, name) is not None
    # the header states the contract and no longer calls a NULL image the "had" configuration
    assert "BIT-IDENTICAL" in header[header.index("THE HADAMARD ROTATION OF THE CACHE"):header.index("int " + name)]
    assert 'NULL: keys are not transformed — trans "had" / none' not in header


def test_bad_arguments_are_refused_before_any_launch():
    """(the pointers are never dereferenced: every refusal comes before the first HIP call)"""
    from flatquant_amd._lib import FQ_EINVAL, FQ_EUNSUPPORTED, lib
    vp, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008)
    scale = ctypes.c_float(128 ** -0.5)

    def had(hd=128, page=16, q=vp, k_new=vp, v_new=vp, src=2, kv_heads=2, group=1, layer=0):
        return lib.fq_kv_decode_append_had_i4(vp, q, 0, k_new, v_new, src, vp, vp, vp, vp, vp, 1, layer, kv_heads, group, page, hd, 1, 0, 0, None, 0, None, scale)

    assert had(hd=64) == FQ_EUNSUPPORTED and b"fq_kv_decode_append_had_i4" in lib.fq_last_error()
    assert had(page=8) == FQ_EUNSUPPORTED and had(page=24) == FQ_EUNSUPPORTED and had(hd=96) == FQ_EUNSUPPORTED
    assert had(k_new=None) == FQ_EINVAL and had(v_new=None) == FQ_EINVAL and had(q=None) == FQ_EINVAL
    assert had(k_new=odd) == FQ_EINVAL and b"aligned" in lib.fq_last_error()
    assert had(src=0) == FQ_EINVAL and had(src=3) == FQ_EINVAL and had(kv_heads=32, src=2) == FQ_EINVAL       # (sixteen copies per source head)
    assert had(group=0) == FQ_EINVAL and had(layer=1) == FQ_EINVAL


def test_ops_refuses_had_with_another_transform_without_a_device():
    from flatquant_amd import ops
    t = torch.zeros(1, 2, 128, dtype=torch.float16)
    m = torch.zeros(128, 128, dtype=torch.float16)
    pages, par, idx = torch.zeros(1, 1, 2, 2, 16, 64, dtype=torch.uint8), torch.zeros(1, 1, 2, 2, 16, 2, dtype=torch.float16), torch.zeros(2, dtype=torch.int32)
    for kw in (dict(trans=m), dict(q_trans=m), dict(rope=(t[0], t[0]))):
        trans = kw.pop("trans", None)
        with pytest.raises(ValueError, match="had=True"):
            ops.kv_decode_append(t, t, t, trans, pages, par, idx, idx[:1], idx[:1], 0, had=True, **kw)
    with pytest.raises(RuntimeError, match="CUDA/ROCm"):        # (had alone passes that check and meets the next one: no CPU path)
        ops.kv_decode_append(t, t, t, None, pages, par, idx, idx[:1], idx[:1], 0, had=True)
    import inspect
    assert inspect.signature(ops.kv_decode_append).parameters["had"].default is False
