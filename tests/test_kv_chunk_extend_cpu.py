"""fq_kv_chunk_extend without a GPU: the symbol and its declaration, the argument checks of the C entry (they return before any HIP call, the
pointers are never dereferenced), the compiler's resource report of the new file's kernels, the cache class's routing constant."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_with_twenty_arguments():
    from flatquant_amd import _lib
    assert "fq_kv_chunk_extend" in _lib.SYMBOLS
    restype, argtypes = _lib.SYMBOLS["fq_kv_chunk_extend"]
    assert restype is ctypes.c_int and len(argtypes) == 20
    # fq_kv_batch_extend's arguments without seq_hint and the workspace pair
    _, ext = _lib.SYMBOLS["fq_kv_batch_extend"]
    assert argtypes == ext[:19] + ext[22:]
    header = open(os.path.join(ROOT, "include", "fqhip.h")).read()
    m = re.search(r"\bint\s+fq_kv_chunk_extend\s*\(([^)]*)\)\s*;", header)
    assert m, "not declared in include/fqhip.h"
    assert len(m.group(1).split(",")) == 20
    assert "seq_hint" not in m.group(1) and "workspace" not in m.group(1)
    assert hasattr(_lib.lib, "fq_kv_chunk_extend")


def test_argument_checks_return_before_any_launch():
    from flatquant_amd._lib import FQ_EINVAL, FQ_EUNSUPPORTED, lib
    vp = 0x1000

    def call(f16=0, o=vp, q=vp, qt=None, data=vp, param=vp, indptr=vp, indices=vp, last=vp, layers=2, layer=1, heads=8, q_group=4, copies=1,
             q_len=64, page=16, hd=128, batch=1):
        return lib.fq_kv_chunk_extend(f16, o, q, qt, 0, data, param, indptr, indices, last, layers, layer, heads, q_group, copies, q_len, page, hd,
                                      batch, None)
    assert call(q_len=0) == FQ_EINVAL and b"q_len" in lib.fq_last_error()
    assert call(q_len=-3) == FQ_EINVAL
    assert call(q_group=4, copies=3) == FQ_EINVAL and b"copies" in lib.fq_last_error()       # copies does not divide q_group
    assert call(heads=6, q_group=4, copies=4) == FQ_EINVAL                                    # ... nor the cache heads
    assert call(heads=16, q_group=16, copies=16) == FQ_EINVAL                                 # copies > 8
    assert call(layer=2) == FQ_EINVAL and call(layer=-1) == FQ_EINVAL                         # layer index
    assert call(hd=64) == FQ_EUNSUPPORTED and b"head_dim" in lib.fq_last_error()
    assert call(hd=96) == FQ_EUNSUPPORTED
    for g in (3, 5, 6, 7, 16):
        assert call(q_group=g) == FQ_EUNSUPPORTED, g
        assert b"q_group" in lib.fq_last_error()
    assert call(q_group=0) == FQ_EINVAL
    assert call(batch=0) == FQ_EINVAL and call(page=0) == FQ_EINVAL
    for name in ("o", "q", "data", "indptr", "indices", "last"):
        assert call(**{name: None}) == FQ_EINVAL, name
    assert call(param=None) == FQ_EINVAL and b"NULL" in lib.fq_last_error()                   # INT4 pages need their parameters
    for name in ("o", "q", "qt", "data"):
        assert call(**{name: 0x1008}) == FQ_EINVAL, name
        assert b"16-byte aligned" in lib.fq_last_error(), name


def test_new_kernels_do_not_spill_and_two_workgroups_share_a_cu():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import parse
    res = {k: r for k, r in parse().items() if r["file"] == "fq_kv_chunk_extend"}
    if not res:
        pytest.skip("no build/fq_kv_chunk_extend.res next to the sources (library built elsewhere)")
    assert set(res) == {f"fq_kv_chunk_extend_kernel<{qt},{f16}>" for qt in (0, 1) for f16 in (0, 1)}, sorted(res)
    for name, r in res.items():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        # the two-deep ring of 64-row K / V tiles (and their parameters) is a static array: two four-wave workgroups in a CU's 160 KB of LDS,
        # at the two waves per SIMD of __launch_bounds__(256, 2)
        assert 0 < r["lds"] and 2 * r["lds"] <= 160 * 1024, (name, r)
        assert r["occupancy"] >= 2, (name, r)


def test_routing_constant_is_none_or_at_least_64():
    from flatquant_amd.deploy.transformers import kv_cache
    c = kv_cache.EXTEND_CHUNK_MIN_TOKENS
    assert c is None or (isinstance(c, int) and c >= 64), c
    from flatquant_amd import ops
    assert ops.kv_chunk_extend_supported(4, 128) and ops.kv_chunk_extend_supported(1, 128) and ops.kv_chunk_extend_supported(8, 128)
    assert not ops.kv_chunk_extend_supported(3, 128) and not ops.kv_chunk_extend_supported(4, 64) and not ops.kv_chunk_extend_supported(0, 128)
