"""ops.kv_decode_append(had=True) between poisoned guard bands (tests/guards.py): the launch that rotates its queries and the new K row writes the
new token's rows and its output and nothing else, and reads q / k_new / v_new inside their bounds."""
import pytest
import torch

from tests import guards
from tests.test_gpu_bounds import IDX_PADS, addressed, drive, paged, rnd

pytestmark = pytest.mark.gpu
F16 = torch.float16


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == F16 and bool(torch.equal(a.view(torch.int16), b.view(torch.int16)))


@pytest.mark.parametrize("lens,cache_heads,src_heads,q_group,page,one_copy,split", [
    ([1, 300, 37], 4, 4, 1, 16, False, True),                 # a workgroup per query head, split; a one-row request
    ([700, 1, 33], 2, 2, 4, 32, False, True),                 # the shared layout, four query heads per cache head, split
    ([600, 1, 300, 520], 8, 8, 4, 16, False, True),           # 32 (request, KV head) pairs: one workgroup serves four query heads
    ([600, 1, 300, 520], 32, 8, 1, 16, True, True)])          # the replicated layout read one copy per group: every copy is written
@pytest.mark.parametrize("transpose_out", [False, True])
def test_had_launch_writes_one_row_and_its_output(ops, lens, cache_heads, src_heads, q_group, page, one_copy, split, transpose_out):
    """o and the cache equal the plain run's, the cache changes in the new token's rows and nowhere else and every byte of those is written,
    q / k_new / v_new (NaN-padded) are read inside their bounds and left as they were"""
    hd, layers, layer = 128, 2, 1
    data, param, indptr, indices, last, used = paged(lens, cache_heads, page, False, hd, layers)
    mask = addressed(used.shape, layers, cache_heads, indptr, indices, last, page, layer, [1] * len(lens))
    data[mask], param[mask] = 0xFF, float("nan")
    bsz = len(lens)
    q = rnd((bsz, cache_heads * q_group, hd), 1, F16, 0.5)
    kn, vn = rnd((bsz, src_heads, hd), 2), rnd((bsz, src_heads, hd), 3)
    before = {}

    def call(q, kn, vn, data, param, indptr, indices, last):
        before[data.data_ptr()] = (data, data.clone(), param, param.clone(), q, q.clone(), kn, kn.clone(), vn, vn.clone())
        return ops.kv_decode_append(q, kn, vn, None, data, param, indptr, indices, last, layer, None, transpose_out, seq_hint=max(lens), split=split,
                                    read_one_copy=one_copy, had=True)

    want, _, _ = drive(ops, call, dict(q=q, kn=kn, vn=vn, data=data, param=param, indptr=indptr, indices=indices, last=last),
                       pads=IDX_PADS, inout=("data", "param"))
    assert bool(torch.isfinite(want[0].float()).all()) and len(before) == 3
    for d1, d0, p1, p0, q1, q0, k1, k0, v1, v0 in before.values():
        assert torch.equal(d1[~mask], d0[~mask]) and guards.same_raw(p1[~mask], p0[~mask])
        # every addressed row was written: 64 bytes of 0xFF cannot come out of a quantiser whose row has a minimum, and no parameter is NaN any more
        assert not bool((d1[mask] == 0xFF).all(dim=-1).any()) and bool(torch.isfinite(p1[mask].float()).all())
        assert bits_equal(q1, q0) and bits_equal(k1, k0) and bits_equal(v1, v0)      # the launch rotates in LDS, never in the caller's tensors
    # the launches it replaces leave the same cache and the same output
    d2, p2 = data.clone(), param.clone()
    o2 = ops.kv_decode_append(ops.hadamard(q), ops.hadamard(kn), vn, None, d2, p2, indptr, indices, last, layer, None, transpose_out, seq_hint=max(lens),
                              split=split, read_one_copy=one_copy)
    assert bits_equal(o2, want[0]) and torch.equal(d2, want[1]) and guards.same_raw(p2, want[2])
    # ... and so every byte of the new rows is written: poisoned the other way round, the rows come out the same
    d3, p3 = data.clone(), param.clone()
    d3[mask], p3[mask] = 0x00, 0.0
    ops.kv_decode_append(q, kn, vn, None, d3, p3, indptr, indices, last, layer, None, transpose_out, seq_hint=max(lens), split=split,
                         read_one_copy=one_copy, had=True)
    assert torch.equal(d3, want[1]) and guards.same_raw(p3, want[2])
