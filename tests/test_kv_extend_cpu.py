"""fq_kv_batch_extend's argument checks (several new tokens per request over the paged KV cache, round 7): they return before any HIP call,
so they hold on a machine without a GPU."""
import ctypes


def test_kv_extend_argument_validation_without_gpu():
    from flatquant_amd._lib import FQ_EINVAL, FQ_EUNSUPPORTED, lib
    vp = ctypes.c_void_p(4096)

    def call(q_len=4, q_group=4, copies=1, heads=8, head_dim=128, batch=1, layers=1, layer=0):
        return lib.fq_kv_batch_extend(0, vp, vp, None, 0, vp, vp, vp, vp, vp, layers, layer, heads, q_group, copies, q_len, 16, head_dim,
                                      batch, 0, None, 0, None)
    assert call(q_len=0) == FQ_EINVAL and b"q_len" in lib.fq_last_error()
    assert call(q_len=-3) == FQ_EINVAL
    assert call(q_group=3, copies=2) == FQ_EINVAL          # copies must divide q_group
    assert call(q_group=4, copies=4, heads=6) == FQ_EINVAL  # ... and the cache heads
    assert call(copies=9, q_group=9) == FQ_EINVAL
    assert call(layer=1) == FQ_EINVAL
    assert call(head_dim=64) == FQ_EUNSUPPORTED
    assert call(head_dim=96) == FQ_EUNSUPPORTED
    assert lib.fq_kv_extend_workspace_bytes(1, 32, 0, 128) < 0
    assert lib.fq_kv_extend_workspace_bytes(64, 32, 4, 128) == 0            # 512 workgroups: never split
    assert lib.fq_kv_extend_workspace_bytes(1, 32, 4, 128) >= 256 * 16 * 130 * 4
