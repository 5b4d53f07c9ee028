"""The prompt's attention core (deploy/transformers/modeling_llama.py:125-137): transformers' ``_flash_attention_forward`` for the one case the
reference uses it in — causal self-attention of a prompt over the un-quantised states the cache returns — as one launch of this library
(ops.prefill_attention, fq_prefill_attention_f16)."""
import torch

from ... import ops


def mask_ranges(mask):
    """A 0/1 ``attention_mask`` [bsz, seq] -> (seq_start, seq_len), int32 [bsz] on the mask's device: row b's ones are positions seq_start[b] ..
    seq_start[b] + seq_len[b] - 1. Left-padded, right-padded, full and all-zero rows (seq_len 0) are accepted; a row whose ones are not one
    contiguous run raises NotImplementedError. Reads the mask on the host (as the cache's masked prompt path does; a prompt call is never
    captured)."""
    if mask.dim() != 2:
        raise ValueError(f"attention_mask must be [bsz, seq], got {tuple(mask.shape)}")
    m = mask != 0
    bsz, seq = m.shape
    n = m.sum(dim=-1, dtype=torch.int64)
    pos = torch.arange(seq, device=m.device, dtype=torch.int64).expand(bsz, seq)
    first = torch.where(m, pos, torch.full_like(pos, seq)).amin(dim=-1) if seq else torch.zeros_like(n)
    last = torch.where(m, pos, torch.full_like(pos, -1)).amax(dim=-1) if seq else torch.full_like(n, -1)
    first = torch.where(n > 0, first, torch.zeros_like(first))
    if bool(((n > 0) & (last - first + 1 != n)).any()):
        raise NotImplementedError("attention_mask: a row's ones must be one contiguous run (left or right padding); masks with holes are not "
                                  "un-padded here")
    return first.to(torch.int32), n.to(torch.int32)


def flash_attention_forward(query_states, key_states, value_states, query_length, attention_mask=None, is_causal=True, q_trans=None):
    """Drop-in for the reference's ``_flash_attention_forward(query_states, key_states, value_states, query_length=q_len, attention_mask=..,
    is_causal=True)`` call: query_states [bsz, seq, heads, 128], key_states / value_states [bsz, seq, kv_heads, 128] -> [bsz, seq, heads, 128]
    fp16. ``q_trans`` (extension): the launch forms fp16(query_states . q_trans) itself (modeling_llama.py:127-129), so the caller's matmul goes.
    ``attention_mask`` [bsz, seq] of 0/1 becomes one valid range per request (mask_ranges); outputs at masked positions are zeros, as
    transformers' pad_input leaves them. transformers un-pads ARBITRARY masks; this takes left padding, right padding and empty rows only and
    raises NotImplementedError for a mask with a hole. Causal prompts only: ``is_causal=False`` or a query length that differs from the key
    length raises NotImplementedError (later pieces of a prompt go through the cache's closure, fq_kv_batch_extend)."""
    if not is_causal:
        raise NotImplementedError("flash_attention_forward: causal attention only")
    if query_states.dim() != 4 or key_states.dim() != 4:
        raise ValueError("flash_attention_forward: query / key states must be [bsz, seq, heads, head_dim]")
    if query_length != key_states.shape[1] or query_states.shape[1] != key_states.shape[1]:
        raise NotImplementedError(f"flash_attention_forward: query length {query_length} != key length {key_states.shape[1]} (a prompt attends "
                                  "itself; steps after it go through the cache's closure)")
    start = length = None
    if attention_mask is not None:
        if attention_mask.shape != key_states.shape[:2]:
            raise ValueError(f"attention_mask must be [bsz, seq] = {tuple(key_states.shape[:2])}, got {tuple(attention_mask.shape)}")
        start, length = (t.to(query_states.device) for t in mask_ranges(attention_mask))
    return ops.prefill_attention(query_states, key_states, value_states, q_trans, start, length)
