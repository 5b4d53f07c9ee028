"""Rotary position embedding on the layout the attention here uses (deploy/transformers/modeling_llama.py:105)."""
import torch

from ... import ops


def apply_rotary_pos_emb(q, k, cos, sin, position_ids=None, unsqueeze_dim=2):
    """Drop-in for transformers' ``apply_rotary_pos_emb(q, k, cos, sin, position_ids, unsqueeze_dim=2)`` on fp16 tensors: q [bsz, seq, heads,
    head_dim], k [bsz, seq, kv_heads, head_dim], cos / sin [bsz, seq, head_dim] (or [1, seq, head_dim], broadcast over the requests) ->
    (q_embed, k_embed), bit-identical to ``(x * cos.unsqueeze(2)) + (rotate_half(x) * sin.unsqueeze(2))`` — ONE launch (ops.rope) instead of
    about ten. ``position_ids`` is ignored, as in transformers since 4.38 (cos / sin are already gathered). Only ``unsqueeze_dim=2`` (heads in
    dimension 2) is the layout of this package's attention; the [bsz, heads, seq, head_dim] layout (``unsqueeze_dim=1``) is refused."""
    if unsqueeze_dim != 2:
        raise NotImplementedError("apply_rotary_pos_emb: only unsqueeze_dim=2 (q / k as [bsz, seq, heads, head_dim])")
    if q.dim() != 4 or k.dim() != 4 or q.shape[:2] != k.shape[:2] or q.shape[-1] != k.shape[-1]:
        raise ValueError(f"apply_rotary_pos_emb: q / k must be [bsz, seq, heads, head_dim], got {tuple(q.shape)} and {tuple(k.shape)}")
    bsz, seq, _, hd = q.shape
    tables = []
    for t in (cos, sin):
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if t.dim() != 3 or t.shape[1:] != (seq, hd) or t.shape[0] not in (1, bsz):
            raise ValueError(f"apply_rotary_pos_emb: cos / sin must be [bsz or 1, seq, head_dim], got {tuple(t.shape)}")
        tables.append(t.to(torch.float16).expand(bsz, seq, hd).contiguous())
    return ops.rope(q.contiguous(), k.contiguous(), tables[0], tables[1])
