"""The attention core of the reference's decoder layer (deploy/transformers/modeling_llama.py:125-139): what follows ``past_key_value.update``."""
import torch

from ..functional.attention import flash_attention_forward


def attention_core(cache_out, query_states, cache_kwargs=None):
    """``cache_out`` is what ``MultiLayerPagedKVCache4Bit.update`` returned. A tuple (the first call per layer: the un-quantised transformed
    keys and the values) runs the prompt launch on it — with ``q_trans = cache_kwargs["trans_matrix_k_inv_t"]`` inside the launch where the
    reference multiplies the queries by it (:127-129) and ``cache_kwargs["attention_mask"]`` as the reference passes it (:135); a closure
    (every later step) is called with the queries (:139). query_states [bsz, q_len, heads, head_dim] -> the attention output of that shape."""
    cache_kwargs = cache_kwargs or {}
    if isinstance(cache_out, tuple):
        key_states, value_states = cache_out
        q_trans = cache_kwargs.get("trans_matrix_k_inv_t")
        if q_trans is not None:
            q_trans = q_trans.to(torch.float16)
        return flash_attention_forward(query_states.to(torch.float16), key_states.to(torch.float16), value_states.to(torch.float16),
                                       query_length=query_states.shape[1], attention_mask=cache_kwargs.get("attention_mask"), is_causal=True,
                                       q_trans=q_trans)
    return cache_out(query_states)
