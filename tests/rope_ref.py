"""Rotary position embedding on the CPU, restated rounding by rounding (a helper of tests/test_rope_cpu.py and tests/test_gpu_rope.py).

transformers' ``apply_rotary_pos_emb`` on fp16 tensors is ``(x * cos) + (rotate_half(x) * sin)``: two fp16 products and one fp16 sum, each
rounded to nearest even. The restatement goes through fp32, three times: a product of two fp16 values has 22 significant bits and is exact
in fp32; a sum of two fp16 values is exact in fp32 while their exponents are at most 13 apart (11 + 13 = 24 bits), and beyond that the smaller
one is below a quarter of the larger one's fp16 ulp, so rounding the fp32 sum to fp16 gives the larger one, as the fp16 addition does."""
import torch


def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def rope_ref(x, cos, sin):
    """x [..., heads, head_dim] fp16, cos / sin [..., head_dim] fp16 (one row per token) -> fp16, three roundings"""
    assert x.dtype == cos.dtype == sin.dtype == torch.float16
    c, s = cos.unsqueeze(-2).float(), sin.unsqueeze(-2).float()
    a = (x.float() * c).half()
    b = (rotate_half(x).float() * s).half()
    return (a.float() + b.float()).half()


def rope_torch(x, cos, sin):
    """the expression itself, on whatever device the tensors live"""
    return (x * cos.unsqueeze(-2)) + (rotate_half(x) * sin.unsqueeze(-2))


def rope_single_rounding(x, cos, sin):
    """what a fused multiply-add chain would give: the exact value, rounded once (not the contract; tests hold the two apart)"""
    c, s = cos.unsqueeze(-2).double(), sin.unsqueeze(-2).double()
    return (x.double() * c + rotate_half(x).double() * s).float().half()


def llama3_tables(positions, head_dim=128, theta=5e5):
    """cos / sin [len(positions), head_dim] fp16 of the unscaled Llama-3 frequencies, computed in fp32 and rounded like transformers does"""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    f = positions.float()[:, None] * inv[None, :]
    emb = torch.cat((f, f), dim=-1)
    return emb.cos().half(), emb.sin().half()
