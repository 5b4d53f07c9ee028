"""The reference of the grouped INT4 GEMM / Linear4bit (fq_int4_gemm_grouped_i32, fq_int4_linear_grouped_f16): the loop of the dense
oracle (oracle/fq_oracle.py: int4_matmul, linear4bit) over the groups' row slices, concatenated. Nothing of the grouped code is in it."""
import numpy as np

from oracle import fq_oracle as O

# sizes below, at and one past every plausible tile height, empty groups at the front, middle and end, one group of more than a tile
G_SIZES = [0, 1, 31, 0, 32, 33, 127, 128, 129, 255, 256, 257, 300, 0]


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def _slices(offsets):
    off = np.asarray(offsets, dtype=np.int64)
    assert off.ndim == 1 and off[0] == 0 and np.all(np.diff(off) >= 0)
    return [(g, int(off[g]), int(off[g + 1])) for g in range(len(off) - 1)]


def grouped_int4_matmul_ref(xp, wp_g, offsets):
    """xp uint8 [rows, K/2], wp_g uint8 [G, N, K/2], offsets [G + 1] -> int32 [rows, N]"""
    xp, wp_g = np.asarray(xp, dtype=np.uint8), np.asarray(wp_g, dtype=np.uint8)
    assert offsets[-1] == xp.shape[0] and len(offsets) == wp_g.shape[0] + 1
    parts = [O.int4_matmul(xp[b:e], wp_g[g]) for g, b, e in _slices(offsets) if e > b]
    return np.concatenate(parts, axis=0) if parts else np.zeros((0, wp_g.shape[1]), dtype=np.int32)


def grouped_linear4bit_ref(xp, sx, wp_g, sw_g, offsets, bias_g=None):
    """... with x scales fp16 [rows], weight scales fp16 [G, N], optional bias fp16 [G, N] -> fp16 [rows, N]"""
    xp, wp_g = np.asarray(xp, dtype=np.uint8), np.asarray(wp_g, dtype=np.uint8)
    assert offsets[-1] == xp.shape[0] and len(offsets) == wp_g.shape[0] + 1
    parts = [O.linear4bit(xp[b:e], sx[b:e], wp_g[g], sw_g[g], None if bias_g is None else bias_g[g]) for g, b, e in _slices(offsets) if e > b]
    return np.concatenate(parts, axis=0) if parts else np.zeros((0, wp_g.shape[1]), dtype=np.float16)
