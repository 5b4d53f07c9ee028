"""CPU side of the grouped INT4 GEMM: the reference helper itself (tests/gemm_grouped_ref.py) against an int64 product, and what the two
C entry points reject. Validation returns before any HIP call, so nothing here needs a GPU: the pointers are never dereferenced."""
import numpy as np
import pytest

from oracle import fq_oracle as O
from tests import gemm_grouped_ref as R

P = 4096       # a non-NULL, 16-byte aligned address
ODD = 4104     # 8- but not 16-byte aligned
ODD4 = 4100    # not 8-byte aligned
FQ_OK, FQ_EINVAL, FQ_EUNSUPPORTED = 0, -1, -2


def _problem(sizes, N, K, seed):
    rng = np.random.default_rng(seed)
    rows, G = int(sum(sizes)), len(sizes)
    xq = rng.integers(-8, 8, (rows, K), dtype=np.int32)
    wq = rng.integers(-8, 8, (G, N, K), dtype=np.int32)
    return xq, wq, O.pack_i4(xq), O.pack_i4(wq), R.offsets_of(sizes)


def test_helper_equals_int64_product():
    sizes = [0, 3, 1, 0, 5, 0]
    xq, wq, xp, wp, off = _problem(sizes, 6, 32, 1)
    c = R.grouped_int4_matmul_ref(xp, wp, off)
    assert c.shape == (9, 6) and c.dtype == np.int32
    for g in range(len(sizes)):
        b, e = off[g], off[g + 1]
        assert np.array_equal(c[b:e], (xq[b:e].astype(np.int64) @ wq[g].astype(np.int64).T).astype(np.int32))


def test_helper_empty_groups_contribute_nothing():
    xq, wq, xp, wp, off = _problem([3, 5], 4, 32, 2)
    wide = np.stack([wp[0] ^ 0x5A, wp[0], wp[0] ^ 0xFF, wp[1], wp[1] ^ 0x33])      # empty groups with other weights at the front, middle, end
    off_wide = R.offsets_of([0, 3, 0, 5, 0])
    assert np.array_equal(R.grouped_int4_matmul_ref(xp, wide, off_wide), R.grouped_int4_matmul_ref(xp, wp, off))
    rng = np.random.default_rng(3)
    sx = rng.random(8).astype(np.float16)
    sw = rng.random((2, 4)).astype(np.float16)
    sw_wide = np.stack([sw[0] * 3, sw[0], sw[1] * 5, sw[1], sw[0] * 7]).astype(np.float16)
    a = R.grouped_linear4bit_ref(xp, sx, wide, sw_wide, off_wide)
    b = R.grouped_linear4bit_ref(xp, sx, wp, sw, off)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
    assert R.grouped_int4_matmul_ref(xp[:0], wp, R.offsets_of([0, 0])).shape == (0, 4)


def test_helper_single_group_is_the_dense_oracle():
    xq, wq, xp, wp, off = _problem([7], 5, 64, 4)
    rng = np.random.default_rng(5)
    sx, sw, b = rng.random(7).astype(np.float16), rng.random((1, 5)).astype(np.float16), rng.standard_normal((1, 5)).astype(np.float16)
    assert np.array_equal(R.grouped_int4_matmul_ref(xp, wp, off), O.int4_matmul(xp, wp[0]))
    y = R.grouped_linear4bit_ref(xp, sx, wp, sw, off, b)
    assert np.array_equal(y.view(np.uint16), O.linear4bit(xp, sx, wp[0], sw[0], b[0]).view(np.uint16))


def test_g_sizes():
    assert sum(R.G_SIZES) == 1549 and len(R.G_SIZES) == 14 and R.offsets_of(R.G_SIZES)[-1] == 1549


# ---- the C ABI: (entry point, argument names in order, values that pass validation) ----
GEMM = ("fq_int4_gemm_grouped_i32",
        [("x", P), ("w_g", P), ("rows", 64), ("N", 32), ("K", 128), ("group_offsets", P), ("n_groups", 4), ("c", P), ("stream", None)])
LINEAR = ("fq_int4_linear_grouped_f16",
          [("x", P), ("x_scale", P), ("w_g", P), ("w_scale_g", P), ("bias_g", None), ("rows", 64), ("N", 32), ("K", 128), ("group_offsets", P),
           ("n_groups", 4), ("y", P), ("stream", None)])

_SIZES = "rows=%d N=%d K=%d n_groups=%d"
_ALIGN_G = "pointer argument %d of {x, w_g, c} is not 16-byte aligned"
_ALIGN_L = "pointer argument %d of {x, w_g, y, w_scale_g, bias_g} is not 16-byte aligned"
_BIG = "shape rows=64 N=32 K=33554432 not supported (K < 2^25, rows <= 2^30)"
# one fault per case: (changes, code, the text behind "<entry point>: ")
CASES = {
    GEMM[0]: [
        (dict(x=None), FQ_EINVAL, "NULL pointer"),
        (dict(w_g=None), FQ_EINVAL, "NULL pointer"),
        (dict(group_offsets=None), FQ_EINVAL, "NULL pointer"),
        (dict(c=None), FQ_EINVAL, "NULL pointer"),
        (dict(x=ODD), FQ_EINVAL, _ALIGN_G % 0),
        (dict(c=ODD), FQ_EINVAL, _ALIGN_G % 2),
        (dict(group_offsets=ODD4), FQ_EINVAL, "group_offsets is not 8-byte aligned"),
        (dict(rows=-1), FQ_EINVAL, "bad sizes " + _SIZES % (-1, 32, 128, 4)),
        (dict(N=0), FQ_EINVAL, "bad sizes " + _SIZES % (64, 0, 128, 4)),
        (dict(n_groups=0), FQ_EINVAL, "bad sizes " + _SIZES % (64, 32, 128, 0)),
        (dict(n_groups=1025), FQ_EUNSUPPORTED, "n_groups=1025 (at most 1024)"),
        (dict(K=48), FQ_EUNSUPPORTED, "K=48 must be a multiple of 32"),
        (dict(K=1 << 25), FQ_EUNSUPPORTED, _BIG),
    ],
    LINEAR[0]: [
        (dict(x=None), FQ_EINVAL, "NULL pointer"),
        (dict(x_scale=None), FQ_EINVAL, "NULL pointer"),
        (dict(w_g=None), FQ_EINVAL, "NULL pointer"),
        (dict(w_scale_g=None), FQ_EINVAL, "NULL pointer"),
        (dict(group_offsets=None), FQ_EINVAL, "NULL pointer"),
        (dict(y=None), FQ_EINVAL, "NULL pointer"),
        (dict(w_g=ODD), FQ_EINVAL, _ALIGN_L % 1),
        (dict(y=ODD), FQ_EINVAL, _ALIGN_L % 2),
        (dict(w_scale_g=ODD), FQ_EINVAL, _ALIGN_L % 3),
        (dict(bias_g=ODD), FQ_EINVAL, _ALIGN_L % 4),
        (dict(group_offsets=ODD4), FQ_EINVAL, "group_offsets is not 8-byte aligned"),
        (dict(rows=-1), FQ_EINVAL, "bad sizes " + _SIZES % (-1, 32, 128, 4)),
        (dict(N=0), FQ_EINVAL, "bad sizes " + _SIZES % (64, 0, 128, 4)),
        (dict(n_groups=0), FQ_EINVAL, "bad sizes " + _SIZES % (64, 32, 128, 0)),
        (dict(n_groups=1025), FQ_EUNSUPPORTED, "n_groups=1025 (at most 1024)"),
        (dict(K=48), FQ_EUNSUPPORTED, "K=48 must be a multiple of 32"),
        (dict(K=1 << 25), FQ_EUNSUPPORTED, _BIG),
    ],
}


def _call(lib, entry, changes):
    name, args = entry
    vals = dict(args)
    assert all(k in vals for k in changes)
    vals.update(changes)
    return getattr(lib, name)(*[vals[n] for n, _ in args])


@pytest.mark.parametrize("entry", [GEMM, LINEAR], ids=lambda e: e[0])
def test_rejections(entry):
    from flatquant_amd._lib import lib
    for changes, code, text in CASES[entry[0]]:
        got = _call(lib, entry, changes)
        assert (got, lib.fq_last_error().decode()) == (code, f"{entry[0]}: {text}"), changes


@pytest.mark.parametrize("entry", [GEMM, LINEAR], ids=lambda e: e[0])
def test_zero_rows_is_ok_without_a_launch(entry):
    from flatquant_amd._lib import lib
    assert _call(lib, entry, dict(rows=0)) == FQ_OK
    assert _call(lib, entry, dict(rows=0, n_groups=1024, K=96, N=5)) == FQ_OK


def test_version():
    from flatquant_amd._lib import lib
    assert lib.fq_version() >= 121
