"""Edge rows through every KV-cache quantiser, bit for bit with the oracle (builders: tests/kv_edge_rows.py; their own checks and the cap on what is
masked here: tests/test_kv_edge_rows_cpu.py).

The three launches that write what every attention launch reads — fq_kv_quant_f16 (ops.kv_quant), fq_kv_quant_append_i4 (ops.kv_quant_append) and
the prologue of fq_kv_decode_append[_rope]_i4 (ops.kv_decode_append) — get the same hand-built rows: all-zero, single-signed, one-hot, outliers,
subnormals, ranges under / at / just above the 1e-5 floor (where the fp16 scale is subnormal and the row's maximum rints to 16), .5 ties, one-ulp
ranges at a large offset, ranges at the top of fp16 and beyond it; every fp16 value between two extrema (the sweeps); the extrema in every pair of
places the kernels reduce separately. Every comparison is np.array_equal on bytes and on fp16 BIT PATTERNS against oracle.fq_oracle.kv_asym_quant /
kv_asym_dequant. The only digits not compared are the UNPINNED ones (the oracle's value before its clip is NaN: 0 / 0 or Inf / Inf), and the only
parameters not compared are NaN zero points; test_kv_edge_rows_cpu.py caps both (lac off: at most 2 digits of the batch, 3 through the
transform; lac: the rows whose scale underflows to 0)."""
import numpy as np
import pytest
import torch

from oracle import fq_oracle as O
from tests import kv_edge_rows as K

pytestmark = pytest.mark.gpu
MODES = [(False, (1.0, 1.0))] + [(True, c) for c in K.CLIPS]
APPEND_CLIP = K.APPEND_CLIP


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the shared oracle cases are read-only)


def bits16(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def u16(a):
    return np.ascontiguousarray(a).view(np.uint16)


def nibbles(p):
    p = np.asarray(p, np.uint8)
    return np.stack((p & 15, p >> 4), axis=-1).reshape(*p.shape[:-1], p.shape[-1] * 2)


def assert_rows(q, pbits, ref, idx, what):
    """packed rows q [n, hd / 2] uint8 and their (scale, zero) bit patterns pbits [n, 2] uint16 against rows idx of an oracle case"""
    idx = np.asarray(idx)
    keep = ~ref["mask"][idx]
    got = nibbles(q)
    assert np.array_equal(got[keep], ref["q"][idx][keep]), (what, "digits", np.argwhere((got != ref["q"][idx]) & keep)[:8].tolist())
    assert np.array_equal(pbits[:, 0], u16(ref["scale"])[idx]), (what, "scale", np.nonzero(pbits[:, 0] != u16(ref["scale"])[idx])[0][:8].tolist())
    zok = ~np.isnan(ref["zero"][idx])
    assert np.array_equal(pbits[zok, 1], u16(ref["zero"])[idx][zok]), (what, "zero", np.nonzero((pbits[:, 1] != u16(ref["zero"])[idx]) & zok)[0][:8].tolist())


def assert_f16(got_bits, want, what, keep=None):
    """fp16 bit patterns equal where the reference is a number, NaN where it is NaN (`keep`: the elements compared at all)"""
    want = np.asarray(want, np.float16)
    nan = np.isnan(want)
    keep = np.ones(want.shape, bool) if keep is None else keep
    assert np.array_equal(got_bits[keep & ~nan], u16(want)[keep & ~nan]), what
    assert np.isnan(got_bits.view(np.float16)[keep & nan]).all(), (what, "NaN")


def run_dense(ops, x, T, clip, lac):
    """-> (q uint8 [rows, hd / 2], params as bits [rows, 2], y bits or None) of ops.kv_quant"""
    out = ops.kv_quant(dev(x), None if T is None else dev(T), clip, lac, return_transformed=T is not None)
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), bits16(out[1]), (bits16(out[2]) if T is not None else None)


# ---------------------------------------------------------------- dense launch ----------------------------------------------------------------
@pytest.mark.parametrize("lac,clip", MODES)
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
def test_dense_batch_equals_the_oracle(ops, hd, trans, lac, clip):
    ref = K.reference(hd, trans, clip, lac)
    T = K.exact_trans(hd) if trans else None
    q, pb, yb = run_dense(ops, ref["x"], T, clip, lac)
    assert_rows(q, pb, ref, np.arange(K.N_BATCH), ("dense", hd, trans, lac, clip))
    if trans:
        assert np.array_equal(yb, u16(K.exact_product(ref["x"], T))), "return_transformed"
    # the de-quantiser on the ORACLE's bytes and parameters (its output does not depend on what the quantiser above did)
    prm = np.stack((ref["scale"], ref["zero"]), axis=-1)
    deq = ops.kv_dequant(dev(ref["packed"]), dev(prm), lac)
    assert_f16(bits16(deq), ref["deq"], ("dequant", hd, trans, lac, clip))


@pytest.mark.parametrize("lac,clip", [(False, (1.0, 1.0)), (True, (0.9, 0.8))])
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
def test_dense_rows_do_not_depend_on_their_place_or_neighbours(ops, hd, trans, lac, clip):
    """the batch rolled by 1 and by 31 rows; tiled beyond n_cu * FQ_KV_OCC (2) * 128 rows with a ragged last tile (the grid-stride loop and its
    prefetch of the next tile run, a wave takes an ordinary row's tile after an edge row's); with NaN rows among the neighbours: every other
    row's bytes and parameters are those of the plain launch (which test_dense_batch_equals_the_oracle holds to the oracle)"""
    ref = K.reference(hd, trans, clip, lac)
    T = K.exact_trans(hd) if trans else None
    x = ref["x"]
    q0, p0, y0 = run_dense(ops, x, T, clip, lac)
    assert_rows(q0, p0, ref, np.arange(K.N_BATCH), "plain")
    for sh in (1, 31):
        q, p, y = run_dense(ops, np.roll(x, sh, axis=0), T, clip, lac)
        assert np.array_equal(q, np.roll(q0, sh, axis=0)) and np.array_equal(p, np.roll(p0, sh, axis=0)), ("rolled", sh)
        assert y0 is None or np.array_equal(y, np.roll(y0, sh, axis=0))
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rows = n_cu * 2 * 128 + 3 * K.N_BATCH
    rows += 1 if rows % 32 == 0 else 0
    idx = np.arange(rows) % K.N_BATCH
    q, p, y = run_dense(ops, x[idx], T, clip, lac)
    assert rows % 32 != 0 and np.array_equal(q, q0[idx]) and np.array_equal(p, p0[idx]), "tiled"
    assert y0 is None or np.array_equal(y, y0[idx])
    bad = x.copy()
    nan_rows = np.arange(0, K.N_BATCH, 4)                  # ordinary rows: every second neighbour of an edge row
    bad[nan_rows] = np.nan
    rest = np.setdiff1d(np.arange(K.N_BATCH), nan_rows)
    q, p, y = run_dense(ops, bad, T, clip, lac)
    assert np.array_equal(q[rest], q0[rest]) and np.array_equal(p[rest], p0[rest]), "NaN neighbours"
    assert y0 is None or np.array_equal(y[rest], y0[rest])


@pytest.mark.parametrize("lac,clip", [(False, (1.0, 1.0)), (True, (0.9, 0.8))])
def test_dense_sweep_of_every_fp16_value_between_the_extrema(ops, lac, clip):
    """every representable x at a fixed (scale, zero): the quotient RN16((x + zero) / scale) from three fmas on v_rcp_f32 and the magic-add rint
    against the oracle's division and rint, ~240k values over scale 1, odd scales, subnormal scales, the floor, the top of the format"""
    ref = K.reference(128, False, clip, lac, "sweep")
    assert not ref["mask"].any()
    q, pb, _ = run_dense(ops, ref["x"], None, clip, lac)
    assert_rows(q, pb, ref, np.arange(len(ref["x"])), ("sweep", lac))


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
def test_dense_extrema_in_every_pair_of_places(ops, hd, trans):
    ref = K.reference(hd, trans, (1.0, 1.0), False, "extrema")
    assert not ref["mask"].any()
    q, pb, _ = run_dense(ops, ref["x"], K.exact_trans(hd) if trans else None, (1.0, 1.0), False)
    assert_rows(q, pb, ref, np.arange(len(ref["x"])), ("extrema", hd, trans))


# ---------------------------------------------------------------- paged caches ----------------------------------------------------------------
def make_cache(seed, lens, cache_heads, page, hd, layers=2):
    """a pre-filled cache whose request b holds lens[b] rows (the new ones included), pages scattered; finite parameters everywhere"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n_pg = [(n + page - 1) // page for n in lens]
    tot = sum(n_pg) + 1                                      # (one page no request owns)
    data = torch.randint(0, 256, (tot, layers, 2, cache_heads, page, hd // 2), generator=g, device="cuda", dtype=torch.uint8)
    param = torch.stack([torch.rand(tot, layers, 2, cache_heads, page, generator=g, device="cuda") * 0.3 + 0.02,
                         torch.rand(tot, layers, 2, cache_heads, page, generator=g, device="cuda") * 2.0 + 0.1], dim=-1).half()
    indptr = torch.tensor(np.concatenate(([0], np.cumsum(n_pg))), dtype=torch.int32, device="cuda")
    indices = torch.randperm(tot, generator=g, device="cuda")[:sum(n_pg)].to(torch.int32).contiguous()
    last = torch.tensor([(n - 1) % page + 1 for n in lens], dtype=torch.int32, device="cuda")
    return data, param, indptr, indices, last


def expected_cache(data, param, indptr, indices, lens, page, layer, added, src_heads, group, kref, kidx, vref, vidx):
    """the pre-filled cache with the oracle's rows where the launch appends them (flat source row (b * added + j) * src_heads + hs -> rows kidx[.] /
    vidx[.] of the oracle cases kref / vref, every one of `group` copies) -> (bytes, care mask per byte, parameter bits, care mask per parameter)"""
    exp, expp = data.cpu().numpy().copy(), bits16(param).copy()
    care, carep = np.full(exp.shape, 0xFF, np.uint8), np.ones(expp.shape, bool)
    ip, ind = indptr.cpu().numpy(), indices.cpu().numpy()
    for b, n in enumerate(lens):
        for j in range(added):
            pos = n - added + j
            pg, entry = ind[ip[b] + pos // page], pos % page
            for hs in range(src_heads):
                r = (b * added + j) * src_heads + hs
                for which, ref, idx in ((0, kref, kidx[r]), (1, vref, vidx[r])):
                    m = ~ref["mask"][idx]
                    cm = (m[0::2] * 0x0F + m[1::2] * 0xF0).astype(np.uint8)
                    for c in range(group):
                        h = hs * group + c
                        exp[pg, layer, which, h, entry] = ref["packed"][idx]
                        care[pg, layer, which, h, entry] = cm
                        expp[pg, layer, which, h, entry] = (u16(ref["scale"])[idx], u16(ref["zero"])[idx])
                        carep[pg, layer, which, h, entry, 1] = not np.isnan(ref["zero"][idx])
    return exp, care, expp, carep


def assert_cache(data, param, expected, what):
    exp, care, expp, carep = expected
    got, gotp = data.cpu().numpy(), bits16(param)
    bad = (got & care) != (exp & care)
    assert not bad.any(), (what, "bytes", np.argwhere(bad)[:6].tolist())
    badp = (gotp != expp) & carep
    assert not badp.any(), (what, "parameters", np.argwhere(badp)[:6].tolist())


@pytest.mark.parametrize("lac", [False, True])
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("src_heads,group", [(1, 1), (2, 4), (1, 8), (2, 1), (1, 4)])
@pytest.mark.parametrize("hd", [128, 64])
def test_paged_append_writes_the_oracle_rows_and_nothing_else(ops, hd, src_heads, group, trans, lac):
    """ops.kv_quant_append with the batch as K and the batch reversed as V (both `which` branches see every row): for every copy the page bytes and
    parameters of each appended row are the oracle's, every other byte of the pre-filled cache is unchanged"""
    n = K.N_BATCH - 1                                        # 48 rows: every edge row, and its neighbours
    bsz, page, layer = 4, 16, 1
    added = n // (bsz * src_heads)
    lens = [added, 17 + added, 33, 40]
    kclip, vclip = (APPEND_CLIP[:2], APPEND_CLIP[2:]) if lac else ((1.0, 1.0), (1.0, 1.0))
    kref, vref = K.reference(hd, trans, kclip, lac), K.reference(hd, False, vclip, lac)
    kidx, vidx = np.arange(n), np.arange(n)[::-1]
    data, param, indptr, indices, last = make_cache(hd + src_heads * 10 + group, lens, src_heads * group, page, hd)
    exp = expected_cache(data, param, indptr, indices, lens, page, layer, added, src_heads, group, kref, kidx, vref, vidx)
    k = dev(kref["x"][kidx]).view(bsz, added, src_heads, hd)
    v = dev(vref["x"][vidx]).view(bsz, added, src_heads, hd)
    ops.kv_quant_append(k, v, dev(K.exact_trans(hd)) if trans else None, data, param, indptr, indices, last, layer, group,
                        clip=APPEND_CLIP if lac else None, lac=lac)
    torch.cuda.synchronize()
    assert_cache(data, param, exp, ("append", hd, src_heads, group, trans, lac))


_decode_rows = {}


def decode_rows():
    """the rows of the decode-prologue test: one request per edge row and per extrema row (head_dim 128) -> the oracle cases {trans: ...} over
    the stacked rows, computed once"""
    if not _decode_rows:
        x = np.concatenate([K.edge_rows(128), K.extrema_rows(128)])
        for trans in (False, True):
            y = O.kv_transform(x, K.exact_trans(128)) if trans else x
            packed, scale, zero, q8 = O.kv_asym_quant(y)
            _decode_rows[trans] = {"x": x, "packed": packed, "scale": scale[:, 0], "zero": zero[:, 0], "q": q8, "mask": K.unpinned(y)}
            assert _decode_rows[trans]["mask"].sum() <= 3    # (test_kv_edge_rows_cpu.py: the +-40000 row, through the transform the 65504 row)
    return _decode_rows


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("route", ["plain", "trans", "rope", "rope_trans"])
@pytest.mark.parametrize("cache_heads,one_copy", [(1, False), (4, False), (4, True)])
def test_decode_prologue_appends_the_oracle_row(ops, cache_heads, one_copy, route, split):
    """ops.kv_decode_append, one request per row, src_heads 1 on 1 and 4 cache heads (every copy is written; `one_copy`: the launch that reads the
    first copy of the replicated layout), caches of 17 .. 40 rows in pages of 16: the extrema are merged across four waves and two half-waves.
    route: no transform, exact_trans (the fragment image), an identity rotary embedding (cos 1, sin 0: the row goes through s_krot), both.
    The new row's bytes and parameters in every copy are the oracle's, the rest of the cache is untouched, and for every request whose new rows
    have finite parameters the attention output equals ops.kv_quant_append + ops.kv_batch_decode by raw bits."""
    trans = route in ("trans", "rope_trans")
    kref, vref = decode_rows()[trans], decode_rows()[False]
    n, hd, page, layer = len(kref["x"]), 128, 16, 1
    lens = [17 + (5 * b) % 24 for b in range(n)]
    assert min(lens) == 17 and max(lens) == 40
    kidx, vidx = np.arange(n), np.arange(n)[::-1]
    data, param, indptr, indices, last = make_cache(7 * cache_heads + one_copy, lens, cache_heads, page, hd)
    if one_copy:                                            # the replicated layout: the copies of a KV head are identical
        data, param = data[:, :, :, :1].expand_as(data).contiguous(), param[:, :, :, :1].expand_as(param).contiguous()
    exp = expected_cache(data, param, indptr, indices, lens, page, layer, 1, 1, cache_heads, kref, kidx, vref, vidx)
    g = torch.Generator(device="cuda").manual_seed(11)
    q = (torch.randn(n, cache_heads, hd, generator=g, device="cuda") * 0.5).half()
    k, v = dev(kref["x"][kidx]).view(n, 1, hd), dev(vref["x"][vidx]).view(n, 1, hd)
    T = dev(K.exact_trans(hd)) if trans else None
    rope = (torch.ones(n, hd, dtype=torch.float16, device="cuda"), torch.zeros(n, hd, dtype=torch.float16, device="cuda")) if route.startswith("rope") else None
    d1, p1 = data.clone(), param.clone()
    ops.kv_quant_append(k.view(n, 1, 1, hd), v.view(n, 1, 1, hd), T, d1, p1, indptr, indices, last, layer, cache_heads)
    o1 = ops.kv_batch_decode(q, d1, p1, indptr, indices, last, layer, seq_hint=max(lens), split=split, **({"kv_copies": cache_heads} if one_copy else {}))
    d2, p2 = data.clone(), param.clone()
    o2 = ops.kv_decode_append(q, k, v, T, d2, p2, indptr, indices, last, layer, seq_hint=max(lens), split=split, read_one_copy=one_copy, rope=rope)
    torch.cuda.synchronize()
    what = ("decode", cache_heads, one_copy, route, split)
    assert_cache(d2, p2, exp, what)
    assert_cache(d1, p1, exp, what + ("two launches",))
    finite = np.array([np.isfinite([kref["scale"][kidx[b]], kref["zero"][kidx[b]], vref["scale"][vidx[b]], vref["zero"][vidx[b]]]).all() for b in range(n)])
    assert finite.sum() >= n - 4
    assert np.array_equal(bits16(o2)[finite], bits16(o1)[finite]), what + ("attention output",)
    assert np.isfinite(o2.float().cpu().numpy()[finite]).all()


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("trans", ["none", "matmul"])
def test_cache_class_pages_hold_the_oracle_rows(ops, trans, fuse):
    """MultiLayerPagedKVCache4Bit: the edge batch as a prompt, as the rows of one multi-token step and of one decode step (fuse: appended by the
    decode launch when the closure is called; otherwise by the append launch): the rows found in the pages equal the oracle's"""
    import flatquant_amd.deploy.transformers as dt
    bsz = heads = 7                                          # 49 (request, head) rows per token
    hd, page, layer = 128, 16, 0
    tr = trans == "matmul"
    ref, vref = K.reference(hd, tr, (1.0, 1.0), False), K.reference(hd, False, (1.0, 1.0), False)
    T = dev(K.exact_trans(hd))
    kw = {"trans_matrix_k": T, "trans_matrix_k_inv_t": T}
    c = dt.MultiLayerPagedKVCache4Bit(bsz, page, 32, torch.device("cuda"), 1, heads, hd, trans=trans, fuse_append=fuse)
    c.pages.zero_(), c.scales.zero_()
    n = K.N_BATCH
    steps = [(1, np.arange(n)), (2, np.concatenate([np.arange(n), np.arange(n)[::-1]])), (1, np.roll(np.arange(n), 5))]
    pos0 = 0
    for si, (added, order) in enumerate(steps):
        # flat source row (b * added + j) * heads + h holds batch row order[.] as K and order[::-1][.] as V
        kidx, vidx = order, order[::-1]
        k = dev(ref["x"][kidx]).view(bsz, added, heads, hd)
        v = dev(vref["x"][vidx]).view(bsz, added, heads, hd)
        out = c.update(k, v, layer, dict(kw))
        if si == 2:
            g = torch.Generator(device="cuda").manual_seed(3)
            o = out((torch.randn(bsz, 1, heads, hd, generator=g, device="cuda") * 0.5).half())
            assert o.shape == (bsz, 1, heads, hd)
        torch.cuda.synchronize()
        sp = c._specs
        data, prm = sp["kv_data"].cpu().numpy(), bits16(sp["kv_param"])
        ip, ind = sp["kv_indptr"].cpu().numpy(), sp["kv_indices"].cpu().numpy()
        for which, rf, idx in ((0, ref, kidx), (1, vref, vidx)):
            rows_q = np.empty((bsz * added * heads, hd // 2), np.uint8)
            rows_p = np.empty((bsz * added * heads, 2), np.uint16)
            for b in range(bsz):
                for j in range(added):
                    pos = pos0 + j
                    pg, entry = ind[ip[b] + pos // page], pos % page
                    sl = slice((b * added + j) * heads, (b * added + j + 1) * heads)
                    rows_q[sl], rows_p[sl] = data[pg, layer, which, :, entry], prm[pg, layer, which, :, entry]
            assert_rows(rows_q, rows_p, rf, idx, ("cache class", trans, fuse, si, "KV"[which]))
        pos0 += added
    assert c.length == pos0 == 4


# ---------------------------------------------------------------- the torch-facing mirror ----------------------------------------------------------------
@pytest.mark.parametrize("lac,clip", MODES)
@pytest.mark.parametrize("hd", [64, 128])
def test_mirror_functions_equal_the_oracle(ops, hd, lac, clip):
    """deploy.transformers.asym_quantize_and_pack_i4 / unpack_i4_and_asym_dequantize on the batch, quantize=False included"""
    import flatquant_amd.deploy.transformers as dt
    ref = K.reference(hd, False, clip, lac)
    x = dev(ref["x"])
    q, scale, zero = dt.asym_quantize_and_pack_i4(x, clip[0], clip[1], lac)
    assert scale.shape == zero.shape == (K.N_BATCH, 1)
    assert_rows(q.cpu().numpy(), np.stack((bits16(scale)[:, 0], bits16(zero)[:, 0]), axis=-1), ref, np.arange(K.N_BATCH), ("mirror", hd, lac, clip))
    fq, scale2, zero2 = dt.asym_quantize_and_pack_i4(x, clip[0], clip[1], lac, quantize=False)
    want = O.kv_asym_dequant(ref["packed"], ref["scale"][:, None], ref["zero"][:, None], lac=True)     # scale * (q - zero) in either mode
    assert_f16(bits16(fq), want, ("mirror fake-quant", hd, lac, clip), keep=~ref["mask"])
    assert np.array_equal(bits16(scale2), bits16(scale))
    deq = dt.unpack_i4_and_asym_dequantize(dev(ref["packed"]), dev(ref["scale"][:, None]), dev(ref["zero"][:, None]), lac)
    assert_f16(bits16(deq), ref["deq"], ("mirror dequant", hd, lac, clip))
