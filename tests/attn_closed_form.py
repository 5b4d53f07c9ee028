"""Attention inputs whose softmax is known exactly (fq_prefill_attention_f16, fq_kv_chunk_extend, fq_kv_batch_extend, fq_kv_batch_decode*,
fq_kv_decode_append*): shared builders, exact references and a NumPy model of the launches' arithmetic (numpy only; no GPU, no torch).
DESIGN 7.5 has the derivations.

A cached row j carries a LEVEL lev[j] and nothing else: the query is zero outside feature c, the key holds its level at feature c. One level is
16 * 128 * log2(e) / sqrt(head_dim) log2 units (261 at head_dim 128): more than fp32's 149 plus the decode launches' margin of 8, so exp2 of a
lower level against a higher one is exactly 0, rows of one level have bit-identical scores and weigh exactly the same. Token t attends the
MEAN of V over S(t), the visible rows at the highest visible level (`sets`, `exact`); the expectation is formed in fp64 from what `dense` reads
back out of the cache (INT4: the bytes, n * scale - zero).

`model` restates the launches' arithmetic (64-row tiles, an fp32 running reference with margin 0 or 8, fp16 weights with the factor 256, (scale,
zero) on the fp32 side) in a few lines that share nothing with the library; tests/test_attn_closed_form_cpu.py holds it to the same bounds
as the GPU file holds the launches."""
import math

import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64
FEATURES = {128: (0, 77, 127), 64: (0, 37, 63)}     # the one non-zero feature c: different K-steps and lane halves carry the score
K_SCALE, Q_I4, Q_F16, K_F16 = 16.0, 128.0, 16.0, 128.0   # INT4 keys: nibble lev, scale 16, q = 128 e_c; fp16 keys: 128 lev e_c, q = +-16 e_c
K_ZEROS = (0.0, 40.0)
GAP = 170.0                                          # log2 units that make a weight exactly 0: 149 (fp32's smallest) + 8 (margin) + slack
SINGLETON = ("sink", "staircase", "one_hot")


def level_step(hd=128):
    return K_SCALE * Q_I4 * math.log2(math.e) / math.sqrt(hd)


# ------------------------------------------------------------------------------------------------ level patterns: n -> lev[0 .. n)

def levels(pattern, n, rng=None, jstar=0):
    lev = np.zeros(n, np.int64)
    if pattern == "sink":
        lev[0] = 1
    elif pattern == "staircase":
        lev = np.arange(n, dtype=np.int64)
    elif pattern == "stairs16":
        lev = np.arange(n, dtype=np.int64) // -(-n // 16)
    elif pattern == "one_hot":
        lev[min(jstar, n - 1)] = 1
    elif pattern == "blocks":
        lev = rng.integers(0, 4, n)
    elif pattern != "uniform":
        raise ValueError(pattern)
    return lev


def one_hot_positions(n, count=64):
    """request b's j*: every position 0 .. 63 of a tile once, in the first, a middle and the last tile"""
    last = (n - 1) // 64
    out = []
    for b in range(count):
        tile = (0, max(last // 2, min(1, last)), last)[b % 3]
        j = 64 * tile + b
        out.append(j if j < n else 64 * (last - 1) + b if last else b % n)
    return out


def sets(eff, qlim):
    """eff[j]: a row's effective level (the query's sign times lev); qlim[t]: the last row token t sees -> bool [T, n], S(t)"""
    eff, qlim = np.asarray(eff), np.asarray(qlim)
    top = np.maximum.accumulate(eff)[qlim]
    return (np.arange(len(eff))[None, :] <= qlim[:, None]) & (eff[None, :] == top[:, None])


def exact(S, v64):
    """the mean of the fp64 rows v64 [n, hd] over each S(t) -> fp64 [T, hd]"""
    return (S.astype(F64) @ v64) / S.sum(1, keepdims=True)


def sets_from_scores(x64, visible):
    """S(t) from fp64 scores in log2 units [T, n]: the visible rows AT the maximum; every other visible row must lie GAP below it (asserted)"""
    xm = np.where(visible, x64, -np.inf)
    S = visible & (xm == xm.max(1, keepdims=True))
    rest = np.where(visible & ~S, xm, -np.inf)
    assert (rest.max(1) < xm.max(1) - GAP).all(), "a row outside S(t) is less than GAP below it"
    return S


# ------------------------------------------------------------------------------------------------ bounds

def bound3(e, c=0.0):
    """|o - e| <= 2^-11 (1 + 2^-9) |e| + 2^-25 + c: half an fp16 ulp, the fp32 product with 1 / l, half a subnormal step; c (INT4 pages):
    2^-22 max_{j in S} (8 s_j + |z_j|) — s (n - 8) and 8 s - z are formed separately in fp32 and e may cancel"""
    return 2.0 ** -11 * (1 + 2.0 ** -9) * np.abs(e) + 2.0 ** -25 + c


def c_term(S, s, z):
    """2^-22 max_{j in S(t)} (8 s_j + |z_j|) -> [T, 1]"""
    w = 8 * np.asarray(s, F64) + np.abs(np.asarray(z, F64))
    return 2.0 ** -22 * np.where(S, w[None, :], 0.0).max(1, keepdims=True)


def bound4(e, A, X, c):
    """risers: |o - e| <= 2^-11 |e| + (2^-10 + 2^-21 X) A + c; A = sum_j p_j (s_j |n_j - 8| + |8 s_j - z_j|) with fp64 weights, X = max |x| + 8:
    one fp16 rounding of each weight, score rounding through exp2, the output's own rounding"""
    return 2.0 ** -11 * np.abs(e) + (2.0 ** -10 + 2.0 ** -21 * X) * A + c


# ------------------------------------------------------------------------------------------------ payloads

V_SCALES = (0.125, 0.25, 1.0, 1.5)
END_F16 = (65504.0, -65504.0, 2.0 ** -14, 2.0 ** -24)
END_SCALES = (3 * 2.0 ** -24, 6.1e-5, 1.0, 255.0, 256.0, 1000.0, 4366.0)


def v_int(rng, n, hd):
    """fp16 V: integers in -8 .. 8 (every sum exact in fp32, a dropped key moves a mean by at least 1 / n); no -0.0"""
    return rng.integers(-8, 9, (n, hd)).astype(F16)


def v_ends_f16(rng, n, hd):
    """fp16 V rows at the ends of the format (singleton sets only): constant rows and mixtures of 65504, -65504, 2^-14, 2^-24"""
    v = np.empty((n, hd), F16)
    for j in range(n):
        v[j] = rng.choice(END_F16, hd) if j % 5 == 4 else END_F16[j % 4]
    if n:
        v[0] = rng.choice(END_F16, hd)
    return v


def v_i4(rng, n, hd):
    """INT4 V: random nibbles, dyadic parameters — scale in {1/8, 1/4, 1, 1.5}, zero a small multiple of the scale (4 .. 11: the values centre on 0, so a mean
    over thousands of rows is small against a single row and one dropped key shows) -> (nib, scale, zero)"""
    s = rng.choice(V_SCALES, n)
    return rng.integers(0, 16, (n, hd)), s.astype(F16), (s * rng.integers(4, 12, n)).astype(F16)


def end_pairs():
    """the (scale, zero) grid of the format-end INT4 rows as fp16 values, with the nibbles n for which n * scale - zero stays within +-65504;
    pairs that allow no nibble are dropped"""
    out = []
    for s in END_SCALES:
        s16 = F16(s)
        for z in (0.0, 8 * float(s16), -8 * float(s16), 7000.0, -65504.0):
            z16 = F16(z)
            if not np.isfinite(z16):
                continue
            ok = [n for n in range(16) if abs(n * float(s16) - float(z16)) <= 65504.0]
            if ok:
                out.append((s16, z16, ok))
    return out


def v_ends_i4(rng, n, hd, first=0):
    """INT4 V rows from end_pairs(), row j the pair (first + j) % len: every nibble present keeps n * scale - zero inside fp16's range"""
    pairs = end_pairs()
    nib, s, z = np.zeros((n, hd), np.int64), np.zeros(n, F16), np.zeros(n, F16)
    for j in range(n):
        s[j], z[j], ok = pairs[(first + j) % len(pairs)]
        nib[j] = rng.choice(ok, hd)
    return nib, s, z


# ------------------------------------------------------------------------------------------------ keys and queries

def keys_f16(lev, c, hd):
    k = np.zeros((len(lev), hd), F16)
    k[:, c] = (K_F16 * lev).astype(F16)
    assert (k[:, c].astype(F64) == K_F16 * lev).all(), "a level beyond fp16's range"
    return k


def keys_i4(lev, c, hd, kzero):
    assert lev.min() >= 0 and lev.max() <= 15
    nib = np.zeros((len(lev), hd), np.int64)
    nib[:, c] = lev
    return nib, np.full(len(lev), K_SCALE, F16), np.full(len(lev), kzero, F16)


def query(c, hd, value):
    q = np.zeros(hd, F16)
    q[c] = value
    return q


def signed_perm(hd, seed=9):
    """a signed permutation T over {+-1, +-2} (tests/kv_edge_rows.py's exact_trans): q . T is one product per element, exact"""
    rng = np.random.default_rng([hd, seed])
    T = np.zeros((hd, hd), F32)
    T[np.arange(hd), rng.permutation(hd)] = rng.choice(np.array([1, 2], F32), hd) * rng.choice(np.array([-1, 1], F32), hd)
    return T.astype(F16)


def before_trans(q, T):
    """the fp16 q0 with q0 . T == q exactly (T a signed permutation over {+-1, +-2}: q0 = q . T^-1, one exact quotient per element)"""
    T = np.asarray(T, F64)
    q0 = (np.asarray(q, F64) @ np.linalg.inv(T)).astype(F16)
    assert ((q0.astype(F64) @ T) == np.asarray(q, F64)).all()
    return q0 + F16(0)


# ------------------------------------------------------------------------------------------------ paged caches (numpy images of the tensors)

def pack(nib):
    """[.., hd] nibbles -> [.., hd / 2] bytes, feature 2 j in the low half of byte j"""
    nib = np.asarray(nib).astype(np.uint8)
    return (nib[..., 0::2] | (nib[..., 1::2] << 4)).astype(np.uint8)


def unpack(b):
    b = np.asarray(b, np.uint8)
    return np.stack((b & 15, b >> 4), axis=-1).reshape(*b.shape[:-1], -1).astype(np.int64)


class Cache:
    """a paged cache of one launch: data [pages, layers, 2, heads, page, hd / 2] uint8 (INT4) or [.., hd] fp16, param [.., page, 2] fp16 (scale,
    zero); request b owns lens[b] rows over scattered pages. Everything no request holds is FINITE filler that differs from the rows
    (0x5A bytes / 3.0, parameters (0.5, 1)), and so is the other layer."""

    def __init__(self, lens, heads, page, hd, f16, seed, layers=2, layer=1, spare=1):
        self.lens, self.heads, self.page, self.hd, self.f16, self.layer = list(lens), heads, page, hd, f16, layer
        n_pg = [-(-n // page) for n in lens]
        tot = sum(n_pg) + spare
        rng = np.random.default_rng([seed, 77])
        self.data = np.full((tot, layers, 2, heads, page, hd), 3.0, F16) if f16 else np.full((tot, layers, 2, heads, page, hd // 2), 0x5A, np.uint8)
        self.param = np.empty((tot, layers, 2, heads, page, 2), F16)
        self.param[..., 0], self.param[..., 1] = 0.5, 1.0
        self.indptr = np.concatenate([[0], np.cumsum(n_pg)]).astype(np.int32)
        self.indices = rng.permutation(tot)[:sum(n_pg)].astype(np.int32)
        self.last = np.array([(n - 1) % page + 1 for n in lens], np.int32)

    @classmethod
    def view(cls, data, param, indptr, indices, last, layer):
        """the numpy images of a cache's tensors as they are (what a launch or the cache class wrote): only `dense` is meant to be used"""
        self = cls.__new__(cls)
        self.data, self.param, self.indptr, self.indices, self.last, self.layer = data, param, indptr, indices, last, layer
        self.page, self.f16, self.heads = data.shape[4], data.dtype == F16, data.shape[3]
        self.hd = data.shape[5] if self.f16 else 2 * data.shape[5]
        self.lens = [int((indptr[b + 1] - indptr[b] - 1) * self.page + last[b]) for b in range(len(last))]
        return self

    def _where(self, b, j):
        return self.indices[self.indptr[b] + j // self.page], j % self.page

    def put(self, b, head, kv, rows, scale=None, zero=None):
        """rows [L_b, hd]: fp16 values (fp16 pages) or nibbles with their (scale, zero) [L_b]"""
        for j in range(self.lens[b]):
            pg, ent = self._where(b, j)
            if self.f16:
                self.data[pg, self.layer, kv, head, ent] = rows[j]
            else:
                self.data[pg, self.layer, kv, head, ent] = pack(rows[j])
                self.param[pg, self.layer, kv, head, ent] = (scale[j], zero[j])

    def dense(self, b, head, kv, data=None, param=None):
        """what the cache holds, read back from the tensors (INT4: from the bytes) -> (values fp64 [L_b, hd] = n * scale - zero, nibbles or None,
        scale fp64 [L_b], zero fp64 [L_b])"""
        data, param = self.data if data is None else data, self.param if param is None else param
        pgs, ents = zip(*[self._where(b, j) for j in range(self.lens[b])])
        raw = data[list(pgs), self.layer, kv, head, list(ents)]
        if self.f16:
            return raw.astype(F64), None, np.ones(len(pgs)), np.zeros(len(pgs))
        par = param[list(pgs), self.layer, kv, head, list(ents)].astype(F64)
        n = unpack(raw)
        return n * par[:, :1] - par[:, 1:], n, par[:, 0], par[:, 1]


# ------------------------------------------------------------------------------------------------ the model of the launches' arithmetic

def scores_f32(q, kraw, ks, kz, hd, f16):
    """scores in log2 units as the launches form them in fp32: [T, n] (q [T, hd] fp16; kraw the fp16 keys or the key nibbles)"""
    sm = F32(1.44269504088896340736) / np.sqrt(F32(hd))
    qf = q.astype(F32)
    dot = (qf.astype(F64) @ np.asarray(kraw, F64).T).astype(F32)                  # (integers below 2^24 here: the matrix pipe's fp32 sum is exact)
    if f16:
        return dot * sm
    return (ks.astype(F32) * sm)[None, :] * dot - ((kz.astype(F32) * sm)[None, :] * qf.sum(1, dtype=F32)[:, None])


BIG_S, BIG_SHIFT = 128.0, 2.0 ** -11       # V rows with s >= 128 enter the matrix pipe as (n - 8) 2^11 with the weight fp16(256 p s 2^-11), as in the kernels
# (2^11, not 2^12: the packed fma's addend -24 * 2^12 is no fp16 value)


def model(x, qlim, vm, s, zc, margin, fixed=True):
    """One launch in NumPy: x [T, n] fp32 scores, row j masked for token t where j > qlim[t]; vm [n, hd] what sits on the matrix pipe (n - 8, or the
    fp16 values with s = 1, zc = 0), s / zc = 8 s - z per row in fp32. 64-row tiles from row 0; the reference m moves to the tile's maximum +
    margin and rescales by exp2(m - m_new); a_j = fp16(256 p_j s_j) is the one rounded quantity; o = fp16((sum a (n - 8) / 256 + sum p zc) / l).
    fixed=False: without the per-row power of two of rows with s >= 128 — what the launches computed before they carried it; kept to show which
    cases need it (OVERFLOW_*)."""
    T, n = x.shape
    x = np.where(np.arange(n)[None, :] <= qlim[:, None], x, -np.inf).astype(F32)
    m, l, za, o = np.full(T, -np.inf, F32), np.zeros(T, F32), np.zeros(T, F32), np.zeros((T, vm.shape[1]), F32)
    sh = np.where((s >= BIG_S) & fixed, F32(BIG_SHIFT), F32(1))
    with np.errstate(over="ignore", invalid="ignore"):
        for t0 in range(0, n, 64):
            xt, sl = x[:, t0:t0 + 64], slice(t0, t0 + 64)
            mx = xt.max(1)
            m_new = np.where(mx > m, mx + F32(margin), m)
            alpha = np.where(mx > m, np.exp2((m - m_new).astype(F64)), 1.0).astype(F32)
            l, za, o, m = l * alpha, za * alpha, o * alpha[:, None], m_new
            p = np.exp2((xt - m[:, None]).astype(F64)).astype(F32)
            a = (p * (F32(256) * s[sl] * sh[sl])[None, :]).astype(F16).astype(F32)
            o = (o + (a.astype(F64) @ (vm[sl].astype(F64) / sh[sl, None].astype(F64))).astype(F32)).astype(F32)
            za = (za + (p.astype(F64) @ zc[sl].astype(F64)).astype(F32)).astype(F32)
            l = (l + p.sum(1, dtype=F32)).astype(F32)
        num = (o * F32(1 / 256) + za[:, None]).astype(F32)
        return ((num * (F32(1) / l)[:, None]) if margin == 0 else (num / l[:, None])).astype(F16)


def census(eff, qlim):
    """branch counts of one (request, row set): (token, tile) pairs that rescale to 0, rows of a 32-token wave that move while neighbours do not,
    and the sizes of S(t): singleton / power of two / other"""
    eff, qlim = np.asarray(eff), np.asarray(qlim)
    T, n = len(qlim), len(eff)
    vis = np.arange(n)[None, :] <= qlim[:, None]
    m = np.full(T, np.iinfo(np.int64).min)
    rescale0 = mixed = 0
    for t0 in range(0, n, 64):
        v = vis[:, t0:t0 + 64]
        mx = np.where(v, eff[None, t0:t0 + 64], np.iinfo(np.int64).min).max(1)
        moved = mx > m
        rescale0 += int((moved & (m > np.iinfo(np.int64).min)).sum())
        for w0 in range(0, T, 32):
            k = int(moved[w0:w0 + 32].sum())
            mixed += k if 0 < k < len(moved[w0:w0 + 32]) else 0
        m = np.maximum(m, mx)
    size = sets(eff, qlim).sum(1)
    pow2 = (size > 1) & ((size & (size - 1)) == 0)
    return dict(rescale0=rescale0, mixed=mixed, singleton=int((size == 1).sum()), pow2=int(pow2.sum()), other=int(((size > 1) & ~pow2).sum()))


# ------------------------------------------------------------------------------------------------ expectations from the built tensors

def expect(q, k64, v64, qlim, hd, nib=None, s=None, z=None, riser=False):
    """One (request, query head): q [T, hd] fp16 (after q_trans), k64 / v64 [n, hd] the fp64 rows `Cache.dense` read (or the fp16 tensors), token t
    sees rows 0 .. qlim[t] -> dict e [T, hd] fp64, tol [T, hd], size [T] (|S(t)|; 0 for risers), S. Exact families: S(t) from the fp64 scores
    (rows outside it GAP below: asserted), e the mean over it, bound 3. Risers: the fp64 softmax, bound 4."""
    x = (q.astype(F64) @ k64.T) * (math.log2(math.e) / math.sqrt(hd))
    vis = np.arange(k64.shape[0])[None, :] <= np.asarray(qlim)[:, None]
    i4 = nib is not None
    if not riser:
        S = sets_from_scores(x, vis)
        e = exact(S, v64)
        return dict(e=e, tol=bound3(e, c_term(S, s, z) if i4 else 0.0), size=S.sum(1), S=S)
    xm = np.where(vis, x, -np.inf)
    p = np.exp2(xm - xm.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    e = p @ v64
    A = p @ (s[:, None] * np.abs(nib - 8) + np.abs(8 * s - z)[:, None])
    X = np.abs(np.where(vis, x, 0.0)).max() + 8
    carry = p > 2.0 ** -100                                       # the rows that carry weight: row 0 and the riser (every other row lies GAP below)
    return dict(e=e, tol=bound4(e, A, X, c_term(carry, s, z)), size=np.zeros(len(qlim), np.int64), S=carry)


# ------------------------------------------------------------------------------------------------ cases of the prompt launch

PATTERNS_F16 = ("uniform", "sink", "staircase", "blocks", "one_hot")
PATTERNS_I4 = ("uniform", "sink", "stairs16", "blocks", "one_hot")


def prefill_case(seqs, heads, kv_heads, seed, trans=False, ends=False, one_hot_batch=False, start=None, seq=None, level0=False):
    """The prompt launch's tensors: request b has seqs[b] tokens (at start[b] of a row of `seq` positions where given: the ranged call; the rest
    of the row is finite filler and its answer zeros). (request, KV head) pairs take different patterns, seeds and features c; query head h
    carries the sign + / - by h % 2 (-: the LOWEST level wins). ends: singleton patterns with format-end V rows, sign + only. level0: the
    uniform pattern's q = 0 replaced by the ordinary query (its keys are all level 0: the same answer bit for bit).
    -> dict q (before q_trans), k, v, qt, e, tol, size (|S(t)|, 0 outside a range), inside"""
    hd, batch, grp = 128, len(seqs), heads // kv_heads
    seq = seq or max(seqs)
    start = start or [0] * batch
    rng = np.random.default_rng([seed, seq, heads])
    q, k, v = (rng.integers(-2, 3, (batch, seq, n, hd)).astype(F16) for n in (heads, kv_heads, kv_heads))
    qt = signed_perm(hd) if trans else None
    e, tol = np.zeros((batch, seq, heads, hd)), np.zeros((batch, seq, heads, hd))
    size, inside, eff = np.zeros((batch, seq, heads), np.int64), np.zeros((batch, seq), bool), {}
    spots = one_hot_positions(seq, batch) if one_hot_batch else None
    for b in range(batch):
        n, s0 = seqs[b], start[b]
        inside[b, s0:s0 + n] = True
        for y in range(kv_heads if n else 0):
            i = b * kv_heads + y + seed
            pats = SINGLETON if ends else PATTERNS_F16
            pat = "one_hot" if one_hot_batch else pats[i % len(pats)]
            c = FEATURES[hd][i % 3]
            jstar = spots[b] if one_hot_batch else int(rng.integers(0, n))
            lev = levels(pat, n, rng, jstar)
            kk = keys_f16(lev, c, hd)
            vv = v_int(rng, n, hd)
            if ends:
                vv[jstar if pat == "one_hot" else 0:] = v_ends_f16(rng, n, hd)[jstar if pat == "one_hot" else 0:]
            k[b, s0:s0 + n, y], v[b, s0:s0 + n, y] = kk, vv
            for h in range(y * grp, (y + 1) * grp):
                sign = 1.0 if ends or h % 2 == 0 else -1.0
                qq = np.tile(query(c, hd, 0.0 if pat == "uniform" and not level0 else sign * Q_F16), (n, 1))
                r = expect(qq, kk.astype(F64), vv.astype(F64), np.arange(n), hd)
                e[b, s0:s0 + n, h], tol[b, s0:s0 + n, h], size[b, s0:s0 + n, h] = r["e"], r["tol"], r["size"]
                q[b, s0:s0 + n, h] = before_trans(qq, qt) if trans else qq
                eff[b, h] = lev * (0 if pat == "uniform" and not level0 else int(sign))
    return dict(q=q, k=k, v=v, qt=qt, e=e, tol=tol, size=size, inside=inside, hd=hd, eff=eff)


PREFILL_GEOMS = [(1, 1, 1), (2, 4, 2), (2, 6, 2)]            # (batch, heads, kv_heads)
PREFILL_SEQS = [1, 63, 64, 65, 129, 300]
# (name, kwargs of prefill_case): every seq with a geometry, with and without q_trans; format-end rows; the 64-request one_hot batch at seq 200
PREFILL_CASES = [(f"seq{s}-g{i % 3}-{'qt' if t else 'plain'}", dict(seqs=[s] * PREFILL_GEOMS[(i + t) % 3][0], heads=PREFILL_GEOMS[(i + t) % 3][1],
                                                                  kv_heads=PREFILL_GEOMS[(i + t) % 3][2], seed=i, trans=bool(t)))
                 for i, s in enumerate(PREFILL_SEQS) for t in (0, 1)]
PREFILL_CASES += [(f"ends-seq{s}", dict(seqs=[s, s, s], heads=6, kv_heads=3, seed=s, trans=s == 129, ends=True)) for s in (65, 129, 300)]
PREFILL_CASES += [("one_hot-batch64-seq200", dict(seqs=[200] * 64, heads=2, kv_heads=1, seed=5, one_hot_batch=True))]
PREFILL_RANGED = dict(seqs=[37, 131, 200, 1, 0], start=[163, 0, 0, 66, 100], seq=200, heads=4, kv_heads=2, seed=11)   # left padding, a length-0 row
PREFILL_UNIFORM = dict(seqs=[129, 129], heads=2, kv_heads=1, seed=0)      # (seed 0, one KV head: both requests... pattern i % 5: uniform and sink)


def prefill_model(case):
    """`model` over a prompt case -> fp16 [batch, seq, heads, hd] (margin 0, fp16 V: s = 1, zc = 0); zeros outside the ranges"""
    q, k, v, qt = case["q"], case["k"], case["v"], case["qt"]
    batch, seq, heads, hd = q.shape
    grp = heads // k.shape[2]
    out = np.zeros(q.shape, F16)
    for b in range(batch):
        pos = np.flatnonzero(case["inside"][b])
        if not len(pos):
            continue
        for h in range(heads):
            qq = q[b, pos, h] if qt is None else (q[b, pos, h].astype(F32) @ qt.astype(F32)).astype(F16)
            kk, vv = k[b, pos, h // grp], v[b, pos, h // grp]
            n = len(pos)
            out[b, pos, h] = model(scores_f32(qq, kk, None, None, hd, True), np.arange(n), vv.astype(F32), np.ones(n, F32), np.zeros(n, F32), 0)
    return out


# ------------------------------------------------------------------------------------------------ cases over the paged cache

RISER_G = (6.0, 7.0, 7.9)                # the riser's score above row 0's, log2 units
RISER_POS = (70, 133, 261)               # a later tile than row 0's; 133 / 261: the same wave as row 0 in a later step of a 4- / 8-wave workgroup
RISER_SCALES = (1.0, 1000.0)


def riser_request(i):
    """the i-th riser combination -> (position, g, V scale of the riser)"""
    return RISER_POS[i % 3], RISER_G[(i // 3) % 3], RISER_SCALES[(i // 9) % 2]


def paged_case(lens, T, sets_n, q_group, page, hd=128, f16=False, copies=1, family="mixed", seed=0, trans=False, one_hot_batch=False, level0=False,
               riser=None):
    """A paged cache and the queries of one launch: request b holds lens[b] rows, its T tokens see rows 0 .. lens[b] - T + t. `sets_n` sets of
    cached rows per request (KV heads); each serves q_group query heads (copies > 1: the replicated layout, copies identical cache heads per
    set, query heads == cache heads). (request, set) pairs take different patterns, seeds, features c and K zero points; query head h carries
    the sign by h % 2 in the family `mixed`. Families: mixed (integer / dyadic payloads), ends (singleton patterns, format-end rows from the
    dominant row on), riser (INT4: row 0 and one later row g log2 units above it, every other row GAP below; `riser` = k: every request holds
    combination k of riser_request, otherwise they cycle).
    -> dict cache, q [batch, T, H, hd] (before q_trans), qt, e, tol, size, G (query heads per set), meta"""
    batch, G = len(lens), copies if copies > 1 else q_group
    assert copies == 1 or q_group == 1
    H, heads = sets_n * G, sets_n * copies
    rng = np.random.default_rng([seed, T, hd, sum(lens)])
    cache = Cache(lens, heads, page, hd, f16, seed)
    q = np.zeros((batch, T, H, hd), F16)
    qt = signed_perm(hd) if trans else None
    e, tol, size = np.zeros((batch, T, H, hd)), np.zeros((batch, T, H, hd)), np.zeros((batch, T, H), np.int64)
    spots = one_hot_positions(min(lens), batch) if one_hot_batch else None
    eff = {}
    for b in range(batch):
        L = lens[b]
        qlim = L - T + np.arange(T)
        for y in range(sets_n):
            i = b * sets_n + y + seed
            c, c2 = FEATURES[hd][i % 3], FEATURES[hd][(i + 1) % 3]
            qrow = None
            if family == "riser":
                pos, g, vscale = riser_request(i if riser is None else riser)
                assert not f16 and pos < L
                knib = np.zeros((L, hd), np.int64)
                knib[[0, pos], c], knib[pos, c2] = 15, 1
                ks, kz = np.full(L, K_SCALE, F16), np.zeros(L, F16)
                qrow = query(c, hd, Q_F16)
                qrow[c2] = g / (K_SCALE * math.log2(math.e) / math.sqrt(hd))
                vnib, vs, vz = v_i4(rng, L, hd)
                vs[0], vz[0], vs[pos], vz[pos] = 1.0, 2.0, vscale, 3 * vscale
                pat = "riser"
            else:
                pats = (("sink", "one_hot") if not f16 else SINGLETON) if family == "ends" else PATTERNS_F16 if f16 else PATTERNS_I4
                pat = "one_hot" if one_hot_batch else pats[i % len(pats)]
                if pat == "staircase" and L > 500:
                    pat = "blocks"                                            # (128 lev must stay an fp16 value)
                jstar = spots[b] if one_hot_batch else int(rng.integers(0, L))
                lev = levels(pat, L, rng, jstar)
                dom = jstar if pat == "one_hot" else 0
                if f16:
                    knib, ks, kz = keys_f16(lev, c, hd), None, None
                    vnib, vs, vz = v_int(rng, L, hd), None, None
                    if family == "ends":
                        vnib[dom:] = v_ends_f16(rng, L, hd)[dom:]
                else:
                    knib, ks, kz = keys_i4(lev, c, hd, K_ZEROS[i % 2])
                    vnib, vs, vz = v_i4(rng, L, hd)
                    if family == "ends":
                        en, es, ez = v_ends_i4(rng, L, hd, first=i * 7)
                        vnib[dom:], vs[dom:], vz[dom:] = en[dom:], es[dom:], ez[dom:]
            for cp in range(copies):
                cache.put(b, y * copies + cp, 0, knib, ks, kz)
                cache.put(b, y * copies + cp, 1, vnib, vs, vz)
            k64, _, _, _ = cache.dense(b, y * copies, 0)
            v64, n64, s64, z64 = cache.dense(b, y * copies, 1)
            for h in range(y * G, (y + 1) * G):
                if family == "riser":
                    qq = np.tile(qrow, (T, 1))
                else:
                    sign = 1.0 if family == "ends" or h % 2 == 0 else -1.0
                    qq = np.tile(query(c, hd, 0.0 if pat == "uniform" and not level0 else sign * (Q_F16 if f16 else Q_I4)), (T, 1))
                    eff[b, h] = lev * (0 if pat == "uniform" and not level0 else int(sign))
                r = expect(qq, k64, v64, qlim, hd, n64, s64, z64, riser=family == "riser")
                e[b, :, h], tol[b, :, h], size[b, :, h] = r["e"], r["tol"], r["size"]
                q[b, :, h] = before_trans(qq, qt) if trans else qq
    return dict(cache=cache, q=q, qt=qt, e=e, tol=tol, size=size, G=G, T=T, hd=hd, f16=f16, copies=copies, family=family, eff=eff)


def paged_rows(case):
    """per (request, query head) of a paged case: (b, h, q after q_trans [T, hd], k64, v64, V nibbles or None, s, z, qlim), read from the cache"""
    cache, q, qt = case["cache"], case["q"], case["qt"]
    for b, L in enumerate(cache.lens):
        qlim = L - q.shape[1] + np.arange(q.shape[1])
        for h in range(q.shape[2]):
            head = (h // case["G"]) * case["copies"]
            v64, nib, s, z = cache.dense(b, head, 1)
            qq = q[b, :, h] if qt is None else (q[b, :, h].astype(F32) @ qt.astype(F32)).astype(F16)
            yield b, h, qq, cache.dense(b, head, 0)[0], v64, nib, s, z, qlim


def prefill_rows(case):
    """the same for a prompt case (the positions inside the request's range)"""
    q, k, v, qt = case["q"], case["k"], case["v"], case["qt"]
    grp = q.shape[2] // k.shape[2]
    for b in range(q.shape[0]):
        pos = np.flatnonzero(case["inside"][b])
        for h in range(q.shape[2] if len(pos) else 0):
            qq = q[b, pos, h] if qt is None else (q[b, pos, h].astype(F32) @ qt.astype(F32)).astype(F16)
            yield b, h, qq, k[b, pos, h // grp].astype(F64), v[b, pos, h // grp].astype(F64), None, None, None, np.arange(len(pos))


def paged_model(case, margin, fixed=True):
    """`model` over a paged case, read from the cache's tensors -> fp16 [batch, T, H, hd]"""
    cache, q, qt, G, hd = case["cache"], case["q"], case["qt"], case["G"], case["hd"]
    out = np.zeros(q.shape, F16)
    for b, L in enumerate(cache.lens):
        qlim = L - q.shape[1] + np.arange(q.shape[1])
        for h in range(q.shape[2]):
            head = (h // G) * case["copies"]
            k64, kn, ks, kz = cache.dense(b, head, 0)
            v64, vn, vs, vz = cache.dense(b, head, 1)
            qq = q[b, :, h] if qt is None else (q[b, :, h].astype(F32) @ qt.astype(F32)).astype(F16)
            if cache.f16:
                x, vm, s, zc = scores_f32(qq, k64, None, None, hd, True), v64.astype(F32), np.ones(L, F32), np.zeros(L, F32)
            else:
                x = scores_f32(qq, kn, ks.astype(F32), kz.astype(F32), hd, False)
                vm, s, zc = (vn - 8).astype(F32), vs.astype(F32), (F32(8) * vs.astype(F32) - vz.astype(F32)).astype(F32)
            out[b, :, h] = model(x, qlim, vm, s, zc, margin, fixed)
    return out


def check(o, case):
    """o fp16 like case['e'] (numpy) -> list of failures (empty: the case holds): all finite; singleton sets on fp16 pages bit-equal to the V row
    (where `bits`); everything within its bound"""
    o = np.asarray(o)
    bad = []
    if not np.isfinite(o).all():
        bad.append(f"{int((~np.isfinite(o)).sum())} non-finite outputs")
    with np.errstate(invalid="ignore"):
        err = np.abs(o.astype(F64) - case["e"])
        over = ~(err <= case["tol"])
    if over.any():
        i = np.unravel_index(np.argmax(np.where(np.isfinite(err), err / case["tol"], np.inf)), err.shape)
        bad.append(f"{int(over.sum())} outputs outside the bound; worst at {i}: got {o[i]}, exact {case['e'][i]}, bound {case['tol'][i]:.3e}")
    return bad


def check_bits(o, case):
    """singleton sets with fp16 V: bit equality with the V row (e is then an fp16 value)"""
    if not case.get("f16", True):
        return []
    one = case["size"] == 1
    want = case["e"][one].astype(F16)
    assert (want.astype(F64) == case["e"][one]).all()
    same = np.asarray(o)[one].view(np.int16) == want.view(np.int16)
    return [] if same.all() else [f"{int((~same).sum())} elements of singleton sets differ from their V row in bits"]


# (L, T) of the extend launches: one tile; L = T with a ragged tile; L - T > 1 tile; the second block holds one token; the diagonal in mid-tile
EXTEND_LT = [(64, 64), (70, 70), (200, 71), (300, 33), (513, 130)]
# name -> kwargs of paged_case; both extend launches are fed every one of them
EXTEND_CASES = {}
for _i, (_L, _T) in enumerate(EXTEND_LT):
    _g = (1, 4, 8)[_i % 3]
    EXTEND_CASES[f"i4-L{_L}-T{_T}-g{_g}-p{(16, 24)[_i % 2]}"] = dict(lens=[_L, _T + 1, _L + 3], T=_T, sets_n=2, q_group=_g, page=(16, 24)[_i % 2], seed=_i)
    EXTEND_CASES[f"f16-L{_L}-T{_T}-g{(4, 8, 1)[_i % 3]}-p{(24, 16)[_i % 2]}"] = dict(lens=[_L, _T + 1, _L + 3], T=_T, sets_n=2, q_group=(4, 8, 1)[_i % 3],
                                                                                 page=(24, 16)[_i % 2], f16=True, seed=10 + _i)
EXTEND_CASES["i4-copies4-L200-T71"] = dict(lens=[200, 90], T=71, sets_n=2, q_group=1, copies=4, page=16, seed=20)
EXTEND_CASES["i4-qt-L300-T33"] = dict(lens=[300, 40], T=33, sets_n=2, q_group=4, page=16, seed=21, trans=True)
EXTEND_CASES["f16-qt-L70-T70"] = dict(lens=[70, 71], T=70, sets_n=1, q_group=2, page=24, f16=True, seed=22, trans=True)
EXTEND_CASES["i4-one_hot-batch64-L200-T200"] = dict(lens=[200] * 64, T=200, sets_n=1, q_group=1, page=16, seed=23, one_hot_batch=True)
EXTEND_CASES["f16-ends-L200-T71"] = dict(lens=[200, 72, 130], T=71, sets_n=3, q_group=2, page=16, f16=True, family="ends", seed=24)
EXTEND_CASES["i4-ends-L200-T71"] = dict(lens=[200, 72, 130, 199, 80, 300], T=71, sets_n=3, q_group=2, page=16, family="ends", seed=25)
EXTEND_CASES["i4-ends-L513-T130"] = dict(lens=[513, 131, 400], T=130, sets_n=4, q_group=1, page=24, family="ends", seed=26)
EXTEND_CASES["i4-riser-T1"] = dict(lens=[300] * 9, T=1, sets_n=2, q_group=4, page=16, family="riser", seed=27)
EXTEND_CASES["i4-riser-T33"] = dict(lens=[300] * 9, T=33, sets_n=2, q_group=1, page=16, family="riser", seed=28)
# the margin launches meet every riser combination in a launch of its own (RISER_EXTEND: fq_kv_batch_extend; the decode's four-head launch below)
N_RISER = 18
RISER_EXTEND = {f"i4-riser{k}-T{T}": dict(lens=[300] * 2, T=T, sets_n=2, q_group=g, page=16, family="riser", seed=70 + k, riser=k)
                for k in range(N_RISER) for T, g in ((1, 4), (33, 1))}
EXTEND_UNIFORM = dict(lens=[200, 72, 130, 199, 71], T=71, sets_n=1, q_group=2, page=16, seed=0)      # patterns i % 5: request 0 is `uniform`

# the decode launches (T = 1). name -> (kwargs of paged_case, kwargs of ops.kv_batch_decode). Lengths 1, 16, 17, 300; head_dim 128 and 64; INT4 and
# fp16 pages; per-head, split (one request of 2048 rows, seq_hint) and merged launches on both sides of 32 (request, KV head) pairs; q_group 2
# (fp32 sums) and 4 (matrix pipe); the replicated layout
DECODE_LENS = [1, 16, 17, 300]
DECODE_CASES = {}
for _hd in (128, 64):
    for _f16 in (False, True):
        _n = f"{'f16' if _f16 else 'i4'}-hd{_hd}"
        DECODE_CASES[f"{_n}-per-head"] = (dict(lens=DECODE_LENS, T=1, sets_n=3, q_group=1, page=16, hd=_hd, f16=_f16, seed=30), dict(split=False))
        DECODE_CASES[f"{_n}-per-head-p24"] = (dict(lens=DECODE_LENS, T=1, sets_n=2, q_group=1, page=24, hd=_hd, f16=_f16, seed=31), dict(split=False))
        DECODE_CASES[f"{_n}-split-2048"] = (dict(lens=[2048], T=1, sets_n=5, q_group=1, page=16, hd=_hd, f16=_f16, seed=32), dict(seq_hint=2048))
        DECODE_CASES[f"{_n}-ends"] = (dict(lens=DECODE_LENS * 2, T=1, sets_n=3, q_group=1, page=16, hd=_hd, f16=_f16, family="ends", seed=33), dict(split=False))
for _f16 in (False, True):
    _n = "f16" if _f16 else "i4"
    for _g in (2, 4):
        DECODE_CASES[f"{_n}-g{_g}-below-32-pairs"] = (dict(lens=DECODE_LENS, T=1, sets_n=2, q_group=_g, page=16, f16=_f16, seed=40 + _g), dict(split=False))
        DECODE_CASES[f"{_n}-g{_g}-merged"] = (dict(lens=DECODE_LENS * 4, T=1, sets_n=2, q_group=_g, page=16, f16=_f16, seed=42 + _g), dict(split=False))
        DECODE_CASES[f"{_n}-g{_g}-merged-ends"] = (dict(lens=DECODE_LENS * 4, T=1, sets_n=2, q_group=_g, page=16, f16=_f16, family="ends", seed=44 + _g), dict(split=False))
    DECODE_CASES[f"{_n}-g4-merged-split-2048"] = (dict(lens=[2048, 300] * 16, T=1, sets_n=1, q_group=4, page=16, f16=_f16, seed=50), dict(seq_hint=2048))
    DECODE_CASES[f"{_n}-copies4-merged"] = (dict(lens=DECODE_LENS * 4, T=1, sets_n=2, q_group=1, copies=4, page=16, f16=_f16, seed=51), dict(split=False))
    DECODE_CASES[f"{_n}-copies2-below-32"] = (dict(lens=DECODE_LENS, T=1, sets_n=2, q_group=1, copies=2, page=16, f16=_f16, seed=52), dict(split=False))
for _g in (1, 2):
    DECODE_CASES[f"i4-riser-g{_g}"] = (dict(lens=[300] * 18, T=1, sets_n=2, q_group=_g, page=16, family="riser", seed=60 + _g), dict(split=False))
for _k in range(N_RISER):                                  # the four-head launch (32 (request, KV head) pairs): one combination per launch
    DECODE_CASES[f"i4-riser{_k}-g4"] = (dict(lens=[300] * 16, T=1, sets_n=2, q_group=4, page=16, family="riser", seed=80 + _k, riser=_k), dict(split=False))
DECODE_UNIFORM = dict(lens=[300, 17, 16, 1, 40], T=1, sets_n=1, q_group=1, page=16, seed=0)

# fq_kv_chunk_extend carries a per-row power of two for V rows with s >= 128; without it these cases reach fp16(256 p s_v) = Inf (p = 1 at
# s_v >= 256): the model with fixed=False returns non-finite values on exactly these
OVERFLOW_CHUNK = ("i4-ends-L200-T71", "i4-ends-L513-T130", "i4-riser-T1", "i4-riser-T33")


def riser_overflows(k):
    """the margin launches' limit p s_v < 256 (fq_kvextend.hip, the four-head form of fq_kvcache.hip): combination k has a riser of scale
    1000 with g >= 7 (p s_v = 2^(g - 8) 1000 = 500, 933; g = 6 gives 250 and passes) — overflows where the riser meets row 0's reference, i.e.
    sits in a later step of the wave that holds row 0"""
    pos, g, scale = riser_request(k)
    return scale == 1000.0 and g >= 7.0


# (route, combination) pairs in which the riser does meet row 0's reference — which positions share row 0's wave depends on the launch's waves and
# splits —: the cases tests/test_gpu_attn_closed_form.py marks xfail(strict=True), exactly these
# (scale 1000, g = 7 / 7.9, position 133 or 261 = row 0's wave; the split launch deals its waves otherwise and only 261 meets row 0's there)
MARGIN_OVERFLOW = {"extend": (13, 14, 16, 17), "extend-split": (14, 17), "g4": (13, 14, 16, 17)}
assert all(riser_overflows(k) and riser_request(k)[0] != 70 for v in MARGIN_OVERFLOW.values() for k in v)
