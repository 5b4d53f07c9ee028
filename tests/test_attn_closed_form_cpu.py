"""tests/attn_closed_form.py held to itself, without a GPU: every pattern's S(t) against a brute-force softmax of the built tensors (weights
outside S exactly 0.0 through fp32 exp2, weights inside equal), every exact answer finite and inside fp16's range, the NumPy model of the
launches' arithmetic inside bounds 3 and 4 on every case tests/test_gpu_attn_closed_form.py runs (and, without the per-row power of two of large
V scales, non-finite on exactly the cases that need it), one key deleted from one S(t) moves the answer outside bound 3, and the branch census of the shapes."""
import functools
import math

import numpy as np
import pytest

from tests import attn_closed_form as A

F32, F64 = np.float32, np.float64
PAGED = {**{f"extend-{n}": kw for n, kw in {**A.EXTEND_CASES, **A.RISER_EXTEND}.items()}, **{f"decode-{n}": kw for n, (kw, _) in A.DECODE_CASES.items()},
         "extend-uniform": A.EXTEND_UNIFORM, "decode-uniform": A.DECODE_UNIFORM}
PREFILL = {**dict(A.PREFILL_CASES), "ranged": A.PREFILL_RANGED, "uniform": A.PREFILL_UNIFORM}


@functools.lru_cache(maxsize=None)
def _case(name):
    return A.paged_case(**PAGED[name]) if name in PAGED else A.prefill_case(**PREFILL[name])


def _rows(name):
    c = _case(name)
    return c, (A.paged_rows(c) if name in PAGED else A.prefill_rows(c))


def _scores(qq, k64, hd):
    return (qq.astype(F64) @ k64.T) * (math.log2(math.e) / math.sqrt(hd))


ALL = list(PREFILL) + list(PAGED)
EXACT = [n for n in ALL if "riser" not in n]


@pytest.mark.parametrize("name", EXACT)
def test_sets_against_a_brute_force_softmax(name):
    """S(t) from the levels == the visible rows at the fp64 maximum; through fp32 exp2 against the maximum (and against the maximum + 8, the margin
    launches' reference) the weights outside S are exactly 0.0 and the weights inside are one value; max + 8 is exact in fp32"""
    c, rows = _rows(name)
    for b, h, qq, k64, v64, nib, s, z, qlim in rows:
        x = _scores(qq, k64, c["hd"])
        vis = np.arange(k64.shape[0])[None, :] <= qlim[:, None]
        S = A.sets(c["eff"][b, h], qlim)
        assert np.array_equal(S, A.sets_from_scores(x, vis)), (b, h)
        x32 = np.where(vis, x.astype(F32), -np.inf).astype(F32)
        top = x32.max(1, keepdims=True)
        assert ((top + F32(8)).astype(F32).astype(F64) == top.astype(F64) + 8).all(), "max + 8 rounds in fp32"
        for ref in (top, top + F32(8)):
            w = np.exp2((x32 - ref).astype(F64)).astype(F32)
            assert (w[~S] == 0.0).all() and (np.where(S, w, w.max(1, keepdims=True)) == w.max(1, keepdims=True)).all() and (w.max(1) > 0).all()


@pytest.mark.parametrize("name", ALL)
def test_exact_answers_are_finite_and_in_range(name):
    c = _case(name)
    assert np.isfinite(c["e"]).all() and np.abs(c["e"]).max() <= 65504 and np.isfinite(c["tol"]).all() and (c["tol"] >= 0).all()
    for k in ("q", "k", "v"):
        assert k not in c or np.isfinite(c[k]).all()
    if name in PAGED:
        assert np.isfinite(c["cache"].param).all() and (c["cache"].f16 is False or np.isfinite(c["cache"].data).all())


@pytest.mark.parametrize("name", list(PREFILL))
def test_model_of_the_prompt_launch_stays_inside_the_bounds(name):
    c = _case(name)
    o = A.prefill_model(c)
    assert not A.check(o, c) and not A.check_bits(o, c)


def _overflows(name, margin):
    """does the model WITHOUT the per-row power of two overflow here? margin 0: the cases of OVERFLOW_CHUNK and every riser launch of scale 1000;
    margin 8 (row 0 and the riser share the model's one running reference): every riser launch that holds a combination with p s_v >= 256"""
    short = name.split("-", 1)[1]
    if "riser" in short and short.split("riser")[1][0].isdigit():
        k = int(short.split("riser")[1].split("-")[0])
        return A.riser_overflows(k) if margin == 8 else A.riser_request(k)[2] == 1000.0
    return short in A.OVERFLOW_CHUNK if margin == 0 else "riser" in short


@pytest.mark.parametrize("name,margin", [(n, m) for n in PAGED for m in (0, 8) if m == 8 or n.startswith("extend")])
def test_model_of_the_paged_launches_stays_inside_the_bounds(name, margin):
    """margin 0: fq_kv_chunk_extend; margin 8: fq_kv_batch_extend and the decode launches. With the per-row power of two of V rows with
    s >= 128 (the launches' arithmetic) the model holds everywhere; without it it returns non-finite values on the cases that reach
    p s_v >= 256, and holds on every other."""
    c = _case(name)
    assert not A.check(A.paged_model(c, margin, fixed=True), c)
    o = A.paged_model(c, margin, fixed=False)
    if _overflows(name, margin):
        assert not np.isfinite(o).all()
    else:
        assert not A.check(o, c)
        if c["f16"]:
            assert not A.check_bits(o, c)


@pytest.mark.parametrize("name", EXACT)
def test_deleting_one_key_moves_the_answer_outside_bound_3(name):
    """per (request, head): the last token and a middle one, the first and the last member of S(t) made invisible in turn"""
    c, rows = _rows(name)
    tried = 0
    for b, h, qq, k64, v64, nib, s, z, qlim in rows:
        x = _scores(qq, k64, c["hd"])
        for t in {len(qlim) - 1, len(qlim) // 2}:
            vis = np.arange(k64.shape[0]) <= qlim[t]
            if vis.sum() < 2:
                continue
            r = A.expect(qq[t:t + 1], k64, v64, qlim[t:t + 1], c["hd"], nib, s, z)
            for j in {int(np.flatnonzero(r["S"][0])[0]), int(np.flatnonzero(r["S"][0])[-1])}:
                keep = vis.copy()
                keep[j] = False
                S2 = A.sets_from_scores(x[t:t + 1], keep[None])
                e2 = A.exact(S2, v64)
                assert (np.abs(e2 - r["e"]) > r["tol"]).any(), (b, h, t, j)
                tried += 1
    lengths = PAGED[name]["lens"] if name in PAGED else PREFILL[name]["seqs"]
    assert tried > 0 or max(lengths) == 1                      # (a request of one row has no key to delete)


@pytest.mark.parametrize("family", ["prompt", "extend", "decode"])
def test_branch_census(family):
    """(the decode shapes have one token per request: a wave of 32 tokens there is the one token, which cannot move while a neighbour does not)"""
    names = list(PREFILL) if family == "prompt" else [n for n in PAGED if n.startswith(family) and "riser" not in n]
    total = {}
    for name in names:
        c, rows = _rows(name)
        for b, h, qq, k64, v64, nib, s, z, qlim in rows:
            for k, n in A.census(c["eff"][b, h], qlim).items():
                total[k] = total.get(k, 0) + n
    print(family, total)
    assert all(total[k] > 0 for k in ("rescale0", "mixed", "singleton", "pow2", "other") if not (family == "decode" and k == "mixed")), total


def test_risers_reach_weights_between_a_half_and_one_under_the_margin():
    """row 0 sets the margin launches' reference 8 above its score; the riser then weighs 2^(g - 8) ... and 1 in the chunk launch"""
    c = _case("extend-i4-riser-T1")
    assert sorted(k for k in range(A.N_RISER) if A.riser_overflows(k)) == [12, 13, 14, 15, 16, 17]
    seen = set()
    for b, h, qq, k64, v64, nib, s, z, qlim in A.paged_rows(c):
        x = _scores(qq, k64, c["hd"])[0]
        pos = int(np.argmax(x))
        g = x[pos] - x[0]
        assert pos >= 64 and 5.9 < g < 8 and (np.delete(x, [0, pos]) < x[0] - A.GAP).all()
        seen.add((pos, round(g), float(s[pos])))
    assert len(seen) == 18


def test_end_pairs_hold_the_scales_of_the_issue():
    pairs = A.end_pairs()
    scales = {float(s) for s, _, _ in pairs}
    assert {1.0, 255.0, 256.0, 1000.0, float(np.float16(4366.0))} <= scales and min(scales) < 2.0 ** -14
    assert any(float(z) == -65504.0 for _, z, _ in pairs) and any(float(z) == 7000.0 for _, z, _ in pairs)
