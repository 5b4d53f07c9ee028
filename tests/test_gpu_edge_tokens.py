"""Edge tokens through every fused transform + INT4 family, bit for bit (builders: tests/edge_tokens.py; their own checks: test_edge_tokens_cpu.py).

The batch is 25 rows: twelve edge tokens (all zero, single-signed, one-hot in the first / last element, a 15000 outlier, subnormals, .5 ties,
constants, an all-zero scale group) at the odd positions, ordinary Gaussian rows between them. Every assertion is BIT EQUALITY:
  (a) exact factors (signed permutations over {-1, -2}: every output element is one product, no accumulation order matters): every output of
      every output set equals the oracle's END TO END — packed bytes, scales, fake-quant bits, transform; the head transform
      (ops.block_quant) and the grouped launch (ops.kron_quant_grouped) the same way;
  (b) random factors: the families' own bar on these rows — the quantiser bit-exact on the kernel's OWN transform (T|P|F|R16 against
      O.quant_outputs of the returned y; the packed-only kernels against the T launch's y, over all of SIGS);
  (c) position and neighbour independence, no reference needed: the batch rolled by one and two rows gives the rolled outputs, and a launch
      ABOVE THE LAUNCHER'S GRID CAP whose row i is batch[i % 25] gives the 25-row outputs tiled, every byte — there a persistent token group
      takes an ordinary token straight after an edge token with the same LDS token buffer and reduction words. The same with NaN / Inf /
      overflowing rows (test names holding "nonfinite"): every OTHER row is bit-identical to the launch in which those rows are zero; the
      non-finite rows' own digits are pinned by no reference and not asserted. The launches whose prologue is not exact (RMSNorm, SiLU.mul,
      the Hadamard rotations) are held under (c) only HERE; tests/test_gpu_prologue_ref.py holds them to derived references.
No tolerance, no flip rate, no skipped pair: where the library has no instantiation the refusal (FQ_EUNSUPPORTED / ValueError) is asserted."""
import numpy as np
import pytest
import torch

from oracle import fq_oracle as O
from tests import edge_tokens as E
from tests.conftest import hadk_matrix, same_bits
from tests.test_gpu_bounds import BIG, WAVE_BIG

pytestmark = pytest.mark.gpu
P, F, T, R16, NC0, Q16 = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
# the sets with packed-only kernels: the first three own the three quantiser routes, the last is the fp16-arithmetic quantiser (the "H16"
# builds of the trio / tall / tiles / fast kernels, fq_quant8_h16), where the small clip pairs make the fp16 scale underflow to 0
PACKED_ONLY = [P | NC0, P, P | R16, P | R16 | Q16]
OTHER_SETS = [F | R16, T | P | F | R16, F | R16 | Q16]
INDEP_SETS = [P | R16, P | NC0, T | P | F | R16]
INDEP_SIGS = [E.SIGS[1], E.SIGS[7]]                     # between them: magic-number rounding with and without the clamp, true division
WAVE_PAIRS = set(E.PAIRS["wave"])
CASES = [(M, N, lowp) for (M, N) in E.ALL_PAIRS for lowp in ("f16", "bf16")]


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


def dev(a, lowp="f16"):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(torch.bfloat16) if lowp == "bf16" else t).cuda()


def bits16(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def kw(flags):
    return dict(round_y_f16=bool(flags & R16), clamp0=not flags & NC0, quant_f16=bool(flags & Q16))


def assert_outputs(o, ci, ref, flags, lowp, what):
    """every output the flag set asks for, against one oracle dict"""
    rows = ref["packed"].shape[0]
    bf = lowp == "bf16"
    as_bits = (lambda a: O.bf16_bits(a)) if bf else (lambda a: np.ascontiguousarray(a).view(np.uint16))
    if flags & P:
        assert np.array_equal(o.q[ci].reshape(rows, -1).cpu().numpy(), ref["packed"]), (what, "packed")
        assert np.array_equal(bits16(o.scale[ci]).reshape(ref["scale16"].shape), as_bits(ref["scale16"])), (what, "scale")
    if flags & F:
        fq = o.fq[ci].reshape(rows, -1)
        ok = np.array_equal(bits16(fq), O.bf16_bits(ref["fq"])) if bf else same_bits(fq.cpu().numpy(), ref["fq"])
        assert ok, (what, "fake-quant bits")
    if flags & T:
        y = o.y.reshape(rows, -1)
        got = O.bf16_from_bits(bits16(y)) if bf else y.cpu().numpy()
        assert np.array_equal(got, ref["y16"]), (what, "transform")


_exact = {}


def exact_case(M, N, lowp):
    """the batch, the exact factors and the oracle's transform of the batch: computed once per (pair, dtype), never modified"""
    key = (M, N, lowp)
    if key not in _exact:
        b = E.batch(M, N, lowp)
        L, R = E.exact_factors(M, N, lowp)
        _exact[key] = (b, L, R, O.kron_transform(b, L, R, lowp=lowp).reshape(E.N_BATCH, -1))
        for a in _exact[key]:
            a.setflags(write=False)
    return _exact[key]


def raw(o):
    """every tensor of a FusedOutputs (or a tuple of tensors / None) as integers: compared with torch.equal, NaNs included"""
    ts = (list(o.q) + list(o.scale) + list(o.fq) + [o.y]) if hasattr(o, "fq") else list(o)
    return [t if t.dtype == torch.uint8 else t.view(torch.int16) for t in ts if t is not None]


def big_rows(M, N, flags):
    """a row count above the grid cap of the launcher this pair and output set reach (tests/test_gpu_bounds.py lists the caps)"""
    if flags & F and M * N > 16384:
        return 519                                      # (footprint of the 16-bit outputs of tokens above 32 KB; their cap is 2 n_cu)
    return WAVE_BIG if (M, N) in WAVE_PAIRS else BIG


# ------------------------------------------------------------------------------------------------ (a) exact factors, end to end

@pytest.mark.parametrize("M,N,lowp", CASES)
def test_exact_factors_every_output_set_against_the_oracle(ops, M, N, lowp):
    assert E.packed_family(M, N) == E.FAMILY[(M, N)]           # (the label in E.PAIRS is the family that runs the pair)
    b, L, R, y = exact_case(M, N, lowp)
    x, Ld, Rd = dev(b, lowp), dev(L, lowp), dev(R, lowp)
    for flags, sigs in [(f, E.SIGS) for f in PACKED_ONLY] + [(f, E.SIGS[:3]) for f in OTHER_SETS]:
        for sig in sigs:
            o = ops.kron_quant(x, Ld, Rd, [sig], flags)
            assert_outputs(o, 0, O.quant_outputs(y, sig[0], sig[1], lowp=lowp, **kw(flags)), flags, lowp, (hex(flags), sig))
    for k in range(0, len(E.SIGS), 3):                  # the multi-clip loop of the packed-only kernels
        o = ops.kron_quant(x, Ld, Rd, E.SIGS[k:k + 3], P | R16)
        for ci, sig in enumerate(E.SIGS[k:k + 3]):
            assert_outputs(o, ci, O.quant_outputs(y, sig[0], sig[1], lowp=lowp, **kw(P | R16)), P | R16, lowp, ("three clips", sig))
    for flags in (P | R16, P | F | T | R16, P | R16 | Q16, P | F | R16 | Q16):   # one scale per 128 elements: FQ_GROUP128 where the dispatch has it, else two launches
        if (M * N) % 128:
            with pytest.raises(ValueError):
                ops.kron_quant(x, Ld, Rd, [E.SIGS[0]], flags, groupsize=128)
            continue
        for sig in E.SIGS[:3]:
            o = ops.kron_quant(x, Ld, Rd, [sig], flags, groupsize=128)
            ref = O.quant_outputs(y, sig[0], sig[1], groupsize=128, lowp=lowp, **kw(flags))
            assert_outputs(o, 0, ref, flags, lowp, ("group 128", hex(flags), sig))


@pytest.mark.parametrize("H", [2, 30, 32, 64])
@pytest.mark.parametrize("transpose_out", [True, False])
@pytest.mark.parametrize("flags,lowp", [(P | NC0, "f16"), (P | NC0 | T | F | R16, "f16"), (P | F | T | R16, "bf16")])
def test_head_transform_exact_against_the_oracle(ops, H, transpose_out, flags, lowp):
    hd = 128
    b = E.batch(hd, H, lowp).reshape(E.N_BATCH, hd, H)
    Pm = E.exact_factors(H, H, lowp)[0]
    x, Pd = dev(b, lowp), dev(Pm, lowp)
    for sig in (E.SIGS if flags == P | NC0 else E.SIGS[:3]):
        o = ops.block_quant(x, Pd, [sig], flags, transpose_out=transpose_out)
        ref = O.block_quant(b, Pm, sig[0], sig[1], transpose_out=transpose_out, lowp=lowp, **kw(flags))
        assert_outputs(o, 0, ref, flags, lowp, (H, sig))


# each edge row (odd positions) alone in its group (1), first (5, 9, 13, 21), last (3, 7, 11, 15, 19) or inside (17, 23); one empty group
GROUP_OFFSETS = [0, 1, 2, 2, 4, 5, 8, 9, 12, 13, 16, 20, 21, 25]


@pytest.mark.parametrize("M,N", [(64, 64), (64, 128)])
@pytest.mark.parametrize("flags,lowp", [(P | NC0, "f16"), (P | F | T | R16, "f16"), (P, "bf16")])
def test_grouped_launch_exact_against_the_oracle(ops, M, N, flags, lowp):
    b, L, R, _ = exact_case(M, N, lowp)
    G = len(GROUP_OFFSETS) - 1
    smax = np.array([E.SIGS[g % len(E.SIGS)][0] for g in range(G)], np.float32)
    smin = np.array([E.SIGS[g % len(E.SIGS)][1] for g in range(G)], np.float32)
    offs = torch.tensor(GROUP_OFFSETS, dtype=torch.int64, device="cuda")
    o = ops.kron_quant_grouped(dev(b, lowp), dev(L, lowp), dev(R, lowp), offs, dev(smax), dev(smin), flags)
    ref = O.kron_quant_grouped(b, L, R, GROUP_OFFSETS, smax, smin, lowp=lowp, **kw(flags))
    assert_outputs(o, 0, ref, flags, lowp, "grouped")


# ------------------------------------------------------------------------------------------------ (b) random factors, the families' own bar

@pytest.mark.parametrize("M,N,lowp", CASES)
def test_random_factors_quantiser_exact_on_the_kernels_own_transform(ops, M, N, lowp):
    b = E.batch(M, N, lowp)
    x, (Ld, Rd) = dev(b, lowp), [dev(m, lowp) for m in E.random_factors(M, N, lowp)]
    to32 = lambda t: O.bf16_from_bits(bits16(t)) if lowp == "bf16" else t.cpu().numpy().astype(np.float32)
    flags = T | P | F | R16
    o = ops.kron_quant(x, Ld, Rd, E.SIGS[:3], flags)
    y = to32(o.y)
    assert np.isfinite(y).all()
    for ci, sig in enumerate(E.SIGS[:3]):
        ref = O.quant_outputs(y, sig[0], sig[1], lowp=lowp, **kw(flags))
        assert_outputs(o, ci, ref, P | F, lowp, ("T|P|F|R16", sig))
    yT = to32(ops.kron_quant(x, Ld, Rd, flags=T).y)
    for flags in (P | R16, P | NC0 | R16, P | R16 | Q16):
        for sig in E.SIGS:
            o = ops.kron_quant(x, Ld, Rd, [sig], flags)
            assert_outputs(o, 0, O.quant_outputs(yT, sig[0], sig[1], lowp=lowp, **kw(flags)), flags, lowp, (hex(flags), sig))


# ------------------------------------------------------------------------------------------------ (c) position and neighbour independence

def independence(call, x, big, others=()):
    """`call(x, *others)` -> outputs with one leading row per row of x. Rolled by 1 and 2 rows; tiled to `big` rows (row i = x[i % 25])."""
    n = x.shape[0]
    base = raw(call(x, *others))
    assert base
    for k in (1, 2):
        got = raw(call(*(torch.roll(t, k, 0).contiguous() for t in (x,) + tuple(others))))
        for a, g in zip(base, got):
            assert torch.equal(g.reshape(n, -1), torch.roll(a.reshape(n, -1), k, 0)), ("rolled by", k)
    idx = torch.arange(big, device=x.device) % n
    got = raw(call(*(t[idx].contiguous() for t in (x,) + tuple(others))))
    for a, g in zip(base, got):
        assert torch.equal(g.reshape(big, -1), a.reshape(n, -1)[idx]), ("tiled to", big)
    return base


@pytest.mark.parametrize("M,N,lowp", CASES)
@pytest.mark.parametrize("flags", INDEP_SETS)
def test_outputs_do_not_depend_on_position_or_neighbours(ops, M, N, lowp, flags):
    x, (Ld, Rd) = dev(E.batch(M, N, lowp), lowp), [dev(m, lowp) for m in E.random_factors(M, N, lowp)]
    independence(lambda t: ops.kron_quant(t, Ld, Rd, INDEP_SIGS, flags), x, big_rows(M, N, flags))


@pytest.mark.parametrize("M,N,lowp", CASES)
@pytest.mark.parametrize("flags", INDEP_SETS)
def test_nonfinite_rows_leave_every_other_row_alone(ops, M, N, lowp, flags):
    b = E.batch(M, N, lowp)
    bad, zeroed = E.nonfinite(b), b.copy()
    zeroed[list(E.NONFINITE_ROWS)] = 0
    Ld, Rd = [dev(m, lowp) for m in E.random_factors(M, N, lowp)]
    call = lambda t: ops.kron_quant(t, Ld, Rd, INDEP_SIGS, flags)
    n, big = E.N_BATCH, big_rows(M, N, flags)
    keep = torch.tensor([i for i in range(n) if i not in E.NONFINITE_ROWS], device="cuda")
    want = [a.reshape(n, -1) for a in raw(call(dev(zeroed, lowp)))]
    xb = dev(bad, lowp)
    for k in (0, 1, 2):
        got = raw(call(torch.roll(xb, k, 0).contiguous()))
        torch.cuda.synchronize()                                                   # the call returns
        for a, g in zip(want, got):
            assert torch.equal(g.reshape(n, -1)[(keep + k) % n], a[keep]), ("rolled by", k)
    idx = torch.arange(big, device="cuda") % n
    sel = torch.isin(idx, keep)
    got = raw(call(xb[idx].contiguous()))
    torch.cuda.synchronize()
    for a, g in zip(want, got):
        assert torch.equal(g.reshape(big, -1)[sel], a[idx][sel]), ("tiled to", big)


# the launches whose prologue is not exact: (c) only

@pytest.mark.parametrize("M,N,flags", [(64, 64, P), (64, 64, P | T | R16), (64, 128, P), (56, 64, P | NC0)])
def test_rmsnorm_launch_independence(ops, M, N, flags):
    x, (Ld, Rd) = dev(E.batch(M, N)), [dev(m) for m in E.random_factors(M, N)]
    independence(lambda t: ops.rmsnorm_kron_quant(t, 1e-5, Ld, Rd, INDEP_SIGS, flags), x, big_rows(M, N, flags))


@pytest.mark.parametrize("M,N", [(112, 128), (128, 128), (128, 224)])
@pytest.mark.parametrize("flags", [P, P | Q16 | R16, P | F | T | R16])
def test_silu_mul_launch_independence(ops, M, N, flags):
    """also at 5 rows (the rows <= 64 build of 128 x 128) and at 67 rows (its neighbour build): the same bytes per token"""
    gate = dev(E.batch(M, N))
    up = dev((np.random.default_rng([M, N, 9]).standard_normal((E.N_BATCH, M * N)) * 0.5).astype(np.float16))     # (15000 x up stays finite)
    Ld, Rd = [dev(m) for m in E.random_factors(M, N)]
    call = lambda g, u: ops.silu_mul_kron_quant(g, u, Ld, Rd, INDEP_SIGS, flags)
    base = independence(call, gate, big_rows(M, N, flags | F), others=(up,))             # (519 above 32 KB: two inputs)
    for rows in (5, 67):
        idx = torch.arange(rows, device="cuda") % E.N_BATCH
        for a, g in zip(base, raw(call(gate[idx].contiguous(), up[idx].contiguous()))):
            assert torch.equal(g.reshape(rows, -1), a.reshape(E.N_BATCH, -1)[idx]), rows


@pytest.mark.parametrize("K,Pw", [(172, 64), (28, 512)])                                 # 11008 and 14336
def test_hadamard_launch_independence(ops, K, Pw):
    x, h = dev(E.batch(K, Pw)), torch.from_numpy(hadk_matrix(K)).cuda()
    for route in (None, "fwht", "kron"):
        independence(lambda t: ops.hadamard_quant(t, K, h, E.SIGS[2], route=route), x, BIG)
    if ops.had_mfma_supported(K * Pw, K):
        independence(lambda t: ops.hadamard_mfma(t, K, h, E.SIGS[2], None, True), x, BIG)
        independence(lambda t: ops.hadamard_mfma(t, K, h, None, None, True), x, BIG)
    else:
        with pytest.raises(ValueError):
            ops.hadamard_mfma(x, K, h, E.SIGS[2], None, True)
