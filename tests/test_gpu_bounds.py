"""Every launch stays inside its buffers and writes all of them (tests/guards.py does the allocating).

One driver, `drive()`, per case:
  1. the call on plain inputs with the product's plain allocator -> `want`;
  2. the caches cleared, the product's `torch` replaced by the guard proxy (poison 0x5A), the inputs copied between pads that would change a
     result if read (NaN / 0xFF; index tensors: valid entries), the call, `check()`; again with 0xA5 and the other input pads;
  3. CONTAINMENT: every pad of every buffer the call allocated — outputs, workspaces, fragment images, blobs, scratch — is intact;
     COMPLETE WRITE: every returned output is bit-identical under both poisons and to `want` (raw bytes);
     NO READ THAT MATTERS: the same equality, because the input pads differ between the two guarded runs;
  4. where a case holds a size no other test of its family holds to the oracle, the family's own parity bar on the same call's outputs
     (quantiser bit-exact on the kernel's own transform; transform within 1e-3 of the row maximum; GEMMs bit-exact against the integer product).

Where the library refuses a shape the refusal is the assertion: the guarded call must refuse too and its outputs must still be all poison.

No case provokes a fault: every shape, index and alignment here is one a correct kernel serves inside its allocations; the guards only make an
overrun land in memory the test owns.

Row counts: 1, 2 / 3, around one tile, and per family one count ABOVE THE LAUNCHER'S OWN GRID CAP (n_cu = 256 on the MI355X) that is no multiple of a
workgroup's token count, so that the persistent / grid-stride second pass runs under the guard. The caps, as the launchers state them:
  * 64 x 64: 4 tokens x n_cu; trio / duo / tiles: 3 / 2 / <= 4 token groups x n_cu; workgroup-per-token, general, tall, fq_hadamard.hip and the
    K-factor Hadamard kernel: <= 4 workgroups x n_cu, one token each -> BIG = 1031 (prime) passes all of them (tpb = 5 where it is <= 4);
  * wave-per-token Kronecker kernels: W = 7 .. 16 waves x n_cu, one token per wave -> WAVE_BIG = 4099 (prime; tokens per block 17: no multiple
    of any W, two to three rounds of the slot loop); the structured Hadamard kernel: 2 / 3 groups x n_cu -> 1031;
  * row quantisers: a workgroup per row: 8 n_cu rows -> 2053; a wave per row, fakequant_bits, RMSNorm, the asymmetric route at a wave per row:
    8 n_cu x 4 rows -> 8209; short rows of 2^k lanes: 8 n_cu x 4 x (64 >> k) rows -> 16411 / 32771 / 65543 at 256 / 128 / 64 columns;
  * register FWHT (K = 1): 4 n_cu x 4 x rows-per-wave (2 n_cu at n = 8192) -> 32771 / 16411 / 8209 / 4099 / 2053 rows at n = 64 / 128 / 256 / 512 .. 4096 / 8192;
  * head transform: <= 4 n_cu x 4 blocks -> 4099; single matrix: 8 n_cu x 128 rows -> 262147; kv_quant: 2 n_cu x 128 rows, kv_dequant: 8 n_cu x 256
    16-byte chunks -> 32771 tokens of 2 heads; appends: 16 n_cu x 256 chunks -> 65600 tokens; sym_quant / sym_dequant / silu_mul: 16 n_cu x 256 items;
    int4_to_frag / int4_to_bf6: 16 n_cu x 256 lanes -> a 4096 x 16384 weight.
The cap counts run at the widths whose footprint stays near 100 MB (rows of at most 4096 elements for the wave-per-row kernels; the wider
buckets of the same templates run at 1031 rows, below their cap).

Which cases are held to the ORACLE next to the plain run: the Kronecker cases whose flags hold both T and R16 — the quantiser then reads the rounded
transform the same call returns, so O.quant_outputs on that y must give the same bits, and y itself lies within 1e-3 of the row maximum of
O.kron_transform. Every pair has such a case at 1, 65 and 1031 rows (519 rows for tokens above 32 KB) and every full-cross pair at 3 rows; bf16 at
3 rows. Sets without T (packed-only and fake-quant-only instantiations) and sets without R16 (the quantiser reads the fp32 accumulator, which no
call returns) are held to the plain run of the same call only: their oracle bars live in the families' own files. Row kernels, sym_quant,
sym_dequant, the GEMMs, kv_quant and the head transform are held to their oracles as each test says."""
import numpy as np
import pytest
import torch

from oracle import fq_oracle as O
from tests import guards
from tests.conftest import hadk_matrix, same_bits
from tests.edge_tokens import packed_family

pytestmark = pytest.mark.gpu
P, F, T, R16, NC0, Q16, ASYM = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x800
F16, BF = torch.float16, torch.bfloat16
SIG4 = [(0.9820137619972229, 0.9820137619972229), (0.9, 0.33), (1.0, 1.0), (0.6, 0.95)]
BIG = 1031
WAVE_BIG = 4099


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------ the driver

def _map(obj, fn):
    if isinstance(obj, torch.Tensor):
        return fn(obj)
    if isinstance(obj, (list, tuple)):
        return type(obj)(_map(o, fn) for o in obj)
    return obj


def _outs(r):
    """every tensor a call returned, flattened in a fixed order"""
    if r is None:
        return []
    if isinstance(r, torch.Tensor):
        return [r]
    if isinstance(r, (list, tuple)):
        return [t for o in r for t in _outs(o)]
    if hasattr(r, "q") and hasattr(r, "fq"):                 # ops.FusedOutputs
        return list(r.q) + list(r.scale) + list(r.fq) + _outs(r.y)
    raise TypeError(type(r))


def _is_byte_buffer(rec):
    """images, blobs, workspaces, scratch: flat uint8 allocations (no output of this package is one)"""
    return rec.dtype == torch.uint8 and len(rec.shape) == 1


def drive(ops, call, inputs, pads=None, inout=(), modules=None, after=None, refuse=False):
    """-> (want, guards, guarded inputs per run). `inputs`: name -> tensor / list of tensors / anything else (passed through). `inout`: names
    of inputs the call writes (cloned per run, their final contents compared like outputs). `after(run_inputs, outs)`: extra checks per run.
    `refuse`: the library is meant to refuse this call (FQ_EUNSUPPORTED / FQ_EINVAL): it must, plain and guarded, and write nothing."""
    from flatquant_amd import _lib
    pads = pads or {}
    fresh = lambda: {k: (_map(v, torch.clone) if k in inout else v) for k, v in inputs.items()}
    plain, refused = fresh(), None
    try:
        want = _outs(call(**plain)) + [t for k in inout for t in _outs(plain[k])]
    except _lib.FqError as e:
        refused = e
        if not refuse:
            raise
    assert not refuse or refused is not None, "the library was meant to refuse this call"
    torch.cuda.synchronize()
    got, gs, used = [], [], []
    for poison in guards.POISONS:
        ops.invalidate_caches()
        g = guards.Guard(poison)
        with g.on(*(modules or (ops,))):
            gi = {k: _map(v, lambda t, k=k: g.guard_input(t, pads.get(k, "auto"))) for k, v in fresh().items()}
            if refused is not None:
                with pytest.raises(_lib.FqError):
                    call(**gi)
                out = []
            else:
                out = _outs(call(**gi)) + [t for k in inout for t in _outs(gi[k])]
            torch.cuda.synchronize()
        g.check()                                                                             # containment, every buffer
        if refused is not None:                                                               # a refused call writes nothing
            for rec in g.find("empty"):
                if not _is_byte_buffer(rec):
                    assert bool((rec.buf == poison).all()), ("a refused call wrote to", rec.shape, rec.dtype)
        elif after is not None:
            after(gi, out)
        got.append(out), gs.append(g), used.append(gi)
    if refused is not None:
        return None, gs, used
    assert len(want) == len(got[0]) == len(got[1]) and len(want) > 0
    for i, w in enumerate(want):
        assert guards.same_raw(got[0][i], got[1][i]), (i, tuple(w.shape), "differs between the two poisons: not written completely, or a pad was read")
        assert guards.same_raw(got[0][i], w), (i, tuple(w.shape), "differs from the plain run")
    return want, gs, used


def rnd(shape, seed, dtype=F16, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def packed(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).cuda()


def mats(M, N, seed, dtype=F16):
    return rnd((M, M), seed, dtype, M ** -0.5), rnd((N, N), seed + 1, dtype, N ** -0.5)


def acts(rows, d, seed, dtype=F16):
    x = rnd((rows, d), seed, dtype)
    if rows > 2:
        x[1] *= 30.0
        x[2] = 0
    return x


def bits16(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def sample_rows(rows):
    return list(range(rows)) if rows <= 70 else [0, 1, 2, rows // 2, rows - 4, rows - 3, rows - 2, rows - 1]


def quant_parity(o, x, L, R, sigs, flags, diag=None):
    """the Kronecker families' bars, on the outputs of ONE call that returned its transform (T) and quantised the ROUNDED transform (R16)"""
    if not (flags & T and flags & R16):
        return
    bf = x.dtype == BF
    lowp = "bf16" if bf else "f16"
    idx = sample_rows(x.shape[0])
    ysel = o.y.reshape(x.shape[0], -1)[idx]
    y = O.bf16_from_bits(bits16(ysel)) if bf else ysel.cpu().numpy().astype(np.float32)
    for ci, (a, b) in enumerate(sigs):
        ref = O.quant_outputs(y, a, b, round_y_f16=True, clamp0=not flags & NC0, quant_f16=bool(flags & Q16), lowp=lowp)
        if flags & P:
            assert np.array_equal(o.q[ci][idx].cpu().numpy(), ref["packed"]), (ci, "packed")
            sc = o.scale[ci].reshape(-1)[idx]
            assert np.array_equal(bits16(sc), O.bf16_bits(ref["scale16"])) if bf else np.array_equal(sc.cpu().numpy(), ref["scale16"]), (ci, "scale")
        if flags & F:
            fq = o.fq[ci].reshape(x.shape[0], -1)[idx]
            assert np.array_equal(bits16(fq), O.bf16_bits(ref["fq"])) if bf else same_bits(fq.cpu().numpy(), ref["fq"]), (ci, "fq")
    if not bf:
        to = lambda t: None if t is None else t.cpu().numpy()
        y32 = O.kron_transform(to(x[idx]), to(L), to(R), to(diag)).reshape(len(idx), -1)
        den = np.abs(y32).max(axis=1, keepdims=True) + 1e-30
        assert np.max(np.abs(y - y32) / den) <= 1e-3


# ------------------------------------------------------------------------------------------------ the guard bites on the device too

def test_the_guard_bites_on_the_device():
    mod = guards.standin_module("guards_standin_ops_gpu")
    x = rnd((5, 37), 1)
    outs = []
    for poison in guards.POISONS:
        g = guards.Guard(poison)
        with g.on(mod):
            outs.append((mod.scale_rows(g.guard_input(x)), mod.skips_last_row(g.guard_input(x))))
        g.check()
        assert all(r.buf.is_cuda for r in g.records)
    assert guards.same_raw(outs[0][0], outs[1][0]) and torch.equal(outs[0][0], x * 2)
    assert not guards.same_raw(outs[0][1], outs[1][1]) and guards.same_raw(outs[0][1][:-1], outs[1][1][:-1])     # the unwritten row
    for where, side, off in ((lambda r: r.front + r.nbytes, "back", 5 * 37 * 2), (lambda r: r.front - 1, "front", -1)):
        g = guards.Guard(0x5A)
        with g.on(mod):
            mod.scale_rows(x)
        rec = g.records[0]
        rec.buf[where(rec)] = 0x11                                  # a torch op that writes INSIDE the guarded buffer, one byte off the payload
        with pytest.raises(guards.GuardError, match=f"{side} pad of empty tensor.*first at payload offset {off}, last at {off}"):
            g.check()


# ------------------------------------------------------------------------------------------------ Kronecker + quantise

OUTPUT_SETS = [P, F, T, P | F | T, P | R16, P | NC0, P | Q16 | R16, P | F | T | R16]
FULL_CROSS_PAIRS = [(64, 64), (64, 128), (128, 128), (20, 12)]        # the 64 x 64 path, the wave kernel, the workgroup-per-token table, the general kernel
# the factor pairs, by the kernel family their packed-only fp16 launch runs (tests.edge_tokens.packed_family: asked of the library below)
PAIRS = {
    "k64": [(64, 64)],
    "wave": [(64, 128), (64, 112), (64, 80), (56, 64), (32, 64)],
    "trio": [(112, 128), (128, 128)],
    "duo": [(128, 224)],
    # every row of the tiles kernel's lists (csrc/fq_kron_route.hpp): both L depths (ceil(M / 16)) of N = 112 / 144 / 148 / 176 / 128, and 144 x 192;
    # N = 64, 64 < M <= 192 (the pairs of fq_kron_tall.hip, on this kernel since round 5): every row (MT, ceil(M / 16)) = (3,5) (3,6) (4,7) (4,8)
    # (5,9) (5,10) (6,11) (6,12). fq_kron_tall_kernel itself runs where a case asks for the fp32 quantiser WITH the transform (ROW_SETS has none:
    # tests/test_gpu_kron_tall.py) or the rotation alone at M > 160 ((3, T, 1, False) at 172 x 64 and 192 x 64).
    "tiles": [(80, 112), (96, 112), (128, 144), (112, 144), (128, 148), (112, 148), (144, 192), (168, 176), (178, 176), (86, 128), (80, 128),
              (96, 128), (100, 144), (80, 64), (96, 64), (112, 64), (128, 64), (140, 64), (160, 64), (172, 64), (192, 64)],
    "table": [(112, 256), (32, 48), (37, 64)],
    "general": [(2, 2), (3, 6), (20, 12), (60, 62), (130, 16), (129, 254), (256, 128)],
}
FAMILY = {mn: fam for fam, pairs in PAIRS.items() for mn in pairs}
# 37 x 64: 37 rows of eight 16-byte pieces are no whole number of waves' lanes — the wave kernel declines, the workgroup-per-token table takes it
WAVE_TEST_PAIRS = PAIRS["wave"] + [(37, 64)]
# (rows, flags, clip sets, diag): every output set at some row count, the multi-clip loops, the instantiations with a compile-time output set
ROW_SETS = [(1, P | F | T | R16, 4, False), (3, T, 1, False), (65, P | R16, 4, False), (65, P | Q16 | R16, 1, False), (65, P | NC0, 1, True),
            (65, P | F | T | R16, 2, False), (BIG, P, 1, False), (BIG, P | F | T | R16, 1, False)]


def kron_case(ops, M, N, rows, flags, n_clips, diag, dtype=F16, groupsize=-1):
    L, R = mats(M, N, M * 1000 + N, dtype)
    x = acts(rows, M * N, rows + M + N, dtype)
    dg = (rnd((M * N,), 5, dtype, 0.25) + 1.0).to(dtype) if diag else None
    sigs = SIG4[:n_clips]
    res = []

    def call(x, L, R, dg):
        o = ops.kron_quant(x, L, R, sigs, flags, diag=dg, groupsize=groupsize)
        res.append(o)
        return o

    drive(ops, call, dict(x=x, L=L, R=R, dg=dg))
    if groupsize < 0:
        quant_parity(res[0], x, L, R, sigs, flags, dg)


@pytest.mark.parametrize("M,N", FULL_CROSS_PAIRS)
@pytest.mark.parametrize("diag", [False, True])
@pytest.mark.parametrize("n_clips", [1, 4])
@pytest.mark.parametrize("flags", OUTPUT_SETS)
def test_kron_every_output_set(ops, M, N, flags, n_clips, diag):
    kron_case(ops, M, N, 3, flags, n_clips, diag)


@pytest.mark.parametrize("rows,flags,n_clips,diag", ROW_SETS)
@pytest.mark.parametrize("M,N", [mn for fam in PAIRS.values() for mn in fam])
def test_kron_every_family_at_the_rows_with_tails(ops, M, N, rows, flags, n_clips, diag):
    assert packed_family(M, N) == FAMILY[(M, N)]                     # (the label in PAIRS is the family that runs the pair)
    if rows == BIG and flags & F and M * N > 16384:
        rows = 519                                                   # (footprint: the 16-bit outputs of tokens above 32 KB)
    kron_case(ops, M, N, rows, flags, n_clips, diag)


@pytest.mark.parametrize("M,N", WAVE_TEST_PAIRS)
@pytest.mark.parametrize("flags,n_clips", [(P, 1), (P | NC0, 4), (F | R16, 1), (T, 1)])
def test_kron_wave_kernels_beyond_one_token_per_wave(ops, M, N, flags, n_clips):
    """W waves x n_cu workgroups hold at most 16 x 256 tokens at a time: at 4099 rows every workgroup gets 17 tokens and its waves run the slot
    loop two to three times (the counted waits, the next slot's pull, the next token's load under this one's stores)"""
    kron_case(ops, M, N, WAVE_BIG, flags, n_clips, False)


@pytest.mark.parametrize("M,N", [(64, 128), (64, 112), (56, 64), (64, 80), (32, 64)])
@pytest.mark.parametrize("n_clips", [1, 3])
def test_rmsnorm_wave_kernels_beyond_one_token_per_wave(ops, M, N, n_clips):
    L, R = mats(M, N, 61)
    drive(ops, lambda **k: ops.rmsnorm_kron_quant(k["x"], 1e-5, k["L"], k["R"], SIG4[:n_clips], P), dict(x=acts(WAVE_BIG, M * N, 63), L=L, R=R))


@pytest.mark.parametrize("M,N", [(96, 128), (128, 128), (128, 224), (112, 256), (80, 112), (128, 144), (144, 192), (168, 176)])
@pytest.mark.parametrize("rows", [3, 65])
def test_kron_table_low_precision_quantiser_with_diag(ops, M, N, rows):
    """a diag keeps the launch off the token-group kernels: the workgroup-per-token table's packed fp16-quantiser instantiations (MT >= 3)"""
    kron_case(ops, M, N, rows, P | Q16 | R16, 1, True)


@pytest.mark.parametrize("M,N", WAVE_TEST_PAIRS)
@pytest.mark.parametrize("rows", [2, BIG])
def test_kron_wave_fake_quant_only(ops, M, N, rows):
    kron_case(ops, M, N, rows, F | R16, 1, False)


@pytest.mark.parametrize("M,N", [(64, 64), (64, 128), (128, 224), (86, 128), (112, 128), (128, 128), (128, 144), (80, 112), (128, 148), (144, 192),
                                 (168, 176), (172, 64), (20, 12), (2, 2)])
@pytest.mark.parametrize("rows,flags,n_clips", [(3, P | F | T | R16, 4), (65, P, 1), (BIG, P | R16, 1)])
def test_kron_bf16(ops, M, N, rows, flags, n_clips):
    kron_case(ops, M, N, rows, flags, n_clips, False, BF)


@pytest.mark.parametrize("rows", [1, 3, 65, BIG])
@pytest.mark.parametrize("flags,n_clips", [(P, 1), (P | NC0, 4), (P | F | T | R16, 2)])
def test_kron64_without_its_workspace(ops, monkeypatch, rows, flags, n_clips):
    """the 64 x 64 launch with no 32 KB image: the fragments are gathered from the matrices"""
    monkeypatch.setitem(ops._WS_BYTES, (64, 64), 0)
    kron_case(ops, 64, 64, rows, flags, n_clips, False)


@pytest.mark.parametrize("M,N,flags", [(64, 64, P), (32, 64, P), (56, 64, P), (64, 128, P | R16), (64, 112, P | F | R16), (32, 64, F | R16),
                                        (112, 128, P | R16), (128, 128, P | F | T | R16), (60, 62, P | R16), (20, 12, P)])
@pytest.mark.parametrize("rows", [1, 3, 65, BIG])
def test_kron_group128_both_forms(ops, M, N, flags, rows):
    """FQ_GROUP128: the packed fp32 launch at N = 64, the group epilogue with R16; a pair without either takes the two launches or is refused"""
    if (M * N) % 128:
        with pytest.raises(ValueError):
            ops.kron_quant(acts(1, M * N, 1), *mats(M, N, 1), [(1.0, 1.0)], flags, groupsize=128)
        return
    kron_case(ops, M, N, rows, flags, 1, False, groupsize=128)


GROUP_OFFSETS = [0, 0, 5, 5, 70, 130, 130, 131]      # empty groups (first, middle, next to last), boundaries inside a workgroup's tokens, one row at the very end


@pytest.mark.parametrize("M,N", [(32, 64), (64, 64), (64, 128), (128, 128), (20, 12)])
@pytest.mark.parametrize("per_group_mats", [False, True])
@pytest.mark.parametrize("flags,dtype", [(P | NC0, F16), (P | F | T | R16, F16), (P, BF)])
def test_kron_grouped(ops, M, N, per_group_mats, flags, dtype):
    G = len(GROUP_OFFSETS) - 1
    rows = GROUP_OFFSETS[-1]
    x = acts(rows, M * N, 3, dtype)
    if per_group_mats:
        L, R = rnd((G, M, M), 7, dtype, M ** -0.5), rnd((G, N, N), 8, dtype, N ** -0.5)
    else:
        L, R = mats(M, N, 9, dtype)
    offs = torch.tensor(GROUP_OFFSETS, dtype=torch.int64, device="cuda")
    smax = torch.linspace(0.6, 1.0, G, device="cuda", dtype=torch.float32)
    smin = torch.linspace(1.0, 0.5, G, device="cuda", dtype=torch.float32)
    drive(ops, lambda **k: ops.kron_quant_grouped(k["x"], k["L"], k["R"], k["offs"], k["smax"], k["smin"], flags),
          dict(x=x, L=L, R=R, offs=offs, smax=smax, smin=smin), pads={"offs": "repeat"},
          refuse=per_group_mats and (M, N) == (20, 12))                       # per-group matrices: the workgroup-per-token kernels only


@pytest.mark.parametrize("M,N", [(172, 64), (112, 128), (112, 256), (128, 224), (64, 128), (64, 64)])
@pytest.mark.parametrize("rows", [1, 3, 65, 519])
@pytest.mark.parametrize("flags,with_up", [(P | Q16 | R16, False), (T | R16, False), (P | T | R16, False), (P | Q16 | R16, True)])
def test_kron_ex_post_scale(ops, M, N, rows, flags, with_up):
    L, R = mats(M, N, 21)
    x = acts(rows, M * N, 22)
    up = acts(rows, M * N, 23) if with_up else None
    refuse = with_up and (M, N) in ((172, 64), (64, 128), (64, 64))        # the SiLU.mul input is fused for the down_proj pairs (M > 64, N >= 128) only
    drive(ops, lambda **k: ops.kron_quant_ex(k["x"], k["L"], k["R"], 0.125, [(0.9, 1.0)], flags, up=k["up"]), dict(x=x, L=L, R=R, up=up), refuse=refuse)


@pytest.mark.parametrize("dtype", [F16, BF])
def test_kron_multi_job_launch(ops, dtype):
    """KronMultiPlan: jobs of different row counts; the job table, the images and the outputs are allocated under the guard"""
    rows = [1, 7, 40, 3, 129]
    xs = [acts(r, 4096, 30 + r, dtype) for r in rows]
    Ls = [rnd((64, 64), 40 + j, dtype, 0.125) for j in range(len(rows))]
    Rs = [rnd((64, 64), 50 + j, dtype, 0.125) for j in range(len(rows))]
    keep = []

    def call(xs, Ls, Rs):
        keep.append(ops.KronMultiPlan(xs, Ls, Rs, (0.9, 0.8), P | NC0))
        return keep[-1].run()

    want, _, _ = drive(ops, call, dict(xs=xs, Ls=Ls, Rs=Rs))
    for j in range(len(rows)):
        one = ops.kron_quant(xs[j], Ls[j], Rs[j], [(0.9, 0.8)], P | NC0)
        assert torch.equal(one.q[0], want[j]) and guards.same_raw(one.scale[0], want[len(rows) + j])


@pytest.mark.parametrize("M,N", [(64, 64), (64, 128), (64, 112), (56, 64), (64, 80), (32, 64), (128, 128)])
@pytest.mark.parametrize("rows", [1, 3, 65, BIG])
@pytest.mark.parametrize("flags,n_clips", [(P, 1), (P | NC0, 4), (P | T | R16, 1)])
def test_rmsnorm_kron_quant(ops, M, N, rows, flags, n_clips):
    L, R = mats(M, N, 61)
    x = acts(rows, M * N, 62)
    drive(ops, lambda **k: ops.rmsnorm_kron_quant(k["x"], 1e-5, k["L"], k["R"], SIG4[:n_clips], flags), dict(x=x, L=L, R=R))


@pytest.mark.parametrize("M,N", [(128, 128), (96, 128), (128, 224), (112, 256), (64, 128)])
@pytest.mark.parametrize("rows", [1, 3, 64, 65, 519])
@pytest.mark.parametrize("flags,n_clips", [(P, 1), (P | Q16 | R16, 1), (P | F | T | R16, 4)])
def test_silu_mul_kron_quant(ops, M, N, rows, flags, n_clips):
    """the FQ_FS table (rows <= 64: the eight-wave build of 128 x 128, and its rows = 65 neighbour); 64 x 128 takes silu_mul + kron_quant"""
    L, R = mats(M, N, 71)
    gate, up = acts(rows, M * N, 72), acts(rows, M * N, 73)
    drive(ops, lambda **k: ops.silu_mul_kron_quant(k["gate"], k["up"], k["L"], k["R"], SIG4[:n_clips], flags), dict(gate=gate, up=up, L=L, R=R))


@pytest.mark.parametrize("tokens", [1, 7, 8, 16])
@pytest.mark.parametrize("eps", [None, 1e-5])
def test_kron64_linear_multi(ops, tokens, eps):
    L, R = mats(64, 64, 81)
    x = acts(tokens, 4096, 82)
    Ns = [64, 96, 2048]
    ws = [packed((N, 2048), 83 + N) for N in Ns]
    imgs = [ops.int4_to_frag(w) for w in ws]
    wsc = [(rnd((N,), 84 + N).abs() * 0.01 + 0.001).half() for N in Ns]
    bias = [rnd((Ns[0],), 85), None, rnd((Ns[2],), 86)]

    def call(x, L, R, imgs, wsc, bias):
        ys = ops.kron64_linear_multi(x, L, R, SIG4[:3], list(zip(imgs, wsc, bias)), eps, NC0)
        assert ys is not None
        return ys

    want, _, _ = drive(ops, call, dict(x=x, L=L, R=R, imgs=imgs, wsc=wsc, bias=bias))
    xin = ops.rmsnorm(x, eps) if eps is not None else x
    o = ops.kron_quant(xin, L, R, SIG4[:3], P | NC0)
    for p in range(3):
        assert guards.same_raw(want[p], ops.int4_skinny_linear(o.q[p], o.scale[p], imgs[p], wsc[p], bias[p], Ns[p]))


def test_launch_plans_allocate_under_the_guard(ops):
    """LaunchPlan (static outputs) and FreshPlan (fresh outputs per run), built while the proxy is installed"""
    L, R = mats(64, 128, 91)
    x = acts(37, 8192, 92)
    keep = []

    def static(x, L, R):
        keep.append(ops.kron_plan(x, L, R, SIG4[:2], P | NC0))
        return keep[-1].run(x)

    def fresh(x, L, R):
        keep.append(ops.kron_fresh_plan(x, L, R, SIG4[0], P | NC0, (37, 4096), (37,)))
        return keep[-1].run(x)

    def rq_static(x):
        keep.append(ops.rowquant_plan(x, SIG4[:2], P | F))
        return keep[-1].run(x)

    def rq_fresh(x):
        keep.append(ops.rowquant_fresh_plan(x, SIG4[0], P, (37, 4096), (37,)))
        return keep[-1].run(x)

    drive(ops, static, dict(x=x, L=L, R=R))
    drive(ops, fresh, dict(x=x, L=L, R=R))
    drive(ops, rq_static, dict(x=x))
    drive(ops, rq_fresh, dict(x=x))


# ------------------------------------------------------------------------------------------------ head transform / single matrix

@pytest.mark.parametrize("H", [2, 28, 40, 64])
@pytest.mark.parametrize("transpose_out", [True, False])
@pytest.mark.parametrize("rows", [1, 3, 700])
@pytest.mark.parametrize("flags,dtype", [(P | NC0 | T | F | R16, F16), (P | NC0, F16), (P | F | T | R16, BF)])
def test_block_quant(ops, H, transpose_out, rows, flags, dtype):
    hd = 128
    x = rnd((rows, hd, H), H + rows, dtype)
    Pm = rnd((H, H), H, dtype, H ** -0.5)
    sigs = [(0.982, 0.982), (0.6, 0.95)]
    res = []

    def call(x, Pm):
        res.append(ops.block_quant(x, Pm, sigs, flags, transpose_out=transpose_out))
        return res[-1]

    drive(ops, call, dict(x=x, Pm=Pm))
    if not flags & T:
        return
    o, lowp, idx = res[0], "bf16" if dtype == BF else "f16", sample_rows(rows)     # the heads file's bar, on rows 1 / 3 / 700 and H = 2
    ysel = o.y.reshape(rows, -1)[idx]
    y = O.bf16_from_bits(bits16(ysel)) if dtype == BF else ysel.cpu().numpy().astype(np.float32)
    for ci, (a, b) in enumerate(sigs):
        ref = O.quant_outputs(y, a, b, round_y_f16=True, clamp0=not flags & NC0, lowp=lowp)
        assert np.array_equal(o.q[ci][idx].cpu().numpy(), ref["packed"]), (ci, "packed")
        fq = o.fq[ci].reshape(rows, -1)[idx]
        assert np.array_equal(bits16(fq), O.bf16_bits(ref["fq"])) if dtype == BF else same_bits(fq.cpu().numpy(), ref["fq"]), (ci, "fq")


@pytest.mark.parametrize("H,flags,dtype", [(28, P | NC0 | T | F | R16, F16), (40, P | NC0, F16), (64, P | NC0, F16), (64, T, F16), (40, P | F | R16, BF), (2, P, F16)])
@pytest.mark.parametrize("transpose_out", [True, False])
def test_block_quant_beyond_the_grid_cap(ops, H, flags, dtype, transpose_out):
    """at most 4 n_cu workgroups of 4 blocks: at 4099 blocks every workgroup strides on"""
    x, Pm = rnd((4099, 128, H), H, dtype), rnd((H, H), H + 1, dtype, H ** -0.5)
    drive(ops, lambda x, Pm: ops.block_quant(x, Pm, [(0.982, 0.9)], flags, transpose_out=transpose_out), dict(x=x, Pm=Pm))


@pytest.mark.parametrize("n", [64, 128])
@pytest.mark.parametrize("rows", [1, 3, 700, BIG * 5, 262147])
@pytest.mark.parametrize("dtype", [F16, BF])
def test_single_trans(ops, n, rows, dtype):
    drive(ops, lambda x, m: ops.single_trans(x, m), dict(x=rnd((rows, n), n + rows, dtype), m=rnd((n, n), n, dtype, n ** -0.5)))


# ------------------------------------------------------------------------------------------------ row kernels

ROWQ_CAP = {64: 65543, 128: 32771, 256: 16411, 512: 8209, 4096: 8209, 16384: 2053}     # above each route's grid cap (module docstring)


@pytest.mark.parametrize("cols,rows", [(c, r) for c in [64, 128, 256, 512, 4096, 11008, 16384, 32768]        # MULTI short rows; a wave per row; a workgroup per row
                                       for r in [1, 3, 65, BIG] + ([ROWQ_CAP[c]] if c in ROWQ_CAP else [])])
@pytest.mark.parametrize("flags,n_clips,dtype", [(P, 1, F16), (P | F, 4, F16), (F | Q16, 2, F16), (F | ASYM, 1, F16), (P | F, 2, BF),
                                                 (F | ASYM | Q16, 1, BF)])
def test_rowquant(ops, cols, rows, flags, n_clips, dtype):
    if rows == BIG and cols > 16384:
        rows = 519
    if rows > BIG:
        n_clips = min(n_clips, 2)                                        # (footprint of the 16-bit outputs at the cap counts)
    x = acts(rows, cols, cols + rows, dtype)
    res = []

    def call(x):
        res.append(ops.rowquant(x, SIG4[:n_clips], flags))
        return res[-1]

    drive(ops, call, dict(x=x))
    if dtype == F16 and not flags & (ASYM | Q16):  # the row quantiser's bar: bit-exact against the oracle
        idx = sample_rows(rows)
        for ci, (a, b) in enumerate(SIG4[:n_clips]):
            ref = O.rowquant(x[idx].cpu().numpy(), a, b)
            if flags & P:
                assert np.array_equal(res[0].q[ci][idx].cpu().numpy(), ref["packed"])
                assert np.array_equal(res[0].scale[ci][idx].cpu().numpy(), ref["scale16"])
            if flags & F:
                assert same_bits(res[0].fq[ci][idx].cpu().numpy(), ref["fq"])


@pytest.mark.parametrize("cols,rows", [(c, r) for c in [64, 128, 4096, 11008] for r in [1, 3, BIG] + ([8209] if c in (128, 4096) else [])])
@pytest.mark.parametrize("nbits", [2, 3, 8])
@pytest.mark.parametrize("flags,dtype", [(0, F16), (ASYM, F16), (Q16, BF)])
def test_fakequant_bits(ops, cols, rows, nbits, flags, dtype):
    drive(ops, lambda x: ops.fakequant_bits(x, (0.9, 0.8), nbits, flags), dict(x=acts(rows, cols, cols + rows, dtype)))


@pytest.mark.parametrize("cols,rows", [(c, r) for c in [8, 4096, 1, 7, 127] for r in [1, 3, 65, BIG]] + [(4096, 2063), (127, 16411)])   # the last two: above 16 n_cu x 256 items
def test_sym_quant(ops, cols, rows):
    """odd cols: the destination is (cols + 1) // 2 bytes wide and the last byte's high nibble is 0 under both poisons"""
    x = acts(rows, cols, cols + rows)
    scale = (x.float().abs().amax(1) / 7 + 0.01).half()
    want, _, _ = drive(ops, lambda x, scale: ops.sym_quant(x, scale), dict(x=x, scale=scale))
    assert want[0].shape == (rows, (cols + 1) // 2)
    assert np.array_equal(want[0].cpu().numpy(), O.sym_quant(x.cpu().numpy(), scale.cpu().numpy()))
    if cols & 1:
        assert not bool((want[0][:, -1] >> 4).any())


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 7), (65, 24), (257, 272), (BIG, 4096)])
def test_sym_dequant(ops, rows, cols):
    g = torch.Generator().manual_seed(rows)
    q = torch.randint(-30000, 30000, (rows, cols), generator=g, dtype=torch.int32).cuda()
    sr, sc = rnd((rows,), 1).abs() * 0.01, rnd((cols,), 2).abs() * 0.01
    want, _, _ = drive(ops, lambda q, sr, sc: ops.sym_dequant(q, sr, sc), dict(q=q, sr=sr, sc=sc), pads={"q": "zeros"})
    assert same_bits(want[0].cpu().numpy(), O.sym_dequant(q.cpu().numpy(), sr.cpu().numpy(), sc.cpu().numpy()).astype(np.float16))


@pytest.mark.parametrize("cols", [8, 2048, 4096, 8192, 11008, 16384])          # each FQ_RN bucket (4, 8, 16, 32 chunks per lane) and the smallest row
@pytest.mark.parametrize("rows", [1, 3, 5, BIG * 2 + 1, 8209])
def test_rmsnorm(ops, cols, rows):
    if cols > 4096 and rows > BIG:
        rows = BIG                                                       # (footprint; the cap count 8209 runs at rows of up to 4096 elements)
    drive(ops, lambda x: ops.rmsnorm(x, 1e-5), dict(x=acts(rows, cols, cols + rows)))


def test_rmsnorm_refuses_what_it_cannot_run(ops):
    drive(ops, lambda x: ops.rmsnorm(x, 1e-5), dict(x=acts(3, 12, 1)), refuse=True)            # cols % 8 != 0
    drive(ops, lambda x: ops.rmsnorm(x, 1e-5), dict(x=acts(3, 16392, 1)), refuse=True)         # cols > 16384


@pytest.mark.parametrize("shape", [(1, 8), (3, 4096), (65, 11008), (BIG * 9, 1024)])     # the last: above 16 n_cu x 256 chunks
def test_silu_mul(ops, shape):
    gate, up = rnd(shape, 1), rnd(shape, 2)
    drive(ops, lambda gate, up: ops.silu_mul(gate, up), dict(gate=gate, up=up))


# ------------------------------------------------------------------------------------------------ Hadamard

def hk(K):
    """the K x K sign factor: the shipped tables, Sylvester's construction for powers of two"""
    if K == 1:
        return None
    if K & (K - 1) == 0:
        from flatquant_amd import ops as _ops
        return _ops._sylvester(K).half().cuda()
    return torch.from_numpy(hadk_matrix(K)).cuda()


# (K, P): the register kernels (P = 64 .. 8192, K = 1: rows per wave 8 / 4 / 2 / 1; K > 1: the K-factor kernel, P = 512 / 1024 and the short
# vectors), fq_hadamard.hip for everything else (P = 32, 16384; K x 2048), the Kronecker forms (172 x 64, 112 x 128) and the structured kernel
HAD_SHAPES = [(1, 32), (1, 64), (1, 128), (1, 256), (1, 512), (1, 1024), (1, 2048), (1, 4096), (1, 8192), (1, 16384),
              (12, 512), (28, 1024), (20, 256), (40, 128), (172, 64), (12, 2048), (36, 32), (28, 512), (60, 512), (108, 128)]


@pytest.mark.parametrize("K,Pw,fwht", [(K, Pw, True) for K, Pw in HAD_SHAPES] + [(K, Pw, False) for K, Pw in HAD_SHAPES if K > 1])
@pytest.mark.parametrize("rows", [1, 3, 37])
def test_hadamard_rotation(ops, K, Pw, rows, fwht):
    """fwht: the register / LDS kernels; otherwise the matrix-pipe route where the shape has one (K = 1 has the one route)"""
    x = acts(rows, K * Pw, K + Pw + rows)
    drive(ops, lambda x, h: ops.hadamard(x, K, h, fwht_route=fwht), dict(x=x, h=hk(K)))


HAD_CAP = [(1, 64, 32771), (1, 128, 16411), (1, 256, 8209), (1, 512, 4099), (1, 1024, 4099), (1, 2048, 4099), (1, 4096, 4099), (1, 8192, 2053),
           (1, 32, BIG), (1, 16384, BIG), (12, 512, BIG), (28, 1024, BIG), (20, 256, BIG), (40, 128, BIG), (172, 64, BIG), (12, 2048, BIG)]


@pytest.mark.parametrize("K,Pw,rows", HAD_CAP)
def test_hadamard_beyond_the_grid_cap(ops, K, Pw, rows):
    """the rotation, the fp32-out transform (K = 1, 64 <= n <= 8192) and the fused Quantizer (+ SiLU.mul input) where the register kernels have
    them, at a row count above each launcher's grid cap"""
    x, h = acts(rows, K * Pw, K + Pw), hk(K)
    drive(ops, lambda x, h: ops.hadamard(x, K, h, fwht_route=True), dict(x=x, h=h))
    if K == 1 and 64 <= Pw <= 8192:
        drive(ops, lambda x: ops.hadamard_fp32(x), dict(x=x))
    if Pw in (512, 1024) or (K == 1 and 512 <= Pw <= 8192):
        drive(ops, lambda x, h: ops.hadamard_quant(x, K, h, (0.9, 0.9), route="fwht"), dict(x=x, h=h))
        drive(ops, lambda x, up, h: ops.hadamard_quant(x, K, h, (0.9, 0.9), up=up, route="fwht"), dict(x=x, up=acts(rows, K * Pw, 9), h=h))


@pytest.mark.parametrize("K,Pw", [(1, 64), (1, 4096), (1, 8192), (12, 512), (20, 256), (1, 32), (1, 16384)])
@pytest.mark.parametrize("rows", [1, 3, 37])
def test_hadamard_fp32_out(ops, K, Pw, rows):
    drive(ops, lambda x, h: ops.hadamard_fp32(x, K, h), dict(x=acts(rows, K * Pw, K + Pw + rows), h=hk(K)))


@pytest.mark.parametrize("K,Pw,dtype", [(1, 4096, BF), (12, 512, BF), (1, 128, torch.float32)])
def test_hadamard_wide(ops, K, Pw, dtype):
    h = None if K == 1 else hk(K).float()
    drive(ops, lambda x, h: ops.hadamard_wide(x, K, h), dict(x=acts(37, K * Pw, 5, dtype), h=h))


@pytest.mark.parametrize("K,Pw,route", [(1, 512, "fwht"), (1, 1024, "fwht"), (1, 2048, "fwht"), (1, 4096, "fwht"), (1, 8192, "fwht"), (1, 256, "fwht"),
                                        (12, 512, "fwht"), (60, 512, "fwht"), (28, 1024, "fwht"), (108, 128, "fwht"), (172, 64, "fwht"),
                                        (28, 512, "kron"), (28, 1024, "kron"), (172, 64, "kron"), (20, 256, None),
                                        (28, 512, "mfma"), (28, 1024, "mfma"), (12, 512, "mfma"), (32, 512, "mfma"), (4, 1024, "mfma")])
@pytest.mark.parametrize("rows", [1, 3, 37])
@pytest.mark.parametrize("with_up", [False, True])
def test_hadamard_quant(ops, K, Pw, route, rows, with_up):
    n = K * Pw
    x = acts(rows, n, K + Pw + rows)
    up = acts(rows, n, 3) if with_up else None
    drive(ops, lambda x, up, h: ops.hadamard_quant(x, K, h, (0.9, 0.9), up=up, route=route), dict(x=x, up=up, h=hk(K)))


@pytest.mark.parametrize("K,Pw", [(28, 512), (28, 1024), (12, 512), (32, 512), (4, 512), (8, 1024)])
@pytest.mark.parametrize("rows", [1, 3, 37, BIG])                         # (1031: above 2 / 3 token groups x n_cu)
def test_hadamard_mfma_variants(ops, K, Pw, rows):
    n = K * Pw
    x, up, h = acts(rows, n, K + rows), acts(rows, n, 4), hk(K)
    drive(ops, lambda x, h: ops.hadamard_mfma(x, K, h, None, None, True), dict(x=x, h=h))                         # the rotation
    drive(ops, lambda x, h: ops.hadamard_mfma(x, K, h, (0.9, 0.9), None, True), dict(x=x, h=h))                   # + Quantizer, with y
    drive(ops, lambda x, h: ops.hadamard_quantizer_mfma(x, K, h, 0.9, want_y=True), dict(x=x, h=h))
    drive(ops, lambda x, up, h: ops.hadamard_quantizer_mfma(x, K, h, 0.9, up=up), dict(x=x, up=up, h=h))          # + SiLU.mul input


@pytest.mark.parametrize("K,Pw", [(172, 64), (140, 64), (28, 512)])
@pytest.mark.parametrize("rows", [1, 3, 37])
def test_hadamard_quantizer(ops, K, Pw, rows):
    x, up = acts(rows, K * Pw, K + rows), acts(rows, K * Pw, 6)
    drive(ops, lambda x, up, h: ops.hadamard_quantizer(x, K, h, 0.9, up=up), dict(x=x, up=up, h=hk(K)))
    drive(ops, lambda x, h: ops.hadamard_quantizer(x, K, h, 1.0), dict(x=x, h=hk(K)))


# ------------------------------------------------------------------------------------------------ INT4 GEMMs

def int_product(xq, wq):
    """the exact integer product on the host: |sum| <= 64 K < 2^53"""
    x = torch.from_numpy(O.unpack_i4(xq.cpu().numpy())).double()
    w = torch.from_numpy(O.unpack_i4(wq.cpu().numpy())).double()
    return (x @ w.T).to(torch.int32)


def gemm_operands(M, N, K, seed=0):
    xq, wq = packed((M, K // 2), seed + M + N), packed((N, K // 2), seed + K + N + 1)
    xs = (rnd((M,), seed + 2).abs() * 0.02 + 0.001).half()
    wsc = (rnd((N,), seed + 3).abs() * 0.02 + 0.001).half()
    return xq, wq, xs, wsc, rnd((N,), seed + 4)


def linear_ref(c, xs, wsc, bias):
    """O.linear4bit on an integer product already at hand: sym_dequant (+ bias, an fp16 add)"""
    y = O.sym_dequant(c.numpy(), xs.cpu().numpy(), wsc.cpu().numpy())
    if bias is not None:
        with np.errstate(over="ignore"):
            y = (y.astype(np.float32) + bias.cpu().numpy().reshape(1, -1).astype(np.float32)).astype(np.float16)
    return y


@pytest.mark.parametrize("M,N,K", [(1, 16, 128), (7, 40, 96), (65, 24, 160), (257, 272, 256), (300, 4096, 512),
                                   (127, 128, 128), (129, 130, 128), (255, 256, 64), (BIG, 48, 128)])
def test_int4_matmul_and_linear(ops, M, N, K):
    xq, wq, xs, wsc, bias = gemm_operands(M, N, K)
    want, _, _ = drive(ops, lambda xq, wq: ops.int4_matmul(xq, wq), dict(xq=xq, wq=wq))
    c = int_product(xq, wq)
    assert torch.equal(want[0].cpu(), c)
    for b in (None, bias):
        want, _, _ = drive(ops, lambda **k: ops.int4_linear(k["xq"], k["xs"], k["wq"], k["wsc"], k["b"]), dict(xq=xq, xs=xs, wq=wq, wsc=wsc, b=b))
        assert same_bits(want[0].cpu().numpy(), linear_ref(c, xs, wsc, b))


@pytest.mark.parametrize("M", [1, 5, 17, 32, 33, 64, 65, 128])
@pytest.mark.parametrize("N", [16, 40, 48, 272, 2304])
def test_int4_skinny(ops, M, N):
    K = 256
    xq, wq, xs, wsc, bias = gemm_operands(M, N, K, 7)
    imgs, _, _ = drive(ops, lambda wq: ops.int4_to_frag(wq), dict(wq=wq))            # the image: containment + the same bytes under both poisons
    img = imgs[0]
    c = int_product(xq, wq)
    want, _, _ = drive(ops, lambda xq, img: ops.int4_skinny_matmul(xq, img, N), dict(xq=xq, img=img))
    assert torch.equal(want[0].cpu(), c)
    ref = ops.int4_linear(xq, xs, wq, wsc, bias)
    for split in (True, False):
        want, _, _ = drive(ops, lambda **k: ops.int4_skinny_linear(k["xq"], k["xs"], k["img"], k["wsc"], k["b"], N, split=split),
                           dict(xq=xq, xs=xs, img=img, wsc=wsc, b=bias))
        assert guards.same_raw(want[0], ref)
    # three problems of one launch: different N, with and without bias
    N2 = 96
    wq2 = packed((N2, K // 2), 11)
    img2, wsc2 = ops.int4_to_frag(wq2), (rnd((N2,), 12).abs() * 0.02 + 0.001).half()
    xq2, xs2 = packed((M, K // 2), 13), (rnd((M,), 14).abs() * 0.02 + 0.001).half()

    def multi(xq, xs, img, wsc, b, xq2, xs2, img2, wsc2):
        return ops.int4_skinny_linear_multi([(xq, xs, img, wsc, b), (xq2, xs2, img2, wsc2, None), (xq, xs, img, wsc, None)])

    want, _, _ = drive(ops, multi, dict(xq=xq, xs=xs, img=img, wsc=wsc, b=bias, xq2=xq2, xs2=xs2, img2=img2, wsc2=wsc2))
    assert guards.same_raw(want[0], ref) and guards.same_raw(want[1], ops.int4_linear(xq2, xs2, wq2, wsc2, None))


@pytest.mark.parametrize("M,N,K", [(33, 4096, 4096), (9, 2048, 8192), (1, 4096, 28672), (128, 1024, 8192), (64, 96, 4096)])
def test_int4_skinny_k_split(ops, M, N, K):
    """the K-split launch: its zeroed workspace is allocated under the guard; the arrival counters ([tiles] int32 in front, csrc/fq_gemm_i4.hip)
    read zero after each of three launches; bit-identical to the unsplit launch"""
    xq, wq, xs, wsc, bias = gemm_operands(M, N, K, 17)
    img = ops.int4_to_frag(wq)
    nbytes = int(ops.lib.fq_int4_skinny_split_workspace_bytes(M, N, K))
    assert nbytes > 0, "this geometry is meant to be split"
    tiles = (N + 31) // 32
    unsplit = ops.int4_skinny_linear(xq, xs, img, wsc, bias, N, split=False)
    state = {}

    def call(xq, xs, img, wsc, b):
        ys = []
        for _ in range(3):
            ys.append(ops.int4_skinny_linear(xq, xs, img, wsc, b, N))
            g = ops.torch._guard if hasattr(ops.torch, "_guard") else None
            if g is not None:
                (rec,) = g.find("zeros", nbytes)
                counters = rec.buf[rec.front:rec.front + tiles * 4].view(torch.int32)
                assert not bool(counters.any()), "arrival counters not back at zero"
                state[g.poison] = True
        return ys

    want, _, _ = drive(ops, call, dict(xq=xq, xs=xs, img=img, wsc=wsc, b=bias))
    assert state == {0x5A: True, 0xA5: True}
    assert all(guards.same_raw(y, unsplit) for y in want)


FP6_SHAPES = [(31, 32, 128), (129, 16, 128), (257, 528, 640), (513, 272, 256), (33, 256, 256), (97, 256, 256), (128, 256, 256), (1, 16, 128),
              (255, 256, 128), (3585, 3344, 256)]      # the last: 15 x 14 = 210 tiles of 256 x 256 (persistent), edge tiles in both dimensions


@pytest.mark.parametrize("M,N,K", FP6_SHAPES)
def test_fp6_path(ops, M, N, K):
    xq, wq, xs, wsc, bias = gemm_operands(M, N, K, 23)
    assert int(ops.lib.fq_bf6_blob_bytes(M, K)) > 0
    xb, _, _ = drive(ops, lambda xq: ops.int4_to_bf6(xq), dict(xq=xq))               # both roles: containment of the blob (its interior padding is
    wb, _, _ = drive(ops, lambda wq: ops.int4_to_bf6(wq, weights=True), dict(wq=wq))  # never written: it must still not reach an output, below)
    c = int_product(xq, wq)
    ref = ops.int4_linear(xq, xs, wq, wsc, bias)
    assert torch.equal(ops.int4_matmul(xq, wq).cpu(), c)
    # blobs converted INSIDE each guarded run: their interior padding holds the run's poison
    def mm(xq, wq):
        return ops.bf6_matmul(ops.int4_to_bf6(xq), ops.int4_to_bf6(wq, weights=True), M, N, K)

    def lin(xq, xs, wq, wsc, b):
        return ops.bf6_linear(ops.int4_to_bf6(xq), xs, ops.int4_to_bf6(wq, weights=True), wsc, b, M, N, K)

    want, _, _ = drive(ops, mm, dict(xq=xq, wq=wq))
    assert torch.equal(want[0].cpu(), c)
    want, _, _ = drive(ops, lin, dict(xq=xq, xs=xs, wq=wq, wsc=wsc, b=bias))
    assert guards.same_raw(want[0], ref)
    for kept in (False, True):                                                        # transient and kept image

        def one(xq, xs, wq, wsc, b):
            return ops.int4_linear_fp6(xq, xs, wq, ops.int4_to_bf6(wq, weights=True) if kept else None, wsc, b)

        want, _, _ = drive(ops, one, dict(xq=xq, xs=xs, wq=wq, wsc=wsc, b=bias))
        assert guards.same_raw(want[0], ref)
    if M <= 513:
        N2 = 48
        wq2, wsc2 = packed((N2, K // 2), 29), (rnd((N2,), 30).abs() * 0.02 + 0.001).half()

        def multi(xq, xs, wq, wsc, b, wq2, wsc2):
            return ops.int4_linear_fp6_multi([(xq, xs, wq, None, wsc, b), (xq, xs, wq2, ops.int4_to_bf6(wq2, weights=True), wsc2, None)])

        want, _, _ = drive(ops, multi, dict(xq=xq, xs=xs, wq=wq, wsc=wsc, b=bias, wq2=wq2, wsc2=wsc2))
        assert guards.same_raw(want[0], ref) and guards.same_raw(want[1], ops.int4_linear(xq, xs, wq2, wsc2, None))


@pytest.mark.parametrize("weights", [False, True])
def test_int4_to_bf6_beyond_the_grid_cap(ops, weights):
    """129 row tiles x 128 K-pairs x 64 lanes: above 16 n_cu x 256 threads, the conversion's grid-stride pass (the same count for int4_to_frag
    is the 4096 x 16384 and 4096 x 28672 images of the K-split and Linear4bit cases)"""
    drive(ops, lambda q: ops.int4_to_bf6(q, weights=weights), dict(q=packed((4097, 8192), 3)))


def test_fp6_refuses_what_it_cannot_run(ops):
    xq, wq, xs, wsc, bias = gemm_operands(5, 24, 128, 31)                             # N % 16 != 0
    drive(ops, lambda **k: ops.int4_linear_fp6(k["xq"], k["xs"], k["wq"], None, k["wsc"], k["b"]), dict(xq=xq, xs=xs, wq=wq, wsc=wsc, b=bias),
          refuse=True)
    drive(ops, lambda wq: ops.int4_to_frag(wq), dict(wq=packed((16, 48), 1)), refuse=True)         # K = 96: not a multiple of 64


# ------------------------------------------------------------------------------------------------ KV path

@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("rows", [1, 3, 65, BIG, 32771])                  # (32771 tokens of 2 heads: above 2 n_cu x 128 rows and 8 n_cu x 256 chunks)
@pytest.mark.parametrize("trans,lac,ret", [(False, False, False), (True, False, False), (True, True, False), (True, False, True), (False, True, False)])
def test_kv_quant_and_dequant(ops, hd, rows, trans, lac, ret):
    x = rnd((rows, 2, hd), hd + rows)
    tm = rnd((hd, hd), 3, F16, hd ** -0.5) if trans else None
    want, _, _ = drive(ops, lambda x, tm: ops.kv_quant(x, tm, (0.9, 0.8), lac, ret), dict(x=x, tm=tm))
    q, param = want[0], want[1]
    dq, _, _ = drive(ops, lambda q, param: ops.kv_dequant(q, param, lac), dict(q=q, param=param))
    if not trans and rows <= BIG:                                                       # the KV quantiser's bar: the oracle, bit for bit
        pk, sc, zr, _ = O.kv_asym_quant(x.cpu().numpy(), 0.9, 0.8, lac)
        assert np.array_equal(q.cpu().numpy(), pk)
        assert same_bits(dq[0].cpu().numpy(), O.kv_asym_dequant(pk, sc, zr, lac))


def paged(lens, heads, page, f16, hd=128, layers=2, spare=3, seed=0):
    """a paged cache whose request b holds lens[b] rows: pages scattered, `spare` pages no request references; the unused tail of every last page
    and every unreferenced page hold 0xFF data (NaN on fp16 pages) and NaN parameters"""
    g = torch.Generator().manual_seed(seed + sum(lens) + page)
    n_pg = [(n + page - 1) // page for n in lens]
    tot = sum(n_pg) + spare
    if f16:
        data = (torch.randn(tot, layers, 2, heads, page, hd, generator=g) * 1.5).half()
    else:
        data = torch.randint(0, 256, (tot, layers, 2, heads, page, hd // 2), generator=g, dtype=torch.uint8)
    param = torch.stack([torch.rand(tot, layers, 2, heads, page, generator=g) * 0.3 + 0.02,
                         torch.rand(tot, layers, 2, heads, page, generator=g) * 2.0 + 0.1], dim=-1).half()
    perm = torch.randperm(tot, generator=g)
    indices = perm[:sum(n_pg)].to(torch.int32)
    indptr = torch.tensor([0] + list(np.cumsum(n_pg)), dtype=torch.int32)
    last = torch.tensor([(n - 1) % page + 1 for n in lens], dtype=torch.int32)
    used = torch.zeros(tot, page, dtype=torch.bool)
    for b, n in enumerate(lens):
        for i, pg in enumerate(indices[int(indptr[b]):int(indptr[b + 1])].tolist()):
            used[pg, :min(page, n - i * page)] = True
    dead = ~used[:, None, None, None, :].expand(tot, layers, 2, heads, page)
    data[dead] = float("nan") if f16 else 0xFF
    param[dead] = float("nan")
    return data.cuda(), param.cuda(), indptr.cuda(), indices.cuda(), last.cuda(), used


def addressed(used_shape, layers, heads, indptr, indices, last, page, layer, counts):
    """-> bool [pages, layers, 2, heads, page]: the rows an append of counts[b] tokens per request writes (they END at the request's length)"""
    m = torch.zeros(used_shape[0], layers, 2, heads, page, dtype=torch.bool)
    ip, ix, la = indptr.tolist(), indices.cpu().long(), last.tolist()
    for b, n_app in enumerate(counts):
        L = (ip[b + 1] - ip[b] - 1) * page + la[b]
        pos = torch.arange(L - n_app, L)
        m[ix[ip[b] + pos // page], layer, :, :, pos % page] = True
    return m.cuda()


def check_append(ops, launch, shape_d, dt_d, shape_p, rows_mask, inputs, pads):
    """the cache filled with poison, guarded; after the launch every byte outside the addressed rows is still the poison, the addressed rows
    equal the plain run's"""
    base = {}
    for poison in guards.POISONS:
        d0 = torch.full(shape_d, poison, dtype=torch.uint8, device="cuda") if dt_d == torch.uint8 else \
            torch.full(shape_d[:-1] + (shape_d[-1] * 2,), poison, dtype=torch.uint8, device="cuda").view(F16)
        p0 = torch.full(shape_p[:-1] + (shape_p[-1] * 2,), poison, dtype=torch.uint8, device="cuda").view(F16)
        launch(d0, p0, **inputs)
        base[poison] = (d0, p0)
    torch.cuda.synchronize()
    for poison in guards.POISONS:
        ops.invalidate_caches()
        g = guards.Guard(poison)
        with g.on(ops):
            d = g.alloc(tuple(shape_d), dt_d, "cuda", "empty")
            p = g.alloc(tuple(shape_p), F16, "cuda", "empty")
            launch(d, p, **{k: _map(v, lambda t, k=k: g.guard_input(t, pads.get(k, "auto"))) for k, v in inputs.items()})
            torch.cuda.synchronize()
        g.check()
        for t, want in zip((d, p), base[poison]):
            raw_t = t.reshape(*rows_mask.shape, -1).view(torch.uint8)
            assert bool((raw_t[~rows_mask] == poison).all()), "a byte outside the addressed rows was written"
            assert torch.equal(raw_t[rows_mask], want.reshape(*rows_mask.shape, -1).view(torch.uint8)[rows_mask]), "addressed rows differ from the plain run"
            assert bool(rows_mask.any()) and not bool((raw_t[rows_mask] == poison).all())
    other = guards.POISONS[1]
    d_a, d_b = base[guards.POISONS[0]][0], base[other][0]
    m = rows_mask
    assert torch.equal(d_a.reshape(*m.shape, -1).view(torch.uint8)[m], d_b.reshape(*m.shape, -1).view(torch.uint8)[m])


APPEND_GEOM = [  # lens AFTER the append, tokens appended per request, page size, head_dim
    ([1, 16, 17, 33], [1, 1, 1, 1], 16, 128),           # last_page_offset in {1, page_size}
    ([5, 32, 40], [5, 3, 40], 16, 128),                 # multi-token steps through seqlen_indptr; a whole cache appended at once
    ([24, 25, 1, 48], [1, 1, 1, 1], 24, 64),
    ([7, 24, 50], [2, 24, 9], 24, 128),
    ([8, 9, 3], [1, 2, 3], 8, 64),
    ([65600, 7], [65600, 7], 16, 128),                  # 65607 tokens x 4 heads x 4 chunks: above 16 n_cu x 256 threads, the grid-stride pass
]


@pytest.mark.parametrize("lens,counts,page,hd", APPEND_GEOM)
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("group", [1, 4])
def test_kv_append_touches_its_rows_and_nothing_else(ops, lens, counts, page, hd, f16, group):
    heads, layers, layer = 4, 2, 1
    if f16 and lens[0] == 65600:
        lens, counts = [16500, 7], [16500, 7]               # (fp16 rows are 16 chunks: the same grid cap at a quarter of the tokens)
    _, _, indptr, indices, last, used = paged(lens, heads, page, f16, hd, layers)
    src = heads // group
    tokens = sum(counts)
    if f16:
        k, v = rnd((tokens, src, hd), 1), rnd((tokens, src, hd), 2)
    else:
        k, v = packed((tokens, src, hd // 2), 1), packed((tokens, src, hd // 2), 2)
    kp, vp = rnd((tokens, src, 2), 3), rnd((tokens, src, 2), 4)
    multi = any(c != 1 for c in counts)
    sl = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32, device="cuda") if multi else None
    mask = addressed(used.shape, layers, heads, indptr, indices, last, page, layer, counts)
    shape_d = (used.shape[0], layers, 2, heads, page, hd if f16 else hd // 2)

    def launch(d, p, indptr, indices, last, k, v, kp, vp, sl):
        ops.kv_append(d, p, indptr, indices, last, k, v, kp, vp, layer, sl, group)

    check_append(ops, launch, shape_d, F16 if f16 else torch.uint8, shape_d[:-1] + (2,), mask,
                 dict(indptr=indptr, indices=indices, last=last, k=k, v=v, kp=kp, vp=vp, sl=sl),
                 {"indptr": "repeat", "indices": "repeat", "last": "repeat", "sl": "repeat"})


@pytest.mark.parametrize("lens,added,page,hd", [([1, 16, 17, 33], 1, 16, 128), ([5, 32, 40, 8], 4, 16, 128), ([24, 25, 2, 48], 2, 24, 64), ([8, 9, 3], 3, 8, 128)])
@pytest.mark.parametrize("trans,lac", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("group", [1, 4])
def test_kv_quant_append_touches_its_rows_and_nothing_else(ops, lens, added, page, hd, trans, lac, group):
    heads, layers, layer = 4, 2, 0
    _, _, indptr, indices, last, used = paged(lens, heads, page, False, hd, layers)
    src = heads // group
    k, v = rnd((len(lens), added, src, hd), 1), rnd((len(lens), added, src, hd), 2)
    tm = rnd((hd, hd), 3, F16, hd ** -0.5) if trans else None
    mask = addressed(used.shape, layers, heads, indptr, indices, last, page, layer, [added] * len(lens))
    shape_d = (used.shape[0], layers, 2, heads, page, hd // 2)

    def launch(d, p, k, v, tm, indptr, indices, last):
        ops.kv_quant_append(k, v, tm, d, p, indptr, indices, last, layer, group, (0.9, 0.8, 0.95, 0.85) if lac else None, lac)

    check_append(ops, launch, shape_d, torch.uint8, shape_d[:-1] + (2,), mask, dict(k=k, v=v, tm=tm, indptr=indptr, indices=indices, last=last),
                 {"indptr": "repeat", "indices": "repeat", "last": "repeat"})


IDX_PADS = {"indptr": "repeat", "indices": "repeat", "last": "repeat"}
DECODE_CASES = [  # lens, cache heads, q_group, copies, page, fp16 pages, split, head_dim
    ([1, 300, 37], 4, 1, 1, 16, False, False, 128),            # plain; a one-row request
    ([1, 300, 37], 4, 1, 1, 16, True, False, 128),
    ([1, 2048, 700], 4, 1, 1, 16, False, True, 128),           # split (12 pairs)
    ([1, 900], 2, 1, 1, 24, True, True, 128),                  # split, fp16 pages of 24
    ([2048, 1, 700], 2, 4, 1, 16, False, True, 128),           # gqa, split
    ([100, 1, 33], 2, 4, 1, 16, True, False, 128),             # gqa, unsplit, fp16
    ([900, 1, 64], 8, 1, 4, 16, False, True, 128),             # copies
    ([900, 1, 64], 8, 1, 4, 32, True, False, 128),
    ([20 + i for i in range(70)], 8, 1, 1, 16, False, True, 128),   # 560 pairs: never split
    ([1, 300, 37], 4, 1, 1, 16, False, False, 64),             # head_dim 64
    ([5, 90], 2, 2, 1, 8, False, True, 128),                   # pages of 8
    # from 32 (request, KV head) pairs on, q_group 2 / 4 / 8 at head_dim 128 take the MERGED kernel: one workgroup per pair (two for a group of 8)
    # serves its query heads from one pass over the rows, p . v on the matrix pipe (fq_kv_decode_kernel<.., QG = 2 / 4>, fq_kvcache.hip)
    ([600, 1, 300, 520], 8, 4, 1, 16, False, True, 128),       # gqa 4, INT4, split (32 workgroups x 2 splits)
    ([600, 1, 300, 520], 8, 4, 1, 16, False, False, 128),      # ... unsplit
    ([600, 1, 300, 520], 8, 4, 1, 16, True, True, 128),        # gqa 4, fp16 pages, split
    ([90, 1, 33, 520], 8, 2, 1, 16, True, False, 128),         # gqa 2, fp16, unsplit
    ([600, 1, 300, 520], 8, 2, 1, 16, False, True, 128),       # gqa 2, INT4, split
    ([600, 1, 300, 520, 17, 16, 15, 700], 4, 8, 1, 16, False, True, 128),    # gqa 8: two workgroups of four query heads per pair, split
    ([40, 1, 300, 52, 17, 16, 15, 70], 4, 8, 1, 24, True, False, 128),       # gqa 8, fp16 pages of 24 (rows straddle pages), unsplit
    ([600, 1, 300, 520], 32, 1, 4, 16, False, True, 128),      # replicated cache read one copy per group of 4: 32 merged pairs, split
    ([600, 1, 300, 520], 32, 1, 4, 16, True, False, 128),      # ... fp16 pages, unsplit
    ([30 + i for i in range(70)], 8, 4, 1, 16, False, True, 128),  # 560 merged workgroups: four waves each, never split
    ([30 + i for i in range(20)], 8, 4, 1, 8, False, True, 128),   # 160 merged workgroups, pages of 8 (not uniform)
]


@pytest.mark.parametrize("lens,heads,q_group,copies,page,f16,split,hd", DECODE_CASES)
@pytest.mark.parametrize("qt,transpose_out", [(False, False), (True, True)])
def test_kv_batch_decode_every_route(ops, lens, heads, q_group, copies, page, f16, split, hd, qt, transpose_out):
    data, param, indptr, indices, last, _ = paged(lens, heads, page, f16, hd)
    H = heads * q_group
    q = rnd((len(lens), H, hd), 1, F16, 0.5)
    tm = rnd((hd, hd), 2, F16, hd ** -0.5) if qt else None

    def call(q, data, param, indptr, indices, last, tm):
        o = ops.kv_batch_decode(q, data, param, indptr, indices, last, 1, tm, transpose_out, seq_hint=max(lens), split=split, kv_copies=copies)
        return [o, ops.kv_batch_decode(q, data, param, indptr, indices, last, 1, tm, transpose_out, seq_hint=0, split=split, kv_copies=copies)]

    want, _, _ = drive(ops, call, dict(q=q, data=data, param=param, indptr=indptr, indices=indices, last=last, tm=tm), pads=IDX_PADS)
    assert all(bool(torch.isfinite(o.float()).all()) for o in want)          # NaN parameters / 0xFF data of dead rows and pages never reach o


EXTEND_CASES = [  # lens, cache heads, q_group, copies, page, T, fp16 pages, split
    ([3, 16, 18], 2, 4, 1, 16, 3, False, True),
    ([2048, 4], 8, 4, 4, 16, 4, False, True),
    ([1500, 17], 8, 4, 1, 16, 16, True, True),
    ([5, 40, 23], 2, 4, 1, 8, 5, False, False),
    ([17, 64, 49], 8, 4, 4, 24, 17, False, True),
    ([100, 81, 1], 1, 8, 1, 24, 1, True, False),
    ([60 + i for i in range(64)], 2, 4, 1, 8, 8, True, True),
    ([50 + i for i in range(65)], 8, 4, 1, 16, 4, False, True),
]


@pytest.mark.parametrize("lens,heads,q_group,copies,page,Tn,f16,split", EXTEND_CASES)
@pytest.mark.parametrize("qt,transpose_out", [(False, False), (True, True)])
def test_kv_batch_extend_every_route(ops, lens, heads, q_group, copies, page, Tn, f16, split, qt, transpose_out):
    data, param, indptr, indices, last, _ = paged(lens, heads, page, f16)
    H = heads // copies * q_group
    q = rnd((len(lens), Tn, H, 128), 1, F16, 0.5)
    tm = rnd((128, 128), 2, F16, 128 ** -0.5) if qt else None
    want, _, _ = drive(ops, lambda **k: ops.kv_batch_extend(k["q"], k["data"], k["param"], k["indptr"], k["indices"], k["last"], 0, k["tm"], transpose_out,
                                                           seq_hint=max(lens), split=split, kv_copies=copies),
                       dict(q=q, data=data, param=param, indptr=indptr, indices=indices, last=last, tm=tm), pads=IDX_PADS)
    assert bool(torch.isfinite(want[0].float()).all())


@pytest.mark.parametrize("lens,cache_heads,src_heads,q_group,page,one_copy,split", [
    ([1, 300, 37], 4, 4, 1, 16, False, True), ([1, 2048, 16, 17], 8, 2, 1, 16, True, True), ([1, 2048, 16, 17], 8, 2, 1, 16, False, False),
    ([700, 1, 33], 2, 2, 4, 32, False, True), ([20 + i for i in range(40)], 8, 8, 1, 16, False, True),
    # 32 (request, KV head) pairs and more: the merged kernel with the append (fq_kv_decode_kernel<.., QG = 4 / 2, APPEND = true>)
    ([600, 1, 300, 520], 8, 8, 4, 16, False, True), ([600, 1, 300, 520], 8, 8, 4, 16, False, False), ([90, 1, 33, 520], 8, 8, 2, 32, False, True),
    ([600, 1, 300, 520], 32, 8, 1, 16, True, True), ([600, 1, 300, 520, 17, 16, 15, 700], 4, 4, 8, 16, False, True)])
@pytest.mark.parametrize("trans,qt,transpose_out", [(False, False, False), (True, True, True)])
def test_kv_decode_append_writes_one_row(ops, lens, cache_heads, src_heads, q_group, page, one_copy, split, trans, qt, transpose_out):
    """the append inside the attention launch: o and the cache equal the plain run's; the cache changes in the new token's rows and nowhere else
    (the new row's slot holds 0xFF / NaN before the launch like every other dead row)"""
    hd, layers, layer = 128, 2, 1
    data, param, indptr, indices, last, used = paged(lens, cache_heads, page, False, hd, layers)
    mask = addressed(used.shape, layers, cache_heads, indptr, indices, last, page, layer, [1] * len(lens))
    data[mask], param[mask] = 0xFF, float("nan")
    H = cache_heads * q_group
    q = rnd((len(lens), H, hd), 1, F16, 0.5)
    kn, vn = rnd((len(lens), src_heads, hd), 2), rnd((len(lens), src_heads, hd), 3)
    tk = rnd((hd, hd), 4, F16, hd ** -0.5) if trans else None
    tq = rnd((hd, hd), 5, F16, hd ** -0.5) if qt else None
    assert ops.kv_decode_append_supported(data, src_heads)
    before = {}

    def call(q, kn, vn, tk, data, param, indptr, indices, last, tq):
        before[data.data_ptr()] = (data, data.clone(), param, param.clone())
        return ops.kv_decode_append(q, kn, vn, tk, data, param, indptr, indices, last, layer, tq, transpose_out, seq_hint=max(lens), split=split,
                                    read_one_copy=one_copy)

    want, _, _ = drive(ops, call, dict(q=q, kn=kn, vn=vn, tk=tk, data=data, param=param, indptr=indptr, indices=indices, last=last, tq=tq),
                       pads=IDX_PADS, inout=("data", "param"))
    assert bool(torch.isfinite(want[0].float()).all()) and len(before) == 3
    for d1, d0, p1, p0 in before.values():
        assert torch.equal(d1[~mask], d0[~mask]) and guards.same_raw(p1[~mask], p0[~mask])
        assert not bool((d1[mask] == 0xFF).all()) and bool(torch.isfinite(p1[mask].float()).all())
    # the two calls it replaces leave the same cache
    d2, p2 = data.clone(), param.clone()
    ops.kv_quant_append(kn[:, None].contiguous(), vn[:, None].contiguous(), tk, d2, p2, indptr, indices, last, layer, cache_heads // src_heads)
    assert torch.equal(d2, want[1]) and guards.same_raw(p2, want[2])


# ------------------------------------------------------------------------------------------------ module level

@pytest.mark.parametrize("disable_quant,fuse_append,trans", [(False, True, "matmul"), (False, False, "matmul"), (True, False, "had")])
def test_paged_cache_class_under_the_guard(ops, disable_quant, fuse_append, trans):
    """MultiLayerPagedKVCache4Bit: prefill, three decode steps and one T = 4 extend step; its own buffers (pages, scales, index tensors) keep
    their pads and every attention output equals an unguarded twin's bit for bit"""
    import flatquant_amd.deploy.transformers as TR
    from flatquant_amd.deploy.transformers import kv_cache as KC
    bsz, prompt, kv_heads, group, hd, layers = 4, 30, 8, 4, 128, 2          # (32 (request, KV head) pairs: the merged decode kernel)
    H = kv_heads * group
    gen = torch.Generator(device="cuda").manual_seed(5)
    tk = (torch.randn(hd, hd, generator=gen, device="cuda") / hd ** 0.5).half()
    kw = {"trans_matrix_k": tk, "trans_matrix_k_inv_t": torch.linalg.inv(tk.float()).T.contiguous().half()}
    steps = [prompt, 1, 1, 1, 4]
    ks = [[torch.randn(bsz, n, kv_heads, hd, generator=gen, device="cuda").half() for _ in range(layers)] for n in steps]
    vs = [[torch.randn(bsz, n, kv_heads, hd, generator=gen, device="cuda").half() for _ in range(layers)] for n in steps]
    qs = [[(torch.randn(bsz, n, H, hd, generator=gen, device="cuda") * 0.5).half() for _ in range(layers)] for n in steps]

    def run():
        c = TR.MultiLayerPagedKVCache4Bit(bsz, 16, 64, "cuda", layers, H, hd, trans=trans, group_size=group, fuse_append=fuse_append,
                                          disable_quant=disable_quant)
        outs = []
        for s, n in enumerate(steps):
            for l in range(layers):
                att = c.update(ks[s][l], vs[s][l], l, dict(kw))
                if s:
                    outs.append(att(qs[s][l]))
                    outs.append(att(qs[s][l], transposed=True))
        torch.cuda.synchronize()
        return c, outs

    _, want = run()
    for poison in guards.POISONS:
        ops.invalidate_caches()
        g = guards.Guard(poison)
        with g.on(ops, KC):
            c, got = run()
        g.check()
        assert len(g.records) > 2 and any(r.shape == tuple(c._pages.shape) for r in g.records)
        assert len(got) == len(want) and all(guards.same_raw(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("rows,N,K", [(5, 96, 256), (40, 1024, 2048), (200, 2048, 256), (200, 96, 256), (1, 4096, 16384)])
def test_linear4bit_under_the_guard(ops, rows, N, K):
    """deploy.nn.Linear4bit: the decode plan, the K-split workspace, the transient FP6 conversion and the int8 path, images and scratch allocated
    under the guard; outputs equal an unguarded twin's"""
    from flatquant_amd.deploy import PackedQuantizedTensor
    from flatquant_amd.deploy.nn import linear as LIN
    xq, wq, xs, wsc, bias = gemm_operands(rows, N, K, 41)

    def run():
        m = LIN.Linear4bit(K, N, bias=True).cuda()
        m.weight.copy_(wq), m.weight_scales.copy_(wsc.float().reshape(N, 1)), m.bias.copy_(bias)
        ys = [m(PackedQuantizedTensor(xq, xs)) for _ in range(2)]
        torch.cuda.synchronize()
        m.release_images()                    # (the class-wide FP6 image account goes back to where it was)
        return ys

    want = run()
    assert guards.same_raw(want[0], ops.int4_linear(xq, xs, wq, wsc, bias)) and guards.same_raw(want[1], want[0])
    for poison in guards.POISONS:
        ops.invalidate_caches()
        g = guards.Guard(poison)
        with g.on(ops, LIN):
            got = run()
        g.check()
        assert any(r.buf.is_cuda for r in g.records)
        assert all(guards.same_raw(a, want[0]) for a in got)
