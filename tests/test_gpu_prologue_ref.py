"""The launches whose prologue is NOT exact — RMSNorm, SiLU.mul, the Hadamard rotations — held to the derived references of tests/prologue_ref.py
(their own checks: tests/test_prologue_ref_cpu.py; derivations: DESIGN.md 7.6). Every assertion is bit equality or membership in a derived set;
NaN is compared as a class; nothing else is masked.
  (0) v_rsq_f32 / v_exp_f32 / v_rcp_f32 measured against float64: at most 2 ulp, and no more than the windows below assume;
  (A) SiLU.mul: every one of the 65536 gates lies in its admissible set, against ten `up` values; every launch that forms the product itself is
      bit-identical to the same launch on ops.silu_mul's output for EVERY gate with |g| <= 24; the edge batch under exact factors;
  (B) RMSNorm: every row is explained by ONE fp32 reciprocal root of the derived window — the standalone kernel at six widths and three eps,
      the fused 64 x 64 and wave launches through the oracle's transform and quantiser, each also tiled above its launcher's grid cap;
  (C) Hadamard: tokens whose rotation is exact in every order — every route returns the bits of the integer rotation, end to end.
The figures the issue asks for are printed (pytest -s shows them), and appended to the file FQ_PROLOGUE_REF_OUT names when it is set — a write
that fails fails the test (profiles/prologue_ref.txt is that file from one run)."""
import os

import numpy as np
import pytest
import torch

from oracle import fq_oracle as O
from tests import edge_tokens as E
from tests import prologue_ref as R
from tests.conftest import hadk_matrix, same_bits
from tests.test_gpu_bounds import BIG, WAVE_BIG

pytestmark = pytest.mark.gpu
P, F, T, R16, NC0, Q16 = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
F16, F32 = np.float16, np.float32
SWEEP_SIGS = [E.SIGS[1], E.SIGS[7]]


@pytest.fixture(scope="module")
def ops():
    from flatquant_amd import ops as _ops
    return _ops


def record(line):
    print(line)
    path = os.environ.get("FQ_PROLOGUE_REF_OUT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().contiguous().cpu().numpy()


def raw(o):
    ts = (list(o.q) + list(o.scale) + list(o.fq) + [o.y]) if hasattr(o, "fq") else list(o)
    return [t if t.dtype == torch.uint8 else t.view(torch.int16) for t in ts if t is not None]


def assert_same(a, b, what):
    ra, rb = raw(a), raw(b)
    assert ra and len(ra) == len(rb), what
    for u, v in zip(ra, rb):
        assert torch.equal(u.reshape(-1), v.reshape(-1)), what


# ---------------------------------------------------------------------------------------------------------------- (0) the hardware functions

@pytest.mark.parametrize("op,assumed", [("rsq", R.U_RSQ), ("exp2", R.U_EXP), ("rcp", R.U_RCP)])
def test_special_function_error_is_what_the_windows_assume(op, assumed):
    from flatquant_amd import _probe
    x = R.sfu_inputs(op)
    u = R.ulp_error(host(_probe.probe_sfu(op, dev(x))), R.sfu_exact(op, x))
    record(f"u_{op[:3]} = {u:.4f} ulp over {x.size} inputs in [{R.SFU_RANGES[op][0]:g}, {R.SFU_RANGES[op][1]:g}]")
    assert u <= R.U_CAP and u <= assumed, (op, u)


# ---------------------------------------------------------------------------------------------------------------- (A) SiLU.mul

def test_silu_mul_every_gate_is_admissible(ops):
    g = np.broadcast_to(R.all_gates(), (len(R.UPS), 65536))
    up = np.broadcast_to(R.UPS[:, None], g.shape)
    got = host(ops.silu_mul(dev(g), dev(up)))
    lo, hi = R.silu_admissible(g)
    ok = R.in_set(got, [R.mul16(lo, up), R.mul16(hi, up)])
    with np.errstate(invalid="ignore", over="ignore"):
        rounded = R.mul16(R.silu_exact(g).astype(F16), up)
    miss = int((~R.in_set(got, [rounded]) & np.isfinite(g.astype(F32))).sum())
    record(f"silu_mul: {miss} of {g.size} outputs differ from fp16(up * fp16(s(g))) with s correctly rounded; {int((~ok).sum())} outside their set")
    bad = np.argwhere(~ok)
    assert not len(bad), (len(bad), [(float(R.UPS[i]), hex(j), hex(int(got.view(np.uint16)[i, j]))) for i, j in bad[:8]])


@pytest.mark.parametrize("M,N", [(112, 128), (128, 224), (86, 128)])
def test_gate_sweep_through_the_silu_kron_launch(ops, M, N):
    gate, up = (dev(a) for a in R.sweep_tokens(M * N))
    Ld, Rd = (dev(m) for m in E.random_factors(M, N))
    x = ops.silu_mul(gate, up)
    for flags in (P, T | P | R16, P | NC0):
        assert_same(ops.silu_mul_kron_quant(gate, up, Ld, Rd, SWEEP_SIGS, flags), ops.kron_quant(x, Ld, Rd, SWEEP_SIGS, flags), (M, N, hex(flags)))


@pytest.mark.parametrize("n,K", [(512, 1), (6144, 12), (14336, 28), (11008, 172), (12288, 12)])
def test_gate_sweep_through_the_silu_hadamard_launches(ops, n, K):
    gate, up = (dev(a) for a in R.sweep_tokens(n))
    h = dev(hadk_matrix(K)) if K > 1 else None
    x = ops.silu_mul(gate, up)
    if n != 12288:
        for route in (None, "fwht", "kron"):
            assert_same(ops.hadamard_quant(gate, K, h, E.SIGS[2], up=up, route=route), ops.hadamard_quant(x, K, h, E.SIGS[2], route=route), (n, route))
    if n in (6144, 12288):
        assert_same(ops.hadamard_mfma(gate, K, h, E.SIGS[2], None, False, up=up)[1:], ops.hadamard_mfma(x, K, h, E.SIGS[2], None, False)[1:], n)
        for ratio in (1.0, 0.9):
            assert_same(ops.hadamard_quantizer_mfma(gate, K, h, ratio, up=up)[:2], ops.hadamard_quantizer_mfma(x, K, h, ratio)[:2], (n, ratio))


@pytest.mark.parametrize("M,N", [(112, 128), (128, 224), (86, 128)])
def test_silu_edge_batch_under_exact_factors(ops, M, N):
    b = E.batch(M, N)
    up = R.edge_up(b)
    L, Rm = E.exact_factors(M, N)
    flags = T | P | F | R16
    o = ops.silu_mul_kron_quant(dev(b), dev(up), dev(L), dev(Rm), E.SIGS[:3], flags)
    y = host(o.y).reshape(E.N_BATCH, -1)
    cands = [O.kron_transform(R.mul16(a, up), L, Rm).reshape(E.N_BATCH, -1).astype(F16) for a in R.silu_admissible(b)]
    assert R.in_set(y, cands).all()
    for ci, sig in enumerate(E.SIGS[:3]):
        ref = O.quant_outputs(y.astype(F32), sig[0], sig[1], round_y_f16=True)
        assert np.array_equal(host(o.q[ci]).reshape(E.N_BATCH, -1), ref["packed"]), sig
        assert same_bits(host(o.scale[ci]).reshape(-1), ref["scale16"].reshape(-1)), sig
        assert same_bits(host(o.fq[ci]).reshape(E.N_BATCH, -1), ref["fq"]), sig


# ---------------------------------------------------------------------------------------------------------------- (B) RMSNorm

def rms_big():
    """a row count above fq_launch_rmsnorm's grid cap (8 n_cu workgroups of four rows: 8192 rows at n_cu = 256) that is no multiple of 25"""
    rows = 32 * torch.cuda.get_device_properties(0).multi_processor_count + E.N_BATCH
    return rows + (rows % E.N_BATCH == 0)


@pytest.mark.parametrize("cols", [8, 40, 1000, 4096, 8192, 16384])
def test_rmsnorm_rows_have_one_reciprocal_root(ops, cols):
    x = R.rms_rows(cols)
    xd = dev(x)
    for eps in (1e-5, 1e-6, 0.0):
        y = host(ops.rmsnorm(xd, eps))
        worst = 0.0
        for i in range(x.shape[0]):
            r, cands, ok = R.rms_search(x[i], y[i], eps, cols)
            assert ok.any(), (cols, eps, i)
            worst = max(worst, R.rms_deviation(r, cands, ok))
        record(f"rmsnorm cols={cols} eps={eps:g}: accepted centre off by {worst:.2f} x 2^-24 at most (window +-{2 * R.rms_width(cols):.1f})")
    idx = torch.arange(rms_big(), device="cuda") % E.N_BATCH               # above the grid cap: rinv carried from an edge row to an ordinary one
    base = ops.rmsnorm(xd, 1e-5).view(torch.int16)
    assert torch.equal(ops.rmsnorm(xd[idx].contiguous(), 1e-5).view(torch.int16), base[idx])


def d_pad(M, N):
    return 4096 if (M, N) == (64, 64) else -(-M // 32) * 32 * N


RMS_FUSED = [(64, 64, fl) for fl in (T | R16, T | P | R16, P, P | NC0)] + \
            [(M, N, fl) for (M, N) in ((32, 64), (56, 64), (64, 80), (64, 112), (64, 128)) for fl in (P, P | NC0)]


@pytest.mark.parametrize("M,N,flags", RMS_FUSED)
def test_rmsnorm_fused_launch_has_one_reciprocal_root(ops, M, N, flags):
    b = E.batch(M, N)
    L, Rm = E.exact_factors(M, N)
    xd, Ld, Rd = dev(b), dev(L), dev(Rm)
    eps = 1e-5
    sig_sets = [E.SIGS[:3], [E.SIGS[7], E.SIGS[8]], E.SIGS[:1]]
    outs = [ops.rmsnorm_kron_quant(xd, eps, Ld, Rd, sigs, flags) for sigs in sig_sets]
    kw = dict(round_y_f16=bool(flags & R16), clamp0=not flags & NC0)
    worst = 0.0
    for i in range(E.N_BATCH):
        r, cands = R.rms_candidates(b[i], eps, d_pad(M, N))
        y = O.kron_transform(R.rms_apply(b[i], cands), L, Rm).reshape(len(cands), -1)
        ok = np.ones(len(cands), bool)
        for sigs, o in zip(sig_sets, outs):
            if flags & T:
                ok &= R.in_set(np.broadcast_to(host(o.y).reshape(E.N_BATCH, -1)[i], y.shape), [y.astype(F16)]).all(axis=1)
            if flags & P:
                for ci, sig in enumerate(sigs):
                    ref = O.quant_outputs(y, sig[0], sig[1], **kw)
                    ok &= (ref["packed"] == host(o.q[ci]).reshape(E.N_BATCH, -1)[i]).all(axis=1)
                    ok &= ref["scale16"].reshape(-1).view(np.uint16) == host(o.scale[ci]).reshape(-1).view(np.uint16)[i]
        assert ok.any(), (M, N, hex(flags), i)
        worst = max(worst, R.rms_deviation(r, cands, ok))
    record(f"rmsnorm_kron_quant {M}x{N} flags={flags:#x}: accepted centre off by {worst:.2f} x 2^-24 at most (window +-{2 * R.rms_width(d_pad(M, N)):.1f})")
    big = BIG if (M, N) == (64, 64) else WAVE_BIG
    idx = torch.arange(big, device="cuda") % E.N_BATCH
    for a, g in zip(raw(outs[0]), raw(ops.rmsnorm_kron_quant(xd[idx].contiguous(), eps, Ld, Rd, sig_sets[0], flags))):
        assert torch.equal(g.reshape(big, -1), a.reshape(E.N_BATCH, -1)[idx]), ("tiled to", big)


@pytest.mark.parametrize("tokens", [[11], [1, 11, 13, 0], list(range(16))])
def test_fused_decode_launch_on_edge_tokens(ops, tokens):
    gen = torch.Generator().manual_seed(len(tokens))

    def _mats(gen, n):
        return (torch.randn(n, n, generator=gen) / n ** 0.5 + torch.eye(n) * 0.5).half().cuda()

    def _problem(ops, gen, N, bias):
        wp = torch.from_numpy(O.pack_i4(torch.randint(-8, 8, (N, 4096), generator=gen, dtype=torch.int32).numpy())).cuda()
        ws = (torch.rand(N, generator=gen) * 0.01 + 0.001).half().cuda()
        return wp, ops.int4_to_frag(wp), ws, (torch.randn(N, generator=gen) * 0.1).half().cuda() if bias else None

    x = dev(E.batch(64, 64)[tokens])
    L, Rm = _mats(gen, 64), _mats(gen, 64)
    Ns, sigs = (4096, 1024, 96), [(1.0, 1.0), (0.71, 0.83), (0.5, 0.45)]
    probs = [_problem(ops, gen, N, p == 1) for p, N in enumerate(Ns)]
    for fl in (0, NC0):
        q = ops.rmsnorm_kron_quant(x, 1e-5, L, Rm, sigs, P | fl)
        ref = ops.int4_skinny_linear_multi([(q.q[p], q.scale[p], probs[p][1], probs[p][2], probs[p][3]) for p in range(len(Ns))])
        got = ops.kron64_linear_multi(x, L, Rm, sigs, [(pr[1], pr[2], pr[3]) for pr in probs], eps=1e-5, flags=fl)
        assert got is not None
        for p in range(len(Ns)):
            assert torch.equal(ref[p].view(torch.int16), got[p].view(torch.int16)), (len(tokens), p, fl)


# ---------------------------------------------------------------------------------------------------------------- (C) Hadamard

HAD_SHAPES = [(6144, 12), (14336, 28), (12288, 12), (28672, 28), (5120, 40), (8960, 140), (11008, 172), (1536, 12), (5120, 20),
              (64, 1), (512, 1), (8192, 1), (32768, 1)]
# the dense Kronecker pair each width must reach (N of _hadamard_as_kron), None where ops has none
DENSE_N = {(6144, 12): 64, (14336, 28): 128, (12288, 12): 128, (28672, 28): 256, (5120, 40): 64, (8960, 140): 64, (11008, 172): 64,
           (1536, 12): None, (5120, 20): 64, (64, 1): None, (512, 1): None, (8192, 1): None, (32768, 1): None}


def bits(t):
    return host(t).view(np.uint16)


def rotations(ops, x, K, h, scale, n):
    """-> {route: fp16 [rows, n]} from every route that exists for the width; refusals asserted"""
    from flatquant_amd import _lib
    out = {"default": ops.hadamard(x, K, h, scale), "fwht": ops.hadamard(x, K, h, scale, fwht_route=True)}
    if K > 1:
        if ops.had_mfma_supported(n, K):
            out["mfma"] = ops.hadamard_mfma(x, K, h, None, scale, True)[0]
        else:
            with pytest.raises(ValueError):
                ops.hadamard_mfma(x, K, h, None, scale, True)
            with pytest.raises(_lib.FqError):
                ops.hadamard_quant(x, K, h, E.SIGS[0], scale, route="mfma")
    kr = ops._hadamard_as_kron(K, n // K, h, x.device)
    assert (None if kr is None else kr[2]) == DENSE_N[(n, K)]
    if kr is not None:
        sc = float(1.0 / torch.tensor(n).sqrt()) if scale is None else scale
        out["kron"] = ops.kron_quant_ex(x, kr[0], kr[1], ops._had_right_div(kr[2]) * sc, [(1.0, 1.0)], T | R16).y
    return out


def check_end_to_end(ops, x, K, h, scale, n, y_ref):
    routes = [None, "fwht"] + (["kron"] if DENSE_N[(n, K)] else []) + (["mfma"] if K > 1 and ops.had_mfma_supported(n, K) else [])
    for sig in E.SIGS[:3]:
        ref = O.rowquant(y_ref, sig[0], sig[1], clamp0=True, quant_f16=True, sig_f16=True)
        for route in routes:
            q, s = ops.hadamard_quant(x, K, h, sig, scale, route=route)
            assert np.array_equal(host(q), ref["packed"]), (n, K, scale, route, sig, "digits")
            assert np.array_equal(bits(s).reshape(-1), ref["scale16"].reshape(-1).view(np.uint16)), (n, K, scale, route, sig, "scales")
    if K > 1:
        from flatquant_amd._lib import FQ_RATIO_POST
        kr = ops._hadamard_as_kron(K, n // K, h, x.device)
        sc = float(1.0 / torch.tensor(n).sqrt()) if scale is None else scale
        for ratio in (1.0, 0.9):
            qr, sr = O.quantizer_plain(y_ref, ratio)
            got = []
            if kr is not None and kr[2] == 64:
                # the tall pair with FQ_RATIO_POST, which ops.hadamard_quantizer reaches at the default scale only: here at every scale, so on the
                # integer tokens and their .5 ties too
                o = ops.kron_quant_ex(x, kr[0], kr[1], ops._had_right_div(64) * sc, [(ratio, 1.0)], P | Q16 | R16 | FQ_RATIO_POST)
                got.append(("tall pair, ratio after", (o.q[0], o.scale[0])))
            if ops.had_mfma_supported(n, K):
                got.append(("quantizer_mfma", ops.hadamard_quantizer_mfma(x, K, h, ratio, scale)[:2]))
            if scale is None and ops.hadamard_quantizer(x, K, h, ratio) is not None:
                got.append(("quantizer", ops.hadamard_quantizer(x, K, h, ratio)))
            for name, (q, s) in got:
                assert np.array_equal(host(q), qr), (n, K, scale, name, ratio, "digits")
                assert np.array_equal(bits(s).reshape(-1), sr.view(np.uint16)), (n, K, scale, name, ratio, "scales")


@pytest.mark.parametrize("n,K", HAD_SHAPES)
def test_every_hadamard_route_returns_the_exact_rotation(ops, n, K):
    x, single = R.had_tokens(n, K)
    hk = hadk_matrix(K) if K > 1 else None
    h = dev(hk) if K > 1 else None
    for scale in R.HAD_SCALES:
        keep = R.had_keep(x, single, scale)
        y_ref = R.had_exact(x[keep], K, hk, scale)
        xd = dev(x[keep])
        for route, y in rotations(ops, xd, K, h, scale, n).items():
            assert np.array_equal(bits(y), y_ref.view(np.uint16)), (n, K, scale, route, int((bits(y) != y_ref.view(np.uint16)).sum()))
        assert np.array_equal(host(ops.hadamard_fp32(xd, K, h, scale)), y_ref.astype(F32)), (n, K, scale, "fp32")
        check_end_to_end(ops, xd, K, h, scale, n, y_ref)
    # the default scale 1 / sqrt(n): single-nonzero tokens, each reading one column of signs of the whole rotation
    s32 = F32(1.0) / np.sqrt(F32(n))
    keep = R.had_keep(x, single, float(s32)) & single
    y_ref = R.had_single_default(x[keep], K, hk, s32)
    xd = dev(x[keep])
    for route, y in rotations(ops, xd, K, h, None, n).items():
        assert np.array_equal(bits(y), y_ref.view(np.uint16)), (n, K, "1/sqrt(n)", route, int((bits(y) != y_ref.view(np.uint16)).sum()))
    check_end_to_end(ops, xd, K, h, None, n, y_ref)
