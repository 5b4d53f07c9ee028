// fq_kron_route.hip — fq_kron_route: the ONE statement of which kernel a Kronecker transform + quantiser launch runs (the order of
// preference among the families and every shared precondition), as host arithmetic on the launch's descriptors. The C ABI's launches
// (fq_capi.hip) ask it and hand the answer to the family's launcher; tests and tools ask it through fq_debug_kron_route.
#include <cstdio>

#include "fq_launch.hpp"

namespace {

FqKronRoute none(int rc) {
    FqKronRoute r = {};
    r.rc = rc;
    r.family = -1;
    return r;
}
FqKronRoute pick(int family, int t0, int t1 = 0, int t2 = 0, int t3 = 0, int t4 = 0, int t5 = 0, int t6 = 0, int t7 = 0, int t8 = 0,
                 int t9 = 0, int t10 = 0) {
    return FqKronRoute{0, family, {t0, t1, t2, t3, t4, t5, t6, t7, t8, t9, t10}, 0};
}

struct Launch {
    int ct;          // the compile-time flags
    bool bf, rms, silu, g128, round16, diag, y, fq0, in2, post_scale, gstride;
    int n_clips, M, N, MT, NT, KS1, lks;
    int64_t rows;
    int masked;
    bool off(int f) const { return (masked >> f) & 1; }
};

// one wave per token where a token fits a wave: packed output; up to N = 80 also fake-quant only / the transform alone
FqKronRoute wave(const Launch& l) {
    const bool os_ok = l.N / 16 <= WAVE_OS_MAXKS, plain = !l.rms && !l.g128;
    const bool fq_only = os_ok && l.ct == FQ_OUT_FAKEQUANT && plain;      // (round 4) 16-bit outputs, fp32 quantiser
    const bool y_only = os_ok && (l.ct == FQ_OUT_TRANSFORM || l.ct == (FQ_OUT_TRANSFORM | FQ_QUANT_F16)) && plain && l.n_clips == 0;
    if ((l.ct != FQ_OUT_PACKED && !fq_only && !y_only) || l.diag) return none(FQ_LAUNCH_NO_KERNEL);
    if ((fq_only && !l.fq0) || (y_only && !l.y)) return none(FQ_LAUNCH_NO_KERNEL);
    if (l.M > 64 || ((l.M * (l.N / 8)) & 63)) return none(FQ_LAUNCH_NO_KERNEL);
    if (l.g128 && (l.N != 64 || (l.M & 1))) return none(FQ_LAUNCH_NO_KERNEL);  // groups = pairs of 64-element rows
    // bf16: 64 x 64 stays with fq_kron64.hip, group-128 launches with the workgroup kernel's group epilogue, and deploy.nn.RMSNorm is an fp16 module
    if (l.bf && ((l.M == 64 && l.N == 64) || l.g128 || l.rms)) return none(FQ_LAUNCH_NO_KERNEL);
    const int os = fq_only ? FQ_OUT_FAKEQUANT : y_only ? FQ_OUT_TRANSFORM : FQ_OUT_PACKED;
#define X(MT_, NT_, KS1_, W_) \
    if (l.MT == MT_ && l.KS1 == KS1_) return pick(FQ_KF_WAVE, MT_, NT_, KS1_, W_, l.rms, l.bf, os);
    FQ_KRON_WAVE_LIST(X)
#undef X
    return none(FQ_LAUNCH_NO_KERNEL);
}

// token groups of NT waves
FqKronRoute tiles(const Launch& l) {
    if (l.N == 64 && l.M > 64 && l.M <= 192 && !l.bf && !l.gstride) {
        // packed with the fp32 quantiser, or the fp16 Quantizer arithmetic (H16: ops.hadamard_quant / hadamard_quantizer / hadamard at 11008, 8960 ...)
        const int cq = l.ct & ~FQ_OUT_TRANSFORM;
        const bool yout = (l.ct & FQ_OUT_TRANSFORM) != 0;
        const bool yonly = yout && (cq & ~FQ_QUANT_F16) == 0 && l.n_clips == 0;
        const bool h16 = yonly || (cq == (FQ_OUT_PACKED | FQ_QUANT_F16) && l.round16);
        if (yout && (!l.y || !h16)) return none(FQ_LAUNCH_NO_KERNEL);
        if (!h16 && cq != FQ_OUT_PACKED) return none(FQ_LAUNCH_NO_KERNEL);
        if (yonly && l.M > 160) return none(FQ_LAUNCH_NO_KERNEL);   // (the rotation ALONE at six row tiles: fq_kron_tall.hip)
#define X(MT_, LKS_, G_) \
    if (l.MT == MT_ && l.lks == LKS_) return pick(FQ_KF_TILES, MT_, 2, 64, G_, LKS_, false, 0, h16);
        FQ_KRON_TILES64_LIST(X)
#undef X
        return none(FQ_LAUNCH_NO_KERNEL);
    }
    if (l.ct != FQ_OUT_PACKED || ((l.N & 15) && (l.M & 1))) return none(FQ_LAUNCH_NO_KERNEL);
#define X(MT_, NT_, N_, G_, LKS_, RS_, F16_) \
    if (l.N == N_ && l.MT == MT_ && l.lks == LKS_ && (l.bf || F16_)) return pick(FQ_KF_TILES, MT_, NT_, N_, G_, LKS_, RS_, l.bf, false);
    FQ_KRON_TILES_LIST(X)
#undef X
    return none(FQ_LAUNCH_NO_KERNEL);
}

// 64 < M <= 128, N = 128, f16, packed output (fp32 or fp16 Quantizer arithmetic): three token groups one phase apart
FqKronRoute trio(const Launch& l) {
    const bool h16 = l.ct == (FQ_OUT_PACKED | FQ_QUANT_F16) && l.round16;
    if (l.bf || l.N != 128 || (l.ct != FQ_OUT_PACKED && !h16)) return none(FQ_LAUNCH_NO_KERNEL);
#define X(MT_, H16_) \
    if (l.MT == MT_ && h16 == H16_) return pick(FQ_KF_TRIO, MT_, H16_, (l.M & 3) != 0);
    FQ_KRON_TRIO_LIST(X)
#undef X
    return none(FQ_LAUNCH_NO_KERNEL);
}

// 96 < M <= 128, N = 224, packed output: two token groups per CU
FqKronRoute duo(const Launch& l) {
    if (l.N != 224 || l.MT != 4 || l.post_scale || l.ct != FQ_OUT_PACKED) return none(FQ_LAUNCH_NO_KERNEL);
    return pick(FQ_KF_DUO, 4, l.M == 128, l.bf);
}

// 64 < M <= 192, N = 64, f16: a wave per ROW tile (172 x 64: Hadamard 11008)
FqKronRoute tall(const Launch& l) {
    if (l.bf || l.N != 64 || l.M <= 64 || l.gstride) return none(FQ_LAUNCH_NO_KERNEL);
    const int cq = l.ct & ~FQ_OUT_TRANSFORM;
    const bool yout = (l.ct & FQ_OUT_TRANSFORM) != 0;
    // the transform ALONE: the fp16-epilogue instantiation with no clip set (the quantiser loop does not run, the rounded pairs go out as they are)
    const bool yonly = yout && (cq & ~FQ_QUANT_F16) == 0 && l.n_clips == 0;
    const bool h16 = yonly || (cq == (FQ_OUT_PACKED | FQ_QUANT_F16) && l.round16);
    if ((cq != FQ_OUT_PACKED && !h16) || (yout && !l.y)) return none(FQ_LAUNCH_NO_KERNEL);
#define X(MT_, H16_, YOUT_) \
    if (l.MT == MT_ && h16 == H16_ && yout == YOUT_) return pick(FQ_KF_TALL, MT_, H16_, YOUT_);
    FQ_KRON_TALL_LIST(X)
#undef X
    return none(FQ_LAUNCH_NO_KERNEL);
}

// the workgroup-per-token kernel: `list` row (MT, NT, KS1) whose LDS fits, with the compile-time output set where one is instantiated
FqKronRoute fast(const Launch& l, bool silu, bool g128) {
    const bool ctf_ok = !l.bf && !g128 && (silu || l.MT >= 3);
    const int h16 = FQ_OUT_PACKED | FQ_QUANT_F16;
    const int ctf = !ctf_ok ? -1 : (l.ct == FQ_OUT_PACKED && !l.off(FQ_KF_NO_CTF)) ? FQ_OUT_PACKED : (l.ct == h16 && l.round16) ? h16 : -1;
    if (fq_kron_fast_lds(l.MT, l.KS1, l.M, l.N) > FQ_LDS_MAX) return none(FQ_LAUNCH_NO_KERNEL);
    // decode-sized SiLU.mul launches of 112 x 128: eight waves per token — the four without an n'-tile halve the rounds of the image copy and the token's loads
    if (silu && FQ_FS_DECODE_W != 4 && l.rows <= 64 && l.MT == 4 && l.NT == 4 && l.KS1 == 8 && l.ct == FQ_OUT_PACKED)
        return pick(FQ_KF_FAST, 4, 4, 8, FQ_FS_DECODE_W, 1, true, FQ_OUT_PACKED, 0, 0, false, false);
#define X(MT_, NT_, KS1_, W_, OCC_, BF16_) \
    if (l.MT == MT_ && l.NT == NT_ && l.KS1 == KS1_ && (!l.bf || BF16_)) return pick(FQ_KF_FAST, MT_, NT_, KS1_, W_, OCC_, silu, ctf, 0, l.bf, false, g128);
#define X5(...) X(__VA_ARGS__, true)
    if (silu) { FQ_KRON_FAST_SILU_LIST(X5) }
    else if (g128) { FQ_KRON_FAST_G128_LIST(X5) }
    else { FQ_KRON_FAST_LIST(X) }
#undef X5
#undef X
    return none(FQ_LAUNCH_NO_KERNEL);
}

// every pair with M <= 256, even N <= 256 and M * N <= 32768: run-time geometry, the L image in LDS if it fits
FqKronRoute general(const Launch& l) {
    const int waves = l.NT <= 4 ? 4 : 8;
    for (int llds = 1; llds >= 0; --llds)
        if (fq_kron_general_lds(l.MT, waves, llds, l.M, l.N) <= FQ_LDS_MAX) return pick(FQ_KF_GENERAL, l.MT, waves, llds, l.bf);
    return none(FQ_LAUNCH_NO_KERNEL);
}

}  // namespace

int fq_kron64_inst(int flags, int rt_flags, bool grouped) {
    const bool bf = (flags & FQ_DT_BF16) != 0;
    const int ct = flags & FQ_CT_MASK, k = grouped ? FQ_K64_GROUPED : 0;
    if (rt_flags & FQ_GROUP128)   // per-128-element scales: packed output, fp32 quantiser arithmetic only
        return ct == FQ_OUT_PACKED ? (FQ_OUT_PACKED | FQ_K64_G128 | k) : -1;
    if (grouped) {   // packed or fake-quant output (+ the transform); the all-low-precision quantiser (main_dpskv3.py:395) on the fake-quant output
        const int q = ct & ~FQ_OUT_TRANSFORM;
        return (q == FQ_OUT_PACKED || q == FQ_OUT_FAKEQUANT || q == (FQ_OUT_FAKEQUANT | FQ_QUANT_F16)) ? (ct | k) : -1;
    }
    if (ct & FQ_IN_RMSNORM) {   // (the RMSNorm-fused launches serve deploy.nn.RMSNorm, an fp16-only module in the reference)
        const int o = ct & ~FQ_IN_RMSNORM;
        return (!bf && (o == FQ_OUT_PACKED || o == FQ_OUT_TRANSFORM || o == (FQ_OUT_TRANSFORM | FQ_OUT_PACKED))) ? ct : -1;
    }
    if ((ct & ~FQ_QUANT_F16) == FQ_OUT_TRANSFORM) return FQ_OUT_TRANSFORM;
    return (ct & (FQ_OUT_PACKED | FQ_OUT_FAKEQUANT)) ? ct : -1;   // output set x fp16-quant arithmetic
}

FqKronRoute fq_kron_route(int flags, int64_t rows, int M, int N, bool diag, const FqQuantOut& out, int64_t ws_bytes, bool try_k64,
                          int masked) {
    Launch l;
    l.bf = (flags & FQ_DT_BF16) != 0;
    l.ct = flags & FQ_CT_MASK & ~FQ_IN_RMSNORM;
    l.rms = (flags & FQ_IN_RMSNORM) != 0;
    l.silu = (flags & FQ_IN_SILU_MUL) != 0;
    l.g128 = (out.rt_flags & FQ_GROUP128) != 0;
    l.round16 = (flags & FQ_ROUND_Y_F16) != 0;
    l.diag = diag, l.y = out.y != nullptr, l.fq0 = out.fq[0] != nullptr, l.in2 = out.in2 != nullptr;
    l.post_scale = out.post_scale != 0.0f, l.gstride = out.ws_group_stride != 0;
    l.n_clips = out.n_clips, l.M = M, l.N = N, l.rows = rows, l.masked = masked;
    l.MT = tiles32(M), l.NT = tiles32(N), l.KS1 = (N + 15) / 16, l.lks = (M + 15) >> 4;
    int ws_skip = 0;
    if (try_k64 && M == 64 && N == 64) {
        // the workspace is OPTIONAL at 64 x 64; the few fp16 output sets fq_kron64.hip has no instantiation for fall through to its second image
        const int k = fq_kron64_inst(flags, out.rt_flags, out.group_offsets != nullptr);
        if (k >= 0) return pick(FQ_KF_K64, k, false, l.bf);
        if (l.bf || (l.g128 && !l.round16)) return none(FQ_LAUNCH_NO_KERNEL);
        if (ws_bytes >= FQ_K64_WS_BYTES) ws_skip = (int)FQ_K64_IMAGE_BYTES;
    }
    if (M < 1 || N < 2 || (N & 1) || M > 256 || N > 256 || (int64_t)M * N > 32768) return none(FQ_LAUNCH_NO_KERNEL);
    // the specialised kernels: N in whole K-steps, M <= 192, 16-byte packed tokens; every other pair: fq_kron_general.hip
    const bool spec = !(N & 15) && M <= 192 && !((M * N / 2) & 15);
    // (the wave kernels take no post_scale; bf16 launches carry none: SiLU.mul / RMSNorm / post-scale are the deploy contract, fp16-only in the reference)
    const bool no_wave = (flags & FQ_NO_WAVE_KERNEL) != 0 || l.post_scale;
    if (l.bf && (l.silu || l.rms || l.post_scale)) return none(FQ_LAUNCH_NO_KERNEL);
    if (l.bf && l.g128 && !l.round16) return none(FQ_LAUNCH_NO_KERNEL);   // (the group epilogue quantises the rounded transform)
    if (l.silu) {   // fused for the down_proj shapes only; said before any workspace complaint
        bool listed = false;
#define X(MT_, NT_, KS1_, W_, OCC_) listed |= l.MT == MT_ && l.NT == NT_ && l.KS1 == KS1_;
        FQ_KRON_FAST_SILU_LIST(X)
#undef X
        if (!spec || !listed) return none(FQ_LAUNCH_NO_KERNEL);
    }
    if (ws_bytes - ws_skip < fq_kron_generic_workspace_bytes(M, N)) return none(FQ_LAUNCH_NEED_WS);
    FqKronRoute r = none(FQ_LAUNCH_NO_KERNEL);
    if (l.silu) {
        if (!diag && l.in2 && !l.g128) r = fast(l, true, false);
    } else if (l.rms) {   // fused RMSNorm: the wave-per-token kernel (packed output) is the one that has it
        if (spec && !no_wave && !diag) r = wave(l);
    } else {
        if (spec && !no_wave && !l.off(FQ_KF_WAVE)) r = wave(l);
        // per-128-element scales: the wave kernel above (N = 64, packed, fp32 accumulator) or the group epilogue of the workgroup-per-token
        // kernel's all-output-sets instantiations (the transform rounded to the activation dtype)
        const bool groups = !diag && !l.g128 && (spec || N == 148);   // the token-group kernels: no diag multiply, no group epilogue
        if (r.rc && groups && !l.off(FQ_KF_TILES)) r = tiles(l);
        if (r.rc && groups && spec && !l.off(FQ_KF_TRIO)) r = trio(l);
        if (r.rc && groups && spec && !l.off(FQ_KF_DUO)) r = duo(l);
        if (r.rc && groups && spec && !l.off(FQ_KF_TALL)) r = tall(l);
        if (r.rc && spec && (!l.g128 || l.round16)) r = fast(l, false, l.g128);
        if (r.rc && !l.g128) r = general(l);   // (the general kernel has no group epilogue)
    }
    r.ws_skip = ws_skip;
    return r;
}

int fq_kron_route_name(const FqKronRoute& r, char* buf, int cap) {
    static const struct { const char* name; int n, type; } fam[FQ_KF_COUNT] = {
        {"fq_kron64_kernel", 3, 2}, {"fq_kron_wave_kernel", 7, 5}, {"fq_kron_tiles_kernel", 8, 6}, {"fq_kron_trio_kernel", 3, -1},
        {"fq_kron_duo_kernel", 3, 2}, {"fq_kron_tall_kernel", 3, -1}, {"fq_kron_fast_kernel", 11, 8}, {"fq_kron_general_kernel", 4, 3}};
    int n = snprintf(buf, cap, "%d", r.rc);
    if (r.rc != 0) return n < cap ? n : -1;
    n = snprintf(buf, cap, "%s<", fam[r.family].name);
    for (int i = 0; i < fam[r.family].n && n < cap; ++i) {
        if (i == fam[r.family].type) n += snprintf(buf + n, cap - n, "%s%s", i ? "," : "", r.t[i] ? "bf16" : "f16");
        else n += snprintf(buf + n, cap - n, "%s%d", i ? "," : "", r.t[i]);
    }
    if (n < cap) n += snprintf(buf + n, cap - n, ">");
    return n < cap ? n : -1;
}
