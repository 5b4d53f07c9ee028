// fq_kron_generic2.hip — second translation unit of the workgroup-per-token Kronecker kernel (fq_kron_fast.hpp): the bf16
// instantiations (path-A surface: kronecker_matmul, {Inv,SVD}DecomposeTransMatrix, the fake-quant contract on bf16 activations),
// the launches with one factor pair per group (fq_kron_quant_grouped_mats_*, deepseekv3_utils.py:443-446) and the group-128
// epilogue instantiations (ActivationQuantizer(groupsize=128), fake_quant_utils.py:72-78): fq_launch_kron_fast2. Which launch runs
// which: fq_kron_route.hip.
#include "fq_kron_fast.hpp"

// Grouped launch in which every group has its own factor pair (fq_kron_quant_grouped_mats_{f16,bf16}): left [G, M, M],
// right [G, N, N]; the workspace holds G fragment images. The workgroup-per-token kernel (all output sets) for the factor pairs
// it is instantiated for; FQ_LAUNCH_NO_KERNEL otherwise.
template <typename T>
static int launch_kron_grouped_mats_t(int flags, const T* x, const T* left, const T* right, int64_t rows, int M, int N,
                                      FqQuantOut out, int n_groups, void* workspace, int64_t workspace_bytes, int n_cu,
                                      hipStream_t stream) {
    if (M < 1 || N < 2 || (N & 15) || M > 192 || ((M * N / 2) & 15)) return FQ_LAUNCH_NO_KERNEL;
    const int64_t img = fq_kron_generic_workspace_bytes(M, N);
    if (!workspace || workspace_bytes < img * n_groups) return FQ_LAUNCH_NEED_WS;
    if (!(flags & FQ_WS_PREPARED)) {
        const int rc = fq_launch_kron_prepare((const f16*)left, (const f16*)right, M, N, workspace, stream, n_groups);
        if (rc != 0) return rc;
    }
    flags &= ~FQ_WS_PREPARED;
    out.ws_group_stride = img / 16;
    const int MT = tiles32(M), NT = tiles32(N), KS1 = N / 16;
    const uint4* ws = reinterpret_cast<const uint4*>(workspace);
#define FQ_FG(MT_, NT_, KS1_, W_, OCC_)                                                                                  \
    if (MT == MT_ && NT == NT_ && KS1 == KS1_)                                                                           \
        return launch_fast<MT_, NT_, KS1_, W_, OCC_, false, -1, 0, T, true>(flags, x, ws, (const T*)nullptr, rows, M, N, out, n_cu, stream);
    // (the pairs an expert's hidden / model dimension decomposes into: 32x64 = 2048 DeepSeek-V3 moe_inter, 64x112 = 7168,
    //  64x64, 56x64, 64x128, 64x80, 112x128, 86..96x128)
    FQ_FG(1, 2, 4, 4, 4) FQ_FG(2, 2, 4, 4, 2) FQ_FG(2, 4, 7, 4, 2) FQ_FG(2, 4, 8, 4, 2) FQ_FG(2, 3, 5, 4, 2) FQ_FG(4, 4, 8, 4, 2)
    FQ_FG(3, 4, 8, 4, 2)
#undef FQ_FG
    return FQ_LAUNCH_NO_KERNEL;
}

int fq_launch_kron_grouped_mats(int flags, const void* x, const void* left, const void* right, int64_t rows, int M, int N,
                                const FqQuantOut& out, int n_groups, void* workspace, int64_t workspace_bytes, int n_cu,
                                hipStream_t stream) {
    if (flags & FQ_DT_BF16)
        return launch_kron_grouped_mats_t<bf16>(flags & ~FQ_DT_BF16, (const bf16*)x, (const bf16*)left, (const bf16*)right, rows, M,
                                                N, out, n_groups, workspace, workspace_bytes, n_cu, stream);
    return launch_kron_grouped_mats_t<f16>(flags, (const f16*)x, (const f16*)left, (const f16*)right, rows, M, N, out, n_groups,
                                           workspace, workspace_bytes, n_cu, stream);
}

// bf16 activations (the path-A surface: kronecker_matmul, {Inv,SVD}DecomposeTransMatrix, the fake-quant contract): the all-output-sets
// instantiation for the factor pairs of the supported model families; and the group-128 epilogue (FQ_GROUP128 with FQ_ROUND_Y_F16:
// ActivationQuantizer(groupsize=128)) on both types.
template <int MT, int NT, int KS1, int W, int OCC, bool G128>
static int launch_fast_t(const FqKronRoute& r, const FqKronArgs& a, const FqQuantOut& out) {
    const uint4* ws = reinterpret_cast<const uint4*>(a.ws);
    if (r.t[8]) return launch_fast<MT, NT, KS1, W, OCC, false, -1, 0, bf16, false, G128>(a.flags, (const bf16*)a.x, ws, (const bf16*)a.diag, a.rows, a.M, a.N, out, a.n_cu, a.stream);
    if constexpr (G128) return launch_fast<MT, NT, KS1, W, OCC, false, -1, 0, f16, false, true>(a.flags, (const f16*)a.x, ws, (const f16*)a.diag, a.rows, a.M, a.N, out, a.n_cu, a.stream);
    return FQ_LAUNCH_NO_KERNEL;   // (f16 without the group epilogue: fq_launch_kron_fast)
}

int fq_launch_kron_fast2(const FqKronRoute& r, const FqKronArgs& a, const FqQuantOut& out) {
#define X(MT_, NT_, KS1_, W_, OCC_) \
    if (r.t[0] == MT_ && r.t[1] == NT_ && r.t[2] == KS1_) return launch_fast_t<MT_, NT_, KS1_, W_, OCC_, true>(r, a, out);
    if (r.t[10]) {
        FQ_KRON_FAST_G128_LIST(X)
        return FQ_LAUNCH_NO_KERNEL;
    }
#undef X
#define X(MT_, NT_, KS1_, W_, OCC_, BF16_)                             \
    if constexpr (BF16_)                                                \
        if (r.t[0] == MT_ && r.t[1] == NT_ && r.t[2] == KS1_) return launch_fast_t<MT_, NT_, KS1_, W_, OCC_, false>(r, a, out);
    FQ_KRON_FAST_LIST(X)
#undef X
    return FQ_LAUNCH_NO_KERNEL;
}
