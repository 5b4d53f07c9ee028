// fq_kron_generic.hip — fused Kronecker transform + per-token INT4 quantisation, ONE WORKGROUP PER TOKEN, for the factor
// pairs deployed models use whose token does not fit a wave or whose output set is not packed-only: d = 14336 (112x128),
// 28672 (128x224), 11008 (86x128), 8192 (64x128), 7168 (64x112), 2048 (32x64), 3584 (56x64), 5120 (64x80), 18432 (128x144),
// 27648 (144x192), 29568 (168x176), 8960 (80x112), and — packed-only, true row length as a template parameter — 18944 (128x148)
// (function_utils.py:11-21 factor pairs); plus the fragment-image builder (fq_kron_prepare_kernel) and fq_launch_kron, which runs
// the kernel fq_kron_route (fq_kron_route.hip) named for a launch: the image first, then the family's launcher. WHICH kernel — the
// order of preference among the families, their preconditions, the instantiation lists — is stated there and in fq_kron_route.hpp only.
//
// Same mathematics and fragment chaining as fq_kron64.hip (U = X.R rounded to fp16, Y^T = U^T.L, the C
// fragment of GEMM 1 is the A fragment of GEMM 2), but a token no longer fits one wave's registers, so:
//   * one 4- or 8-wave workgroup owns one token; the token is staged in LDS once (coalesced 16-byte loads, row
//     pitch padded to an odd number of 16-byte chunks -> conflict-free ds_read_b128 A fragments);
//   * wave w computes the 32-column n'-tiles w, w+WAVES, ...: GEMM 1 for its tile over all rows, fp16
//     conversion in registers, GEMM 2 against all of L; its slice of Y stays in registers;
//   * the B-operand fragments of R and L come from a caller-provided WORKSPACE in fragment order
//     (fq_kron_prepare_kernel, launched by the same C-ABI call; <= 170 KB, L2-resident);
//   * per-token max/min: wave all-reduce + 8 floats of LDS; quantised nibbles / fp16 outputs are staged in
//     LDS and written out with full 16-byte coalesced stores.
// This single pass replaces the reference's split path for M > 64 (kron_matmul.py:213-247), which writes the
// fp16 intermediate to HBM and re-reads it (+4 B/element).
#include "fq_kron_fast.hpp"

namespace {

// Workspace layout: rfrag [NT][KS1][64 lanes] uint4, then lfrag [2*MT][MT][64 lanes] uint4.
// blockIdx.y = group (fq_kron_quant_grouped_mats_*: left [G, M, M], right [G, N, N], one image per group; 0 otherwise).
__global__ void fq_kron_prepare_kernel(const f16* __restrict__ left, const f16* __restrict__ right, int M, int N,
                                       int MT, int NT, int KS1, uint4* __restrict__ ws) {
    const int n_r = NT * KS1 * 64, n_l = 2 * MT * MT * 64;
    left += (size_t)blockIdx.y * M * M;
    right += (size_t)blockIdx.y * N * N;
    ws += (size_t)blockIdx.y * (n_r + n_l);
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < n_r + n_l; item += gridDim.x * blockDim.x) {
        f16x8 v;
        if (item < n_r) {
            const int f = item >> 6, ln = item & 63, h = ln >> 5, c = ln & 31;
            const int nt = f / KS1, s = f - nt * KS1;
            const int np = ncol(NT, nt, c);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int n = s * 16 + h * 8 + j;
                v[j] = (n < N && np < N) ? right[n * N + np] : (f16)0.0f;
            }
        } else {
            const int it = item - n_r;
            const int f = it >> 6, ln = it & 63, h = ln >> 5, c = ln & 31;
            const int ks = f / MT, mo = f - ks * MT;
            const int mp = mo * 32 + c;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int m = (ks >> 1) * 32 + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3);
                v[j] = (m < M && mp < M) ? left[m * M + mp] : (f16)0.0f;
            }
        }
        ws[item] = __builtin_bit_cast(uint4, v);
    }
}

}  // namespace

int64_t fq_kron_generic_workspace_bytes(int M, int N) {
    const int MT = tiles32(M), NT = tiles32(N), KS1 = (N + 15) / 16;
    return ((int64_t)NT * KS1 + 2 * (int64_t)MT * MT) * 1024;
}

int fq_launch_kron_prepare(const f16* left, const f16* right, int M, int N, void* workspace, hipStream_t stream, int groups) {
    const int MT = tiles32(M), NT = tiles32(N), KS1 = (N + 15) / 16;
    const int items = (NT * KS1 + 2 * MT * MT) * 64;
    hipLaunchKernelGGL(fq_kron_prepare_kernel, dim3((items + 255) / 256, groups), dim3(256), 0, stream, left, right, M, N, MT,
                       NT, KS1, reinterpret_cast<uint4*>(workspace));
    return (int)hipGetLastError();
}

// The f16 instantiations without the group epilogue (bf16, group-128: fq_launch_kron_fast2, fq_kron_generic2.hip).
template <int MT, int NT, int KS1, int W, int OCC, bool SILU>
static int launch_fast_ct(const FqKronRoute& r, const FqKronArgs& a, const FqQuantOut& out) {
    const f16 *x = (const f16*)a.x, *diag = (const f16*)a.diag;
    const uint4* ws = reinterpret_cast<const uint4*>(a.ws);
    if constexpr (SILU || MT >= 3) {   // the rows with a compile-time output set
        if (r.t[6] == FQ_OUT_PACKED) return launch_fast<MT, NT, KS1, W, OCC, SILU, FQ_OUT_PACKED>(a.flags, x, ws, diag, a.rows, a.M, a.N, out, a.n_cu, a.stream);
        if (r.t[6] == (FQ_OUT_PACKED | FQ_QUANT_F16))
            return launch_fast<MT, NT, KS1, W, OCC, SILU, FQ_OUT_PACKED | FQ_QUANT_F16>(a.flags, x, ws, diag, a.rows, a.M, a.N, out, a.n_cu, a.stream);
    }
    return launch_fast<MT, NT, KS1, W, OCC, SILU>(a.flags, x, ws, diag, a.rows, a.M, a.N, out, a.n_cu, a.stream);
}

int fq_launch_kron_fast(const FqKronRoute& r, const FqKronArgs& a, const FqQuantOut& out) {
    if (r.t[8] || r.t[10]) return fq_launch_kron_fast2(r, a, out);
#define X(MT_, NT_, KS1_, W_, OCC_) \
    if (r.t[0] == MT_ && r.t[1] == NT_ && r.t[2] == KS1_ && r.t[3] == W_) return launch_fast_ct<MT_, NT_, KS1_, W_, OCC_, true>(r, a, out);
    if (r.t[5]) {
        if (FQ_FS_DECODE_W != 4 && r.t[1] == 4 && r.t[3] == FQ_FS_DECODE_W)   // the decode form of 112 x 128 (fq_kron_route.hip)
            return launch_fast<4, 4, 8, FQ_FS_DECODE_W, 1, true, FQ_OUT_PACKED>(a.flags, (const f16*)a.x, reinterpret_cast<const uint4*>(a.ws), (const f16*)a.diag,
                                                                                a.rows, a.M, a.N, out, a.n_cu, a.stream);
        FQ_KRON_FAST_SILU_LIST(X)
        return FQ_LAUNCH_NO_KERNEL;
    }
#undef X
#define X(MT_, NT_, KS1_, W_, OCC_, BF16_) \
    if (r.t[0] == MT_ && r.t[1] == NT_ && r.t[2] == KS1_) return launch_fast_ct<MT_, NT_, KS1_, W_, OCC_, false>(r, a, out);
    FQ_KRON_FAST_LIST(X)
#undef X
    return FQ_LAUNCH_NO_KERNEL;
}

// Which kernel: fq_kron_route. This is the rest of a launch — the fragment image, then the route's family.
int fq_launch_kron(const FqKronRoute& r, int flags, const f16* x, const f16* left, const f16* right, const f16* diag, int64_t rows, int M, int N,
                   const FqQuantOut& out, void* workspace, int n_cu, hipStream_t stream) {
    if (r.rc != 0) return r.rc;
    workspace = static_cast<unsigned char*>(workspace) + r.ws_skip;
    if (!(flags & FQ_WS_PREPARED)) {   // the fragment image is a re-arrangement of 16-bit words: the same kernel for both types
        const int rc = fq_launch_kron_prepare(left, right, M, N, workspace, stream);
        if (rc != 0) return rc;
    }
    flags &= ~(FQ_WS_PREPARED | FQ_NO_WAVE_KERNEL | FQ_DT_BF16 | FQ_IN_SILU_MUL);
#ifdef FQ_MEASURE
    if (const char* dbg = getenv("FQ_KRON_DBG"))   // measurement: ablation bits of the fast kernel
        if (r.family == FQ_KF_FAST || r.family == FQ_KF_GENERAL) flags |= atoi(dbg) & 0x7000;
#endif
    const FqKronArgs a = {flags, x, workspace, diag, rows, M, N, n_cu, stream};
    switch (r.family) {
        case FQ_KF_WAVE: return fq_launch_kron_wave(r, a, out);
        case FQ_KF_TILES: return fq_launch_kron_tiles(r, a, out);
        case FQ_KF_TRIO: return fq_launch_kron_trio(r, a, out);
        case FQ_KF_DUO: return fq_launch_kron_duo(r, a, out);
        case FQ_KF_TALL: return fq_launch_kron_tall(r, a, out);
        case FQ_KF_FAST: return fq_launch_kron_fast(r, a, out);
        case FQ_KF_GENERAL: return fq_launch_kron_general(r, a, out);
    }
    return FQ_LAUNCH_NO_KERNEL;
}

int fq_launch_kron_generic(int flags, const f16* x, const f16* left, const f16* right, const f16* diag,
                           int64_t rows, int M, int N, const FqQuantOut& out, void* workspace,
                           int64_t workspace_bytes, int n_cu, hipStream_t stream) {
    const FqKronRoute r = fq_kron_route(flags, rows, M, N, diag != nullptr, out, workspace ? workspace_bytes : 0, false, fq_kron_measure_mask());
    return fq_launch_kron(r, flags, x, left, right, diag, rows, M, N, out, workspace, n_cu, stream);
}
