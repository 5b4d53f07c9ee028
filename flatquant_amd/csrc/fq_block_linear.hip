// fq_block_linear.hip — THE HEAD TRANSFORM AS THE GEMM'S PROLOGUE, decode regime: the o_proj input transform across heads
// (x[t] [head_dim, heads] . P [heads, heads], deploy/kernels/block_matmul.py:29-104), its per-token INT4 quantiser and the Linear4bit behind
// it (deploy/nn/linear.py:40-54) as ONE launch for M <= 16 tokens of hidden size 4096 (R = 128, C = 32) — modeling_llama.py:141-148, the
// launch pair fq_block_quant_f16 -> fq_int4_skinny_linear_f16 of the captured decode step, the last transform + GEMM pair of the step that
// was two dependent launches (fq_kron64_linear_kernel, fq_kron64.hip, removed the others).
//
// The structure is fq_kron64_linear_kernel's with another stage 2. Every persistent workgroup (8 waves)
//   1. requests P (2 KB), the A fragments of its tokens (8 KB each, straight from HBM into registers as the C = 32 variant of fq_block_kernel
//      loads them: 16-byte loads, 2 KB contiguous per instruction) and its first TWO feature tiles of weights at once,
//   2. transforms and quantises the M tokens itself — a wave per token (waves w, w + 8): eight v_mfma_f32_32x32x16_f16, the k order, the row
//      permutation (rmap), the extrema, fq_token_scale and the quantiser of fq_block_kernel<4, 1, false, NAT = false, PK = true> — while the
//      weights are in flight, and leaves the token's 2 KB of packed digits in LDS in K order (k = c R + r: the transposed [C][R] packed row
//      the two-launch form stores) with the fp16-rounded scale next to them,
//   3. walks its feature tiles exactly as fq_kron64_linear_kernel does: two-slot weight ring, int8 MFMAs over the 8 waves' K shares, ds_add
//      reduction, sym_dequant + bias epilogue, counted waits.
// 128 .. 256 workgroups repeat 4096 x 32 MACs per token (a quarter of what the 64 x 64 Kronecker prologue repeats); nobody waits for a
// producer launch and the quantised activations never reach memory. Bit-identical to the two launches (tests/test_gpu_head_linear.py).
//
// The code of stages 1 and 3 is a COPY of fq_kron64_linear_kernel's, not shared with it: that kernel's register allocation and schedule
// were tuned by hand around its inline-asm waits, and its lines of the resource report are held fixed (tests/test_head_linear_cpu.py).
// As there, every VMEM operation is inline asm so that the compiler's own s_waitcnt bookkeeping never waits for the prefetched weights.
#include "fq_common.hpp"
#include "fq_gemm_common.hpp"
#include "fq_launch.hpp"

namespace {

constexpr int BL_WAVES = 8, BL_THREADS = BL_WAVES * 64, BL_MAXM = 16;
constexpr int BL_R = 128, BL_C = 32, BL_K = BL_R * BL_C, BL_RT = BL_R / 32, BL_KS = BL_C / 16;
constexpr int BL_KB = BL_K / 64;                  // 64-k blocks of a weight row tile
constexpr int BL_BPW = BL_KB / BL_WAVES;          // blobs per wave and tile: 8
constexpr int BL_PFRAG_BYTES = BL_KS * 64 * 16;   // P in MFMA B-fragment order: [s][lane] x 16 B
// a token's packed digits in LDS: 2 KB + 16 B, so that the 16 tokens' B-fragment reads of stage 3 (one ds_read_b128 per lane, lane c reads
// token c at the same offset) fall into 16 different 16-byte bank groups instead of one
constexpr int BL_TOK_STRIDE = BL_K / 2 + 16;
typedef int bl_i32x16 __attribute__((ext_vector_type(16)));

// physical row supplied by A-fragment lane index i of row tile rt: lane (h, c') of the C/D fragment ends with the 64 consecutive rows
// r = 64 h .. 64 h + 63 of output column c' (fq_block.hip, rmap with RT = 4)
__device__ __forceinline__ int bl_rmap(int rt, int i) { return ((i >> 2) & 1) * (BL_RT * 16) + rt * 16 + (i & 3) + 4 * (i >> 3); }

// Loads whose completion is waited for by hand; "+v": the destination is the register the variable already lives in (fq_kron64.hip, kl_load16)
__device__ __forceinline__ void bl_load16(u32x4& d, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off nt" : "+v"(d) : "v"(p) : "memory"); }
__device__ __forceinline__ void bl_load2(unsigned& d, const void* p) { asm volatile("global_load_ushort %0, %1, off" : "+v"(d) : "v"(p) : "memory"); }
// ONE asm statement per wait, the count selected at run time inside it (sel 0..3): fq_kron64.hip, KL_WAIT4
#define BL_WAIT4(sel, C0, C1, C2, C3, ...)                                                                               \
    asm volatile("s_cmp_eq_u32 %[n], 0\n\ts_cbranch_scc1 5f\n\ts_cmp_eq_u32 %[n], 1\n\ts_cbranch_scc1 6f\n\t"           \
                 "s_cmp_eq_u32 %[n], 2\n\ts_cbranch_scc1 7f\n\ts_waitcnt vmcnt(" #C3 ")\n\ts_branch 9f\n"                \
                 "5:\n\ts_waitcnt vmcnt(" #C0 ")\n\ts_branch 9f\n6:\n\ts_waitcnt vmcnt(" #C1 ")\n\ts_branch 9f\n"        \
                 "7:\n\ts_waitcnt vmcnt(" #C2 ")\n9:"                                                                   \
                 : __VA_ARGS__ : [n] "s"(__builtin_amdgcn_readfirstlane(sel)) : "scc", "memory")

__global__ __launch_bounds__(BL_THREADS) void fq_block_linear_kernel(const f16* __restrict__ x, const f16* __restrict__ P, int M, float sig_max,
                                                                     float sig_min, int rt_flags, const uint4* __restrict__ wimg,
                                                                     const f16* __restrict__ scol, const f16* __restrict__ bias, int N,
                                                                     f16* __restrict__ yout) {
    using namespace fqgemm;
    extern __shared__ __attribute__((aligned(16))) unsigned char blsm[];
    // [P fragments 2 KB][M packed tokens, BL_TOK_STRIDE apart][tile sums 2 x 32 x 33 int][scales 16 float]
    uint4* pfrag = reinterpret_cast<uint4*>(blsm);
    unsigned char* digs = blsm + BL_PFRAG_BYTES;
    int (*tile)[32][33] = reinterpret_cast<int (*)[32][33]>(digs + (size_t)M * BL_TOK_STRIDE);
    float* sc_lds = reinterpret_cast<float*>(digs + (size_t)M * BL_TOK_STRIDE + 2 * 32 * 33 * 4);
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, c = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_tiles = N >> 5, step = (int)gridDim.x;
    const int t0 = (int)blockIdx.x;                        // tiles t0, t0 + step, ...
    const f16* bsrc = bias != nullptr ? bias : scol;       // (a dummy source keeps the number of loads per tile fixed: the waits below count them)

    // ---- 1. everything this workgroup needs from memory, requested at once ----
    // P's B fragments: slot (s, lane (fh, fc)) = P[16 s + 8 fh .. + 8][fc], gathered by threads 0..127 (the others repeat the same addresses:
    // every wave issues the same number of loads)
    unsigned gp[8] = {};
    {
        const int item = tid & 127, s = item >> 6, fh = (item >> 5) & 1, fc = item & 31;
        const f16* pp = P + (s * 16 + fh * 8) * BL_C + fc;
#pragma unroll
        for (int j = 0; j < 8; ++j) bl_load2(gp[j], pp + j * BL_C);
    }
    // the A fragments of this wave's tokens (wave-uniform: 8 loads per token, older than every weight request): lane (h, c) of row tile rt
    // supplies row rmap(rt, c), k = 16 s + 8 h .. + 8
    u32x4 XA[2][BL_RT][BL_KS] = {};
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
        const int m = wave + rd * BL_WAVES;
        if (m < M) {
#pragma unroll
            for (int rt = 0; rt < BL_RT; ++rt) {
                const f16* xp = x + (size_t)m * BL_K + bl_rmap(rt, c) * BL_C + h * 8;
#pragma unroll
                for (int s = 0; s < BL_KS; ++s) bl_load16(XA[rd][rt][s], xp + s * 16);
            }
        }
    }
    // weights of two tiles in flight per wave: ring slot = tile parity; + the tile's column scale and bias for this thread's output element
    u32x4 W0[BL_BPW] = {}, W1[BL_BPW] = {};
    unsigned s0 = 0, b0 = 0, s1 = 0, b1 = 0;
    const int nl = tid & 31, mrow = tid >> 5;              // the output element of this thread in a tile: token mrow (clamped below), feature nl
#define BL_REQ(Wr, sr, br, t)                                                                                     \
    {                                                                                                             \
        const uint4* wp_ = wimg + ((size_t)(t) * BL_KB + wave) * 64 + lane;                                       \
        _Pragma("unroll") for (int j = 0; j < BL_BPW; ++j) bl_load16(Wr[j], wp_ + (size_t)j * BL_WAVES * 64);     \
        bl_load2(sr, scol + (t) * 32 + nl);                                                                       \
        bl_load2(br, bsrc + (t) * 32 + nl);                                                                       \
    }
    const bool have0 = t0 < n_tiles, have1 = t0 + step < n_tiles;
    if (have0) BL_REQ(W0, s0, b0, t0)
    if (have1) BL_REQ(W1, s1, b1, t0 + step)
    // P and the tokens are older than the weights: wait for them only (10 loads per requested tile stay in flight)
    {
        const int sel = have1 ? 2 : have0 ? 1 : 0;
#define BL_XA(rd) "+v"(XA[rd][0][0]), "+v"(XA[rd][0][1]), "+v"(XA[rd][1][0]), "+v"(XA[rd][1][1]), "+v"(XA[rd][2][0]), "+v"(XA[rd][2][1]), \
                  "+v"(XA[rd][3][0]), "+v"(XA[rd][3][1])
        BL_WAIT4(sel, 0, 10, 20, 20, "+v"(gp[0]), "+v"(gp[1]), "+v"(gp[2]), "+v"(gp[3]), "+v"(gp[4]), "+v"(gp[5]), "+v"(gp[6]), "+v"(gp[7]),
                 BL_XA(0), BL_XA(1));
#undef BL_XA
    }
    if (tid < BL_KS * 64)
        pfrag[tid] = make_uint4(gp[0] | (gp[1] << 16), gp[2] | (gp[3] << 16), gp[4] | (gp[5] << 16), gp[6] | (gp[7] << 16));
    for (int i = tid; i < 2 * 32 * 33; i += BL_THREADS) (&tile[0][0][0])[i] = 0;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                          // P's fragments are in LDS (the tokens: every wave waited for its own loads)

    // ---- 2. transform + quantise: wave w takes tokens w, w + 8 (fq_block_kernel<4, 1, false, false, true>, one token) ----
    const int qflags = FQ_OUT_PACKED | (rt_flags & FQ_NO_CLAMP0);
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
        const int m = wave + rd * BL_WAVES;
        if (m >= M) continue;
        const uint4* myp = pfrag + lane;
        f32x16 Y[BL_RT];
#pragma unroll
        for (int rt = 0; rt < BL_RT; ++rt) {
            Y[rt] = f32x16{0};
#pragma unroll
            for (int s = 0; s < BL_KS; ++s)
                Y[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, XA[rd][rt][s]), __builtin_bit_cast(f16x8, myp[s * 64]), Y[rt], 0, 0, 0);
        }
        // The first readers of the accumulators are the inline-asm max / min below, and the compiler pads no MFMA -> VALU hazard for a reader
        // inside an asm string (found on the GPU: with the extrema interleaved behind each tile's MFMA the token's scale came from stale
        // registers). All eight MFMAs first, then the wait states of the last one (an 8-pass XDL result needs 12; 20 given), nothing moved across.
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(Y[0]), "+v"(Y[1]), "+v"(Y[2]), "+v"(Y[3]));
        __builtin_amdgcn_sched_barrier(0);
        // lane (h, c) now holds, for column c, rows r = 64 h + 16 rt + reg
        float pmx[BL_RT], pmn[BL_RT];  // one independent max3 / min3 chain per tile
#pragma unroll
        for (int rt = 0; rt < BL_RT; ++rt) {
            const f32x16& t = Y[rt];
            float a = FqMaxOp()(t[0], t[1]), b = FqMinOp()(t[0], t[1]);
#pragma unroll
            for (int r = 2; r < 16; r += 2) {
                a = fq_max3(a, t[r], t[r + 1]);
                b = fq_min3(b, t[r], t[r + 1]);
            }
            pmx[rt] = a;
            pmn[rt] = b;
        }
        float vmax = pmx[0], vmin = pmn[0];
#pragma unroll
        for (int k = 1; k < BL_RT; ++k) {
            vmax = fmaxf(vmax, pmx[k]);
            vmin = fminf(vmin, pmn[k]);
        }
        vmax = fq_wave_max(vmax);
        vmin = fq_wave_min(vmin);
        const float scale = fq_token_scale<0>(vmax, vmin, sig_max, sig_min, qflags);
        const float inv = fq_fast_inv(scale);
        const bool magic = fq_magic_ok(vmax, vmin, inv), clampq = fq_needs_clamp(vmax, vmin, inv);
        const float ilo = fq_inv_lo(inv), ihi = fq_inv_hi(inv);
        if (lane == 0) sc_lds[m] = (float)(f16)scale;      // (the fp16 scale the packed launch stores and the GEMM reads)
        // the token's transposed packed row [C][R / 2]: column c, bytes 32 h .. + 32
        unsigned char* qrow = digs + (size_t)m * BL_TOK_STRIDE + c * (BL_R / 2) + h * (BL_RT * 8);
        uint2 pk[BL_RT];
#pragma unroll
        for (int i = 0; i < BL_RT; ++i) {
            const f32x16& t = Y[i];
            unsigned long long d0 = ~0ull, d1 = ~0ull;
            pk[i] = uint2{0u, 0u};
            if (magic) {
                if (clampq) {
                    pk[i].x = fq_quant8<true>(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], inv, ilo, ihi, d0);
                    pk[i].y = fq_quant8<true>(t[8], t[9], t[10], t[11], t[12], t[13], t[14], t[15], inv, ilo, ihi, d1);
                } else {
                    pk[i].x = fq_quant8<false>(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], inv, ilo, ihi, d0);
                    pk[i].y = fq_quant8<false>(t[8], t[9], t[10], t[11], t[12], t[13], t[14], t[15], inv, ilo, ihi, d1);
                }
            }
            if (d0)  // rare: an ambiguous digit somewhere in the wave -> the true division for this dword
                pk[i].x = fq_pack8(fq_qexact(t[0], scale), fq_qexact(t[1], scale), fq_qexact(t[2], scale), fq_qexact(t[3], scale),
                                   fq_qexact(t[4], scale), fq_qexact(t[5], scale), fq_qexact(t[6], scale), fq_qexact(t[7], scale));
            if (d1)
                pk[i].y = fq_pack8(fq_qexact(t[8], scale), fq_qexact(t[9], scale), fq_qexact(t[10], scale), fq_qexact(t[11], scale),
                                   fq_qexact(t[12], scale), fq_qexact(t[13], scale), fq_qexact(t[14], scale), fq_qexact(t[15], scale));
            if (i & 1) *reinterpret_cast<uint4*>(qrow + (i - 1) * 8) = make_uint4(pk[i - 1].x, pk[i - 1].y, pk[i].x, pk[i].y);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    // ---- 3. the feature tiles (fq_kron64_linear_kernel's stage 3) ----
    // B fragments of this wave's 8 k-blocks: token min(c, M - 1), packed bytes 32 kb + 16 h .. (loop-invariant: registers)
    u32x4 BX[BL_BPW];
    {
        const unsigned char* xr = digs + (size_t)(c < M ? c : M - 1) * BL_TOK_STRIDE + 16 * h;
#pragma unroll
        for (int j = 0; j < BL_BPW; ++j) BX[j] = *reinterpret_cast<const u32x4*>(xr + (wave + j * BL_WAVES) * 32);
    }
    const int mo_ = mrow < M ? mrow : M - 1;               // rows >= M hold copies of token M - 1: the same value to the same address
    const f16 srow = (f16)sc_lds[mo_];
    int par = 0;
    auto consume = [&](u32x4 (&Wr)[BL_BPW]) {
        bl_i32x16 acc = bl_i32x16{0};
#pragma unroll
        for (int j = 0; j < BL_BPW; ++j) {
            const i32x4_t a0 = unpack16(make_uint2(Wr[j][0], Wr[j][1])), a1 = unpack16(make_uint2(Wr[j][2], Wr[j][3]));
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, unpack16(make_uint2(BX[j][0], BX[j][1])), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, unpack16(make_uint2(BX[j][2], BX[j][3])), acc, 0, 0, 0);
        }
        return acc;
    };
    auto finish = [&](const bl_i32x16& acc, unsigned sr, unsigned br, int t) {
        // lane (h, c): token c, features 16 h + r; the eight waves' partial sums meet in LDS
#pragma unroll
        for (int r = 0; r < 16; ++r) atomicAdd(&tile[par][c][16 * h + r], acc[r]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const int v = tile[par][mrow][nl] >> 8;            // products carry 256 (unpack16)
        f16 yv = dequant1(v, srow, __builtin_bit_cast(f16, (unsigned short)sr));
        if (bias != nullptr) yv = yv + __builtin_bit_cast(f16, (unsigned short)br);
        const unsigned yb = (unsigned)__builtin_bit_cast(unsigned short, yv);
        f16* dst = yout + (size_t)mo_ * N + t * 32 + nl;
        asm volatile("global_store_short %0, %1, off" : : "v"(dst), "v"(yb) : "memory");
        tile[par][mrow][nl] = 0;                           // (this buffer is next used two tiles on: a barrier lies in between)
        par ^= 1;
    };
    for (int t = t0; t < n_tiles; t += 2 * step) {
        // Issue order of an iteration: [wait slot 0] MFMAs, request slot 0 again (10 loads), store of tile t (1), [wait slot 1] MFMAs, request
        // slot 1 again (10), store of tile t + step (1). Operations YOUNGER than the loads a wait is for:
        //   slot 0, first iteration: slot 1's request (10 | 0);          later: store, slot 1's request, store (12 | 2)
        //   slot 1, first iteration: slot 0's new request, store (11 | 1); later: store, request, store (12 | 2)
        const bool nx = t + step < n_tiles, first = t == t0;
#define BL_W0 "+v"(W0[0]), "+v"(W0[1]), "+v"(W0[2]), "+v"(W0[3]), "+v"(W0[4]), "+v"(W0[5]), "+v"(W0[6]), "+v"(W0[7]), "+v"(s0), "+v"(b0)
        {
            const int sel = (first ? 0 : 2) + (nx ? 1 : 0);    // first: 0 | 10, later: 2 | 12
            BL_WAIT4(sel, 0, 10, 2, 12, BL_W0);
        }
#undef BL_W0
        const bl_i32x16 a0 = consume(W0);
        unsigned sk0, bk0;   // (real moves: a C++ copy lets the allocator keep the OLD value in place and load the new one elsewhere)
        asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3" : "=&v"(sk0), "=&v"(bk0) : "v"(s0), "v"(b0));
        if (t + 2 * step < n_tiles) BL_REQ(W0, s0, b0, t + 2 * step)
        finish(a0, sk0, bk0, t);
        if (!nx) break;
        // tile t + step (slot 1): younger = slot 0's 10 loads (when requested) + the store of tile t
        const bool nx2 = t + 2 * step < n_tiles;
#define BL_W1 "+v"(W1[0]), "+v"(W1[1]), "+v"(W1[2]), "+v"(W1[3]), "+v"(W1[4]), "+v"(W1[5]), "+v"(W1[6]), "+v"(W1[7]), "+v"(s1), "+v"(b1)
        {
            const int sel = (first ? 0 : 2) + (nx2 ? 1 : 0);   // first: 1 | 11, later: 2 | 12
            BL_WAIT4(sel, 1, 11, 2, 12, BL_W1);
        }
#undef BL_W1
        const bl_i32x16 a1 = consume(W1);
        unsigned sk1, bk1;
        asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3" : "=&v"(sk1), "=&v"(bk1) : "v"(s1), "v"(b1));
        if (t + 3 * step < n_tiles) BL_REQ(W1, s1, b1, t + 3 * step)
        finish(a1, sk1, bk1, t + step);
    }
#undef BL_REQ
}

}  // namespace

// The fused o_proj launch (fq_block_linear_f16): FQ_LAUNCH_NO_KERNEL when the shape is not covered.
int fq_launch_block_linear(const f16* x, const f16* P, int64_t M, int R, int C, float sig_max, float sig_min, int rt_flags, const void* wimg,
                           const f16* scol, const f16* bias, int N, f16* y, int n_cu, hipStream_t stream) {
    if (R != BL_R || C != BL_C || M < 1 || M > BL_MAXM || N < 32 || (N & 31)) return FQ_LAUNCH_NO_KERNEL;
    // workgroups: one per CU (or one per tile when there are fewer tiles), trimmed so that they walk the same number of tiles where the count
    // allows (fq_launch_kron64_linear)
    const int tiles = N >> 5;
    int grid = n_cu < tiles ? n_cu : tiles;
    if (grid < 1) grid = 1;
    const int per = (tiles + grid - 1) / grid;
    grid = (tiles + per - 1) / per;
    const int lds = BL_PFRAG_BYTES + (int)M * BL_TOK_STRIDE + 2 * 32 * 33 * 4 + BL_MAXM * 4;   // <= 43.6 KB: under the default cap
    hipLaunchKernelGGL(fq_block_linear_kernel, dim3((unsigned)grid), dim3(BL_THREADS), lds, stream, x, P, (int)M, sig_max, sig_min, rt_flags,
                       reinterpret_cast<const uint4*>(wimg), scol, bias, N, y);
    return (int)hipGetLastError();
}
