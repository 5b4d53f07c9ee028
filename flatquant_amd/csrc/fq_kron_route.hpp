// fq_kron_route.hpp — WHICH kernel runs a Kronecker transform + quantiser launch: the instantiation lists of every kernel family and the
// one function that picks from them (fq_kron_route, fq_kron_route.hip: pure host arithmetic on the launch's descriptors, no HIP call).
// The family files generate their launch switches from the same lists, so an instantiation is added HERE and nowhere else; the launchers
// (fq_launch.hpp) launch what they are handed and decide nothing.
#pragma once
#include "fq_common.hpp"

enum FqKronFamily { FQ_KF_K64, FQ_KF_WAVE, FQ_KF_TILES, FQ_KF_TRIO, FQ_KF_DUO, FQ_KF_TALL, FQ_KF_FAST, FQ_KF_GENERAL, FQ_KF_COUNT };

// The answer. rc = 0: `family` and the kernel's template arguments `t`, in declaration order (a bool as 0 / 1, the element type as
// 0 = f16, 1 = bf16); rc = FQ_LAUNCH_NO_KERNEL / FQ_LAUNCH_NEED_WS otherwise.
struct FqKronRoute {
    int rc, family;
    int t[11];
    int ws_skip;   // bytes of the workspace in front of the fragment image the kernel reads (64 x 64 on the second image of its workspace)
};

// What fq_kron_route is told beyond flags / rows / M / N (FqQuantOut carries n_clips, rt_flags, post_scale, ws_group_stride and the
// pointers whose PRESENCE matters: in2, y, fq[0], group_offsets).
//   flags: the compile-time flags, FQ_DT_BF16, FQ_IN_RMSNORM / FQ_IN_SILU_MUL, FQ_NO_WAVE_KERNEL; ws_bytes: 0 without a workspace;
//   try_k64: the caller is kron_dispatch (fq_capi.hip), whose 64 x 64 launches go to fq_kron64.hip first;
//   masked: bit f = family f is masked (measurement builds: fq_kron_measure_mask(); 0 in the product library).
FqKronRoute fq_kron_route(int flags, int64_t rows, int M, int N, bool diag, const FqQuantOut& out, int64_t ws_bytes, bool try_k64,
                          int masked = 0);
constexpr int FQ_K64_G128 = 0x10000;     // fq_kron64_kernel's internal template bits (not ABI flags): the FQ_GROUP128 instantiation,
constexpr int FQ_K64_GROUPED = 0x20000;  // the grouped-launch instantiations (fq_kron_quant_grouped_f16)
// The 64 x 64 kernel's FLAGS template argument for a launch, or -1 (fq_rmsnorm_kron_quant_f16 asks for it directly).
int fq_kron64_inst(int flags, int rt_flags, bool grouped);
// "fq_kron_tiles_kernel<3,4,128,3,6,0,f16,0>", the format of tools/kernel_resources.py; -> strlen, or -1 when `cap` is too small
int fq_kron_route_name(const FqKronRoute& r, char* buf, int cap);

constexpr int FQ_KF_NO_CTF = FQ_KF_COUNT;   // mask bit: no compile-time output set in the workgroup-per-token kernel
#ifdef FQ_MEASURE
static inline int fq_kron_measure_mask() {
    static const char* const env[] = {nullptr, "FQ_KRON_NO_WAVE", "FQ_KRON_NO_TILES", "FQ_KRON_NO_TRIO", "FQ_KRON_NO_DUO", "FQ_KRON_NO_TALL",
                                      nullptr, nullptr, "FQ_KRON_NO_CTF"};
    int m = 0;
    for (int f = 0; f <= FQ_KF_NO_CTF; ++f) m |= (env[f] && getenv(env[f])) << f;
    return m;
}
#else
static constexpr int fq_kron_measure_mask() { return 0; }
#endif

static inline int tiles32(int n) { return (n + 31) / 32; }
// dynamic LDS of the workgroup-per-token kernel (L image + padded token + packed stage) and of the general kernel with / without L in LDS
static inline size_t fq_kron_fast_lds(int MT, int KS1, int M, int N) {
    return (size_t)2 * MT * MT * 1024 + (size_t)MT * 32 * ((KS1 * 2) | 1) * 16 + (((size_t)M * N / 2 + 15) & ~(size_t)15) + 128;
}
static inline size_t fq_kron_general_lds(int MT, int waves, bool llds, int M, int N) {
    return (size_t)MT * 32 * ((((N + 15) / 16) * 2) | 1) * 16 + (((size_t)M * N / 2 + 15) & ~(size_t)15) + 2 * waves * sizeof(float) + 48 +
           (llds ? (size_t)2 * MT * MT * 1024 : 0);
}
constexpr size_t FQ_LDS_MAX = 160 * 1024;

// One persistent workgroup per CU, each taking `per_wg` tokens at a time: -> the grid, and the tokens per workgroup in *tpb.
static inline unsigned fq_persistent_grid(int64_t rows, int per_wg, int n_cu, int64_t* tpb) {
    int64_t blocks = (rows + per_wg - 1) / per_wg;
    if (blocks > n_cu) blocks = n_cu;
    if (blocks < 1) blocks = 1;
    *tpb = (rows + blocks - 1) / blocks;
    return (unsigned)blocks;
}

// ---- the instantiation lists (measurement knobs: -D on the compile line) ----
#ifndef WAVE_OS_MAXKS
#define WAVE_OS_MAXKS 5   // 16-bit outputs on the wave kernel up to N = 16 x this = 80 (measured, profiles/r04_wave_fakequant.txt: the wider pairs — 128 elements per lane, two waves per SIMD — are faster on the workgroup-per-token kernel: 64 x 128 fake-quant 145 vs 121 us)
#endif
// fq_kron_wave_kernel<MT, NT, KS1, W, RMS, T, OS>: X(MT, NT, KS1, W); per row: packed (f16, bf16, f16 with the RMSNorm) and, up to
// KS1 = WAVE_OS_MAXKS, fake-quant only / transform only (f16, bf16)
#define FQ_KRON_WAVE_LIST(X)                                                                                              \
    X(2, 4, 8, 7)   /* 64x128 */                                                                                         \
    X(2, 4, 7, 8)   /* 64x112 */                                                                                         \
    X(2, 3, 5, 12)  /* 64x80 (5120 = Qwen2.5-14B/32B hidden, in the reference's benchmark list: kernel_benchmark.py:234-246) */ \
    X(2, 2, 4, 16)  /* 56x64, (64x64 stays with fq_kron64.hip) */                                                        \
    X(1, 2, 4, 16)  /* 32x64 */

#ifndef TILES_G112   // measurement knobs (tools/variants.sh): groups of the 80 x 112 and 128 x 144 launches, streamed R at N = 144
#define TILES_G112 4   // (measured: 3 groups 113 us, 4 groups 107.5 us per 16384 tokens of 80 x 112; 121-127 VGPRs with four A fragments in flight)
#endif
#ifndef TILES_G144
#define TILES_G144 2
#endif
#ifndef TILES_RS144
#define TILES_RS144 false
#endif
#ifndef TILES_G64
#define TILES_G64 4   // (measurement knob) token groups of the 172 x 64 launch
#endif
// fq_kron_tiles_kernel<MT, NT, N, GROUPS, LKS, RS, T, H16 = false>, packed output: X(MT, NT, N, GROUPS, LKS, RS, F16), LKS = ceil(M / 16);
// every row on bf16, and on f16 where F16 says so (fp16 112 x 128 is fq_kron_trio.hip's, the same speed)
#define FQ_KRON_TILES_LIST(X)                                                                                             \
    X(3, 4, 112, TILES_G112, 5, false, 1) X(3, 4, 112, TILES_G112, 6, false, 1)   /* 80 x 112: four groups of four waves */ \
    X(4, 5, 144, TILES_G144, 7, TILES_RS144, 1) X(4, 5, 144, TILES_G144, 8, TILES_RS144, 1)   /* 128 x 144: two groups of five waves */ \
    X(5, 6, 192, 2, 9, true, 1)   /* 144 x 192: two groups of six waves, R streamed; 160 KB hold nine K-steps of L */     \
    X(4, 5, 148, 2, 7, false, 1) X(4, 5, 148, 2, 8, false, 1)   /* 128 x 148 (18944, Qwen2.5-7B ffn), even M: two groups of five waves, rows of 296 bytes */ \
    X(6, 6, 176, 1, 11, false, 1) X(6, 6, 176, 1, 12, false, 1)   /* 168 x 176 (29568, Qwen2.5-72B ffn): ONE group of six waves (two tokens + the L image would need 184 KB); the next token's DMA still runs under GEMM 2 and the quantiser */ \
    X(3, 4, 128, 3, 5, false, 1) X(3, 4, 128, 3, 6, false, 1)   /* 86 x 128 (11008, Llama-2-7B ffn): 123 us where fq_kron_trio.hip's MT = 3 build took 145 */ \
    X(4, 4, 128, 3, 7, false, 0) X(4, 4, 128, 3, 8, false, 0)   /* bf16 112 x 128: three groups of four waves */
// ... at N = 64 (the TALL pairs — Hadamard rotations as a Kronecker launch — on two-wave token groups), f16: X(MT, LKS, GROUPS), each with
// H16 = false (packed, fp32 quantiser) and true (the fp16 Quantizer arithmetic: packed and / or the rounded transform). Four groups of two
// waves where 4 tokens + the L image fit 160 KB (a token: 2 LKS KB, the image: LKS x MT KB); 172 x 64 = 88 + 66 KB
#define FQ_KRON_TILES64_LIST(X) X(3, 5, 4) X(3, 6, 4) X(4, 7, 4) X(4, 8, 4) X(5, 9, 4) X(5, 10, 4) X(6, 11, TILES_G64) X(6, 12, 3)

// fq_kron_trio_kernel<MT, H16, TAIL> (N = 128, f16): X(MT, H16), each with TAIL = (M % 4 != 0). Packed launches of M <= 96 run the
// tiles kernel, so MT = 3 exists for the fp16 Quantizer arithmetic only.
#define FQ_KRON_TRIO_LIST(X) X(4, false) X(4, true) X(3, true)

// fq_kron_tall_kernel<MT, H16, YOUT> (N = 64, f16): what the tiles kernel's N = 64 rows leave — the fp32 quantiser WITH the transform
// (a test-only set) and the rotation alone at six row tiles (measured, profiles/r05_tall_on_tiles.txt: 172 x 64 180 us there, 171 here)
#define FQ_KRON_TALL_LIST(X) X(3, false, true) X(4, false, true) X(5, false, true) X(6, false, true) X(6, true, true)

#ifndef FQ_GEN_OCC2
#define FQ_GEN_OCC2 2   // MT = 2 shapes (measurement knobs): workgroups per CU, waves per workgroup
#endif
#ifndef FQ_GEN_W2
#define FQ_GEN_W2 4
#endif
#ifndef FQ_FS_DECODE_W
#define FQ_FS_DECODE_W 8   // (measurement knob) waves of the decode-sized 112 x 128 SiLU.mul launch; 4 = the prefill build at every size
#endif
// fq_kron_fast_kernel<MT, NT, KS1, WAVES, OCC, SILU, CTF, NV, T, GM, G128>, the workgroup-per-token kernel: X(MT, NT, KS1, WAVES, OCC, BF16).
// Every row: all output sets (CTF = -1) on f16, and on bf16 where BF16 says so; MT >= 3 on f16 also CTF = packed and packed | fp16 quantiser.
#define FQ_KRON_FAST_LIST(X)                                                                                              \
    X(2, 4, 8, FQ_GEN_W2, FQ_GEN_OCC2, 1) X(4, 4, 8, 4, 2, 1) X(3, 4, 8, 4, 2, 1) X(4, 7, 14, 8, 1, 1) X(2, 4, 7, FQ_GEN_W2, FQ_GEN_OCC2, 1)  \
    X(4, 8, 16, 8, 1, 0)   /* 112 x 256: the Hadamard rotation of 28672 = (28 x 4) x 256 as a Kronecker product */           \
    X(1, 2, 4, 4, 4, 1) X(2, 2, 4, 4, FQ_GEN_OCC2, 1) X(2, 3, 5, 4, FQ_GEN_OCC2, 1)                                                \
    X(4, 5, 9, 8, 1, 1)    /* 128 x 144 = 18432 (DeepSeek-V3 dense ffn), and every 96 < M <= 128 with N = 144 */             \
    X(3, 4, 7, 4, 2, 1)    /* 80 x 112 = 8960 (Qwen2.5-1.5B ffn) */                                                          \
    X(1, 2, 3, 4, 4, 1)    /* 32 x 48 = 1536 (Qwen2.5-1.5B hidden) */                                                        \
    X(5, 6, 12, 8, 1, 1)   /* 144 x 192 = 27648 (Qwen2.5-32B ffn) */                                                         \
    X(6, 6, 11, 8, 1, 1)   /* 168 x 176 = 29568 (Qwen2.5-72B ffn) */
// ... with x_up * silu(x_gate) formed while the token is staged (SILU, f16, the down_proj shapes): CTF = -1, packed, packed | fp16 quantiser;
// and the decode form of 112 x 128 packed (rows <= 64: FQ_FS_DECODE_W waves, one workgroup per CU)
#define FQ_KRON_FAST_SILU_LIST(X) X(4, 4, 8, 4, 2) X(3, 4, 8, 4, 2) X(4, 7, 14, 8, 1) X(4, 8, 16, 8, 1)
// ... with the group-128 epilogue (G128, CTF = -1, f16 and bf16): DeepSeek-V3's 64 x 112 hidden and 32 x 64 moe_inter; the N = 64, 80, 128 pairs
#define FQ_KRON_FAST_G128_LIST(X) X(1, 2, 4, 4, 4) X(2, 2, 4, 4, 2) X(2, 4, 7, 4, 2) X(2, 4, 8, 4, 2) X(2, 3, 5, 4, 2) X(3, 4, 8, 4, 2) X(4, 4, 8, 4, 2)
