// fq_gemm_i4_grouped.hip — grouped INT4 x INT4 -> INT32 GEMM: the Linear4bit of every expert of a mixture-of-experts layer as ONE
// launch, the consumer of fq_kron_quant_grouped_*'s packed rows.
//     c[r][n] = sum_k x[r][k] * w[g(r)][n][k],   g(r) = the group with group_offsets[g] <= r < group_offsets[g+1]
// x [rows, K/2] packed nibbles sorted by group, w [n_groups, N, K/2], group_offsets a DEVICE array that is never read on the host:
// no synchronisation, no launch per expert, capturable in a graph. An extension (the reference's DeepSeek path is fake-quant only);
// its contract is the loop of fq_int4_linear_f16 / fq_int4_gemm_i32 over the groups' row slices, bit for bit.
//
// The arithmetic and the inner loop are fq_gemm_i4.hip's int8 matrix path: nibble-in-high-half unpack (unpack16), v_mfma_i32_32x32x32_i8,
// LDS-DMA stages with the XOR swizzles, counted vmcnt, one barrier per K step, >> 8 at the end, the prow row permutation, the
// dequant16f<CLAMP> epilogue chosen by Kb > 10176 / 2. Integer sums and the same epilogue: the bits cannot depend on the tiling.
//
// What is new is the tile schedule.
//  * Grid. Group sizes exist only on the device, so the grid comes from a bound that needs no offsets: with a token tile of GBM rows
//    sum_g ceil(rows_g / GBM) <= rows / GBM + n_groups. Workgroups past the real tile count leave together, before the K loop.
//  * Locating a tile. Every workgroup forms the prefix sums of ceil(rows_g / GBM) itself: thread t loads the offsets of groups 2t and
//    2t + 1 (n_groups <= 1024 = 2 x 512 threads; n_groups + 1 distinct eight-byte words, L2-resident after the first workgroups), a wave
//    scan (six ds_bpermute steps), the eight wave totals through LDS, the prefix array (1025 ints) to LDS, then a ten-step binary
//    search that every lane runs on the same LDS words. The result goes through readfirstlane: group, row bounds and the operand
//    bases live in SGPRs. No preparatory launch, no workspace.
//  * Bounds. A tile's rows are its group's [begin + GBM * tile, end): DMA source rows past the group's end are clamped to the group's
//    last row (they never leave x, and they never read another expert's rows as if they were this one's), the epilogue stores only
//    rows inside the group. All row arithmetic is int64_t.
//
// GBM = 128 (the dense kernel's tile is 256 x 256), BN = 256, eight waves of 64 x 64.
//  * Expert groups are ragged: 131072 rows over 256 experts average 512 rows, a 2048-token step (16384 rows) averages 64, and under
//    Zipf routing most groups are smaller than their average. A 256-row tile would spend 3/4 of its MFMAs on padding at 64 rows; 128
//    spends half, and a smaller tile does not pay: such a launch is bound by streaming every expert's weights once (N K / 2 bytes per
//    non-empty group whatever the tile height), while each halving of GBM doubles the weight bytes the LDS-DMA moves per MFMA in the
//    large groups that hold most of the rows.
//  * LDS: three stages of (128 + 256) x 64 B = 72 KB, plus 4.1 KB for the prefix array: 76.2 KB, so TWO workgroups fit a CU's 160 KB;
//    eight waves at <= 128 VGPRs (__launch_bounds__(512, 2)) make that 4 waves per SIMD, the dense kernel's occupancy, with the
//    second workgroup's DMA and unpack VALU in the shadow of the first one's MFMAs — and a workgroup whose tile is mostly padding
//    shares its CU with one that is not.
//  * Order: xcd_tile (fq_gemm_common.hpp) over (real token tiles) x (feature tiles), the token-tile count taken from the scan. Workgroups
//    are dealt round-robin to the XCDs; each XCD walks a contiguous share of the sequence, eight feature tiles of one token tile, then
//    the next token tile. Token tiles are numbered group by group, so the workgroups resident on an XCD form a patch of a few
//    CONSECUTIVE token tiles x 8 feature tiles: neighbours share the row tile (x rows re-read from that XCD's L2), and the token
//    tiles of one group follow each other on the same XCD, so a group's weight tiles (7.3 MB at K = 7168, N = 2048: more than an
//    XCD's 4 MB L2 whole, 0.9 MB per feature tile) are re-read from L2 by the group's next token tile rather than from HBM.
//
// General shapes (K % 32 == 0 but K % 128 != 0, N % 16 != 0, K >= 2^17 up to 2^25): one thread per output element, unscaled products,
// the group by binary search in group_offsets. Correct, not fast: with it the entry points take exactly the dense ones' shapes.
// No hand-over protocol between workgroups anywhere: nothing here depends on memory-model details of one architecture.
#include "fq_gemm_common.hpp"
#include "fq_launch.hpp"

namespace {

using namespace fqgemm;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void lds_void_g;

constexpr int GBM = 128, BN = 256;           // output tile (tokens x output features)
constexpr int FQ_I8_K_LIMIT = 1 << 17;       // the first K the int8 path does not take (256 * 64 * K < 2^31)
constexpr int FQ_SIMPLE_K_LIMIT = 1 << 25;   // the first K no kernel of this file takes (64 * K < 2^31)
constexpr int FQ_MAX_GROUPS = 1024;
constexpr int BKB = 64;                      // packed bytes of K per stage and row (128 nibbles = 4 MFMA K-steps)
constexpr int STAGES = 3;
constexpr int TILE_BYTES = (BN + GBM) * BKB; // 24 KB: [W rows 0..255][X rows 0..127], 64 bytes each
constexpr int GW = 8, GT = GW * 64;          // waves, threads
constexpr int NWM = 2;                       // waves along the token dimension (4 along the feature dimension)
constexpr int TMT = GBM / 32 / NWM;          // 32-token tiles per wave (2: a wave owns 64 x 64)
constexpr int DPW = (BN + GBM) / 16 / GW;    // DMA instructions (16 rows x 64 B) per wave and stage: 3
static_assert(DPW * GW * 16 == BN + GBM && 2 * GT >= FQ_MAX_GROUPS, "tile / scan geometry");

__device__ __forceinline__ int swz_x(int r) { return (r >> 2) & 3; }
__device__ __forceinline__ int swz_w(int r) { return ((r >> 2) & 1) | (((r >> 4) & 1) << 1); }

struct GroupedArgs {
    const uint8_t* X;        // [rows, Kb]
    const uint8_t* W;        // [n_groups, N, Kb]
    const int64_t* offsets;  // [n_groups + 1], device
    int n_groups, N, Kb;
    GemmOut out;             // c / y [rows, N]; srow [rows]; scol, bias [n_groups, N]
};

__global__ __launch_bounds__(GT, 2) void fq_gemm_i4_grouped_kernel(GroupedArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[STAGES * TILE_BYTES];
    __shared__ int s_pre[FQ_MAX_GROUPS + 1];   // s_pre[g] = token tiles in front of group g (g > n_groups: the total)
    __shared__ int s_wave[GW];
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, c = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N, Kb = a.Kb, n_groups = a.n_groups;

    // ---- the schedule: prefix sums of ceil(rows_g / GBM), then this workgroup's (group, tile in group, feature tile)
    {
        const int g0 = 2 * tid;
        int64_t o0 = 0, o1 = 0, o2 = 0;
        if (g0 < n_groups) {
            o0 = a.offsets[g0];
            o1 = a.offsets[g0 + 1];
            o2 = g0 + 1 < n_groups ? a.offsets[g0 + 2] : o1;
        }
        const int c0 = (int)((o1 - o0 + GBM - 1) / GBM), c1 = (int)((o2 - o1 + GBM - 1) / GBM);
        int incl = c0 + c1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int excl = incl - (c0 + c1);
#pragma unroll
        for (int w = 0; w < GW; ++w)
            if (w < wave) excl += s_wave[w];
        s_pre[g0] = excl;
        s_pre[g0 + 1] = excl + c0;
        if (tid == GT - 1) s_pre[FQ_MAX_GROUPS] = excl + c0 + c1;
        __syncthreads();
    }
    const int tiles_m = __builtin_amdgcn_readfirstlane(s_pre[FQ_MAX_GROUPS]);
    int mb, nb;
    if (!xcd_tile(blockIdx.x, tiles_m, (N + BN - 1) / BN, mb, nb)) return;   // (workgroup-uniform: the whole workgroup leaves)
    int g;
    {
        int lo = 0, hi = n_groups;   // invariant: s_pre[lo] <= mb < s_pre[hi]; the LAST group with s_pre[g] <= mb: empty groups are skipped
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_pre[mid] <= mb) lo = mid;
            else hi = mid;
        }
        g = __builtin_amdgcn_readfirstlane(lo);
    }
    const int tile_in_g = __builtin_amdgcn_readfirstlane(mb - s_pre[g]);
    const int64_t m_end = fq_uniform_i64(a.offsets[g + 1]);
    const int64_t m0 = fq_uniform_i64(a.offsets[g]) + (int64_t)tile_in_g * GBM;   // < m_end: the tile exists
    const int n0 = nb * BN;
    const int nk = Kb / BKB;
    const uint8_t* __restrict__ X = a.X;
    const uint8_t* __restrict__ W = a.W + (int64_t)g * N * Kb;
    GemmOut out = a.out;
    out.scol += (int64_t)g * N;
    if (out.bias != nullptr) out.bias += (int64_t)g * N;

    // ---- DMA plan: a stage is 24 instructions of 1 KB (16 rows x 64 B); wave w issues instructions 3w .. 3w+2.
    // instruction i < 16 -> weight rows 16 i .., else token rows 16 (i - 16) .. ; lane l: row + (l >> 2), physical
    // 16-byte piece l & 3 holds logical piece (l & 3) ^ swz(row)
    const unsigned char* gsrc[DPW];
#pragma unroll
    for (int j = 0; j < DPW; ++j) {
        const int i = wave * DPW + j;
        const int r = (i < 16 ? i : i - 16) * 16 + (lane >> 2);  // row inside the weight / token part
        const int piece = (lane & 3) ^ (i < 16 ? swz_w(r) : swz_x(r));
        int64_t grow;
        const unsigned char* base;
        if (i < 16) {
            grow = n0 + r < N ? n0 + r : N - 1;
            base = W;
        } else {
            grow = m0 + r < m_end ? m0 + r : m_end - 1;   // the group's last row, never the next group's
            base = X;
        }
        gsrc[j] = base + grow * Kb + piece * 16;
    }
    const unsigned lds0 = (unsigned)(size_t)(lds_void_g*)smem;
    auto issue_stage = [&](int kb) {
        const unsigned dst = lds0 + (unsigned)((kb % STAGES) * TILE_BYTES) + (unsigned)(wave * DPW) * 1024u;
#pragma unroll
        for (int j = 0; j < DPW; ++j) {
            const unsigned char* src = gsrc[j] + (int64_t)kb * BKB;
            unsigned keep;
            asm volatile(
                "s_mov_b32 %0, m0\n\t"
                "s_mov_b32 m0, %2\n\t"
                "s_nop 0\n\t"
                "global_load_lds_dwordx4 %1, off\n\t"
                "s_mov_b32 m0, %0"
                : "=&s"(keep)
                : "v"(src), "s"(__builtin_amdgcn_readfirstlane((int)(dst + (unsigned)j * 1024u)))
                : "memory");
        }
    };

    // ---- fragment read offsets (bytes inside a stage): see fq_gemm_i4.hip
    int woff[2], xoff[TMT];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) woff[tn] = ((wave / NWM) * 64 + tn * 32 + prow(c)) * BKB;
#pragma unroll
    for (int tm = 0; tm < TMT; ++tm) xoff[tm] = BN * BKB + ((wave % NWM) * (TMT * 32) + tm * 32 + c) * BKB;
    const int wm = wave % NWM, wn = wave / NWM;
    const int wsw = swz_w(prow(c));
    const int xsw = swz_x(c);

    i32x16 acc[2][TMT];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int tm = 0; tm < TMT; ++tm) acc[tn][tm] = i32x16{0};

    uint4 r0w[2], r0x[TMT], r1w[2], r1x[TMT];
#define FQ_READ(ST, P, RW, RX)                                                                                      \
    {                                                                                                                \
        _Pragma("unroll") for (int tn = 0; tn < 2; ++tn) RW[tn] =                                                    \
            *reinterpret_cast<const uint4*>((ST) + woff[tn] + (((2 * (P) + h) ^ wsw) << 4));                         \
        _Pragma("unroll") for (int tm = 0; tm < TMT; ++tm) RX[tm] =                                                  \
            *reinterpret_cast<const uint4*>((ST) + xoff[tm] + (((2 * (P) + h) ^ xsw) << 4));                         \
    }
#define FQ_COMPUTE(RW, RX)                                                                                          \
    _Pragma("unroll") for (int half = 0; half < 2; ++half) {                                                         \
        i32x4 wf[2], xf[TMT];                                                                                        \
        _Pragma("unroll") for (int tn = 0; tn < 2; ++tn) wf[tn] =                                                    \
            unpack16(half ? make_uint2(RW[tn].z, RW[tn].w) : make_uint2(RW[tn].x, RW[tn].y));                        \
        _Pragma("unroll") for (int tm = 0; tm < TMT; ++tm) xf[tm] =                                                  \
            unpack16(half ? make_uint2(RX[tm].z, RX[tm].w) : make_uint2(RX[tm].x, RX[tm].y));                        \
        _Pragma("unroll") for (int tn = 0; tn < 2; ++tn) _Pragma("unroll") for (int tm = 0; tm < TMT; ++tm)          \
            acc[tn][tm] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[tn], xf[tm], acc[tn][tm], 0, 0, 0);               \
    }
#pragma unroll
    for (int p = 0; p < STAGES; ++p)
        if (p < nk) issue_stage(p);
    {   // stage 0 landed: up to STAGES - 1 younger stages of this wave in flight
        const int younger = nk - 1 < STAGES - 1 ? nk - 1 : STAGES - 1;
        if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(2 * DPW) : "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(DPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    FQ_READ(smem, 0, r0w, r0x)
    for (int kb = 0; kb < nk; ++kb) {
        const unsigned char* st = smem + (kb % STAGES) * TILE_BYTES;
        FQ_READ(st, 1, r1w, r1x)
        FQ_COMPUTE(r0w, r0x)
        if (kb + 1 < nk) {
            // stage kb+1 landed: the stage kb+2 of this wave may still be in flight
            const int younger = nk - 2 - kb < STAGES - 2 ? nk - 2 - kb : STAGES - 2;
            if (younger == 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" : : "n"(DPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();  // every wave holds all of stage kb in registers: its buffer is free
            if (kb + STAGES < nk) issue_stage(kb + STAGES);
            const unsigned char* sn = smem + ((kb + 1) % STAGES) * TILE_BYTES;
            FQ_READ(sn, 0, r0w, r0x)
        }
        FQ_COMPUTE(r1w, r1x)
    }
#undef FQ_READ
#undef FQ_COMPUTE

    // ---- epilogue: lane (h, c) of tile (tn, tm) holds n = n0 + wn*64 + tn*32 + 16 h + r (r = 0..15) of token
    //      m = m0 + wm*64 + tm*32 + c; products carry a factor 256. Rows past the group's end are not stored. ----
#pragma unroll
    for (int tm = 0; tm < TMT; ++tm) {
        const int64_t m = m0 + wm * (TMT * 32) + tm * 32 + c;
        if (m >= m_end) continue;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int nbase = n0 + wn * 64 + tn * 32 + 16 * h;
            if (nbase >= N) continue;  // N % 16 == 0 (checked by the launcher)
            int v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = acc[tn][tm][r] >> 8;
            if (out.c != nullptr) {
                int4* cp = reinterpret_cast<int4*>(out.c + m * N + nbase);
#pragma unroll
                for (int q = 0; q < 4; ++q) cp[q] = make_int4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
            }
            if (out.y != nullptr) {
                f16x8 o0, o1;
                f32x16 vf;
#pragma unroll
                for (int r = 0; r < 16; ++r) vf[r] = (float)v[r];
                const f16x8 s0 = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(out.scol + nbase));
                const f16x8 s1 = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(out.scol + nbase + 8));
                f16x8 b0 = {}, b1 = {};
                if (out.bias != nullptr) {
                    b0 = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(out.bias + nbase));
                    b1 = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(out.bias + nbase + 8));
                }
                if (Kb > 10176 / 2) dequant16f<true>(vf, out.srow[m], s0, s1, out.bias != nullptr, b0, b1, o0, o1);   // (|q| <= 64 K)
                else dequant16f<false>(vf, out.srow[m], s0, s1, out.bias != nullptr, b0, b1, o0, o1);
                uint4* yp = reinterpret_cast<uint4*>(out.y + m * N + nbase);
                yp[0] = __builtin_bit_cast(uint4, o0);
                yp[1] = __builtin_bit_cast(uint4, o1);
            }
        }
    }
}

// Any other shape fq_int4_gemm_i32 accepts: one thread per output element, products added UNSCALED (exact for K < FQ_SIMPLE_K_LIMIT),
// the row's group by binary search (the LAST group whose offset is <= the row: empty groups are skipped). Correct, not fast.
__global__ __launch_bounds__(256) void fq_gemm_i4_grouped_simple_kernel(GroupedArgs a, int64_t rows) {
    const int N = a.N, Kb = a.Kb;
    const int64_t total = rows * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / N;
        const int n = (int)(i - m * N);
        int lo = 0, hi = a.n_groups;   // invariant: offsets[lo] <= m < offsets[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.offsets[mid] <= m) lo = mid;
            else hi = mid;
        }
        const int64_t gn = (int64_t)lo * N + n;
        const uint32_t* xp = reinterpret_cast<const uint32_t*>(a.X + m * Kb);
        const uint32_t* wp = reinterpret_cast<const uint32_t*>(a.W + gn * Kb);
        int acc = 0;
        for (int k = 0; k < Kb / 4; ++k) {
            const uint32_t xv = xp[k], wv = wp[k];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc += (((int)(xv << (28 - 4 * e))) >> 28) * (((int)(wv << (28 - 4 * e))) >> 28);
        }
        if (a.out.c != nullptr) a.out.c[i] = acc;
        if (a.out.y != nullptr) {
            f16 v = dequant1(acc, a.out.srow[m], a.out.scol[gn]);
            if (a.out.bias != nullptr) v = v + a.out.bias[gn];
            a.out.y[i] = v;
        }
    }
}

}  // namespace

// FQ_LAUNCH_NO_KERNEL: a shape fq_launch_gemm_i4 refuses (K % 32, K >= 2^25, rows > 2^30), n_groups outside 1 .. 1024, or a grid beyond 2^31 - 1.
int fq_launch_gemm_i4_grouped(const uint8_t* X, const uint8_t* Wg, int64_t rows, int N, int K, const int64_t* group_offsets, int n_groups,
                              int32_t* c, f16* y, const f16* srow, const f16* scol_g, const f16* bias_g, hipStream_t stream) {
    if ((K & 31) || K < 32 || K >= FQ_SIMPLE_K_LIMIT || rows < 1 || N < 1 || rows > (1 << 30) || n_groups < 1 || n_groups > FQ_MAX_GROUPS)
        return FQ_LAUNCH_NO_KERNEL;
    GroupedArgs a;
    a.X = X;
    a.W = Wg;
    a.offsets = group_offsets;
    a.n_groups = n_groups;
    a.N = N;
    a.Kb = K / 2;
    a.out.c = c;
    a.out.y = y;
    a.out.srow = srow;
    a.out.scol = scol_g;
    a.out.bias = bias_g;
    if ((K & 127) || (N & 15) || K >= FQ_I8_K_LIMIT) {
        int64_t blocks = (rows * (int64_t)N + 255) / 256;
        if (blocks > 65536) blocks = 65536;
        hipLaunchKernelGGL(fq_gemm_i4_grouped_simple_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a, rows);
        return (int)hipGetLastError();
    }
    // sum_g ceil(rows_g / GBM) <= rows / GBM + n_groups: every group adds at most one partly filled tile. Rounded up to the XCD count (see xcd_tile).
    const int64_t tiles_m = rows / GBM + n_groups;
    const int64_t blocks = 8 * ((tiles_m * ((N + BN - 1) / BN) + 7) / 8);
    if (blocks > 0x7FFFFFFFll) return FQ_LAUNCH_NO_KERNEL;
    hipLaunchKernelGGL(fq_gemm_i4_grouped_kernel, dim3((unsigned)blocks), dim3(GT), 0, stream, a);
    return (int)hipGetLastError();
}
