// fq_kv_chunk_extend.hip — causal attention of a PROMPT-SIZED step over the paged KV cache (fq_kv_chunk_extend): the contract of
// fq_kv_batch_extend (fq_kvextend.hip) in the shape of the prompt launch (fq_prefill_attn.hip). FlashInfer covers the step with its append
// attention over a paged cache (include/flashinfer/prefill.cuh); the reference binds only the decode kernel.
//
// What it computes: request b has length L_b after the step's T rows were appended (kv_indptr / last_page_offset; precondition L_b >= T); query
// token t attends cached rows 0 .. L_b - T + t; query head h reads cache head (h / q_group) * copies. INT4 pages de-quantised as n * scale -
// zero, or fp16 pages; scores / sqrt(128); softmax and sums in fp32; o rounded to fp16 once; the optional q' = fp16(q . q_trans) inside the
// launch; the optional [batch, T, head_dim, H] output. head_dim 128, any page size >= 1 (rows are addressed through the page table one by
// one), q_group 1 / 2 / 4 / 8.
// Rows INSIDE 0 .. L_b - 1 are assumed finite, as in the prompt launch: a row above a token's diagonal gets the weight 0, but it still goes
// through the matrix pipe with the rest of its 64-row tile (0 . NaN). Rows at or beyond L_b — the unused tail of a last page, and on fp16
// pages whatever lies there — are never loaded: they enter LDS as zeros.
//
// Why: fq_kv_batch_extend is the merged decode launch with its 16 A rows filled. A workgroup there walks the whole cache for 16 (token, head)
// rows, so the nibble unpack is repeated per 16 rows and the launch is bound by it. Here a four-wave workgroup owns one set of cached rows (a KV
// head, or one copy of the replicated layout) and 128 A rows: 128 / q_group consecutive tokens x the q_group heads, token-major as there, a wave
// 32 of them with Q in registers. A 64-row tile is unpacked ONCE per 128 A rows into the swizzled fp16 image of the prompt launch (ds_read_b128
// row reads for K, ds_read_b64_tr_b16 transposed reads for V), both products run on v_mfma_f32_32x32x16_f16 and the softmax is lane-local, as
// there. Tiles start at cache row 0 of the request; two-deep LDS ring, register staging ahead of the arithmetic, one barrier per tile. With 256
// threads a thread stages one 16-byte load of K and one of V per INT4 tile (a quarter of a row), and one of each row's two (scale, zero) pairs.
// Grid: batch x row sets x ceil(T q_group / 128), late (long) blocks first. No split over rows, no workspace, no atomics.
//
// INT4 arithmetic: the nibbles stay exact and (scale, zero) act on the fp32 side, as in the decode and extend launches. K sits in LDS as n
// (0 .. 15), score = s_k (q . n) - z_k sum_f q_f with sum_f q_f formed once per A row in fp32 (after q_trans). V sits in LDS as n - 8 and
// o = sum_i a_i (n_i - 8) + sum_i p_i (8 s_i - z_i), a_i = fp16(256 p_i s_i) the one rounded quantity (the 256 keeps small weights out of the
// fp16 subnormals, as in fq_kvextend.hip); the second sum is a scalar per A row carried beside the softmax denominator.
// V rows with s >= 128 carry a power of two: they sit in LDS as (n - 8) 2^11 (|.| <= 16384) and their weight is fp16(256 p s 2^-11), exact both ways,
// so a dominant row of any fp16 scale stays finite (p = 1 at s = 4368: 546). The commit step's packed add is a packed fma that carries it; the scale reaches the row's four threads by one DPP move.
//
// Causality and ends: tiles wholly above a wave's last visible row are skipped, only tiles that touch a diagonal or L_b pay for the mask.
// Determinism: every sum of a token is formed tile by tile from row 0 in an order that depends on its absolute position, its head and the
// rows before it alone (a rescale by exp2(0) and the products of a masked row, p = 0, change no bit), so two launches are bit-identical and
// a step fed as two consecutive launches equals the one launch.
#include "fq_kv_common.hpp"
#include "fq_launch.hpp"

namespace {

using namespace fqkv;

constexpr int CX_HD = 128, CX_QB = 128, CX_KT = 64, CX_THREADS = 256;
constexpr int CX_TILE = CX_KT * CX_HD * 2;        // one K or V tile as fp16: 16 KB
constexpr int CX_PAR = 4 * CX_KT * 4;             // per tile: K scale', K zero', V scale', V zero' as fp32 [64] each
constexpr int CX_STAGE = 2 * CX_TILE + CX_PAR;
constexpr int CX_LDS = 2 * CX_STAGE;              // the two-deep ring: 66 KB, two workgroups per CU
constexpr float CX_PSCALE = 256.0f;               // weights enter the matrix pipe as fp16(256 p ..)

struct CxArgs {
    f16* o;                  // [batch, T, QH, HD] or [batch, T, HD, QH] (transpose_out)
    const f16* q;            // [batch, T, QH, HD]
    const f16* qt;           // [HD, HD] or nullptr
    const uint8_t* data;
    const uint32_t* param;   // half2 (scale, zero) per entry
    const int* indptr;
    const int* indices;
    const int* last_page_offset;
    int num_layers, layer_idx, num_heads, page_size, copies;
    int T, QH, gshift, NY, batch, nblk, transpose_out, pshift;
};

// byte offset of 16-byte chunk ch (0..15) of row `row` in a [rows][128 x fp16] image (fq_prefill_attn.hip's swizzle)
__device__ __forceinline__ int cx_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

typedef __fp16 cx_h4 __attribute__((__vector_size__(8)));
typedef __attribute__((address_space(3))) cx_h4 cx_lds_h4;
__device__ __forceinline__ f16x4 cx_tr(const unsigned char* p) {
    return __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((cx_lds_h4*)(p)));
}
__device__ __forceinline__ f16x8 cx_cat(f16x4 a, f16x4 b) { return f16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; }

// the eight nibbles of a dword (feature 2 j in the low half of byte j) as eight fp16 values n + off16 - 16 in FEATURE order: kv_unpack8 leaves
// 16 + n in the order 0 4 1 5 2 6 3 7, two byte permutes per pair put them back, one packed fma takes the 16 away (exact; mul: 1, or the power
// of two of a V row with a large scale)
__device__ __forceinline__ uint4 cx_unpack(uint32_t w, uint32_t ebits, f16x2 mul, f16x2 off) {
    uint32_t u[4];
    kv_unpack8(w, ebits, u);
    const uint32_t lo = 0x05040100u, hi = 0x07060302u;
    uint32_t n[4] = {__builtin_amdgcn_perm(u[1], u[0], lo), __builtin_amdgcn_perm(u[3], u[2], lo), __builtin_amdgcn_perm(u[1], u[0], hi),
                     __builtin_amdgcn_perm(u[3], u[2], hi)};
#pragma unroll
    for (int i = 0; i < 4; ++i) n[i] = __builtin_bit_cast(uint32_t, __builtin_elementwise_fma(__builtin_bit_cast(f16x2, n[i]), mul, off));
    return make_uint4(n[0], n[1], n[2], n[3]);
}

template <bool QT, bool F16>
__global__ __launch_bounds__(CX_THREADS, 2) void fq_kv_chunk_extend_kernel(CxArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char cx_smem[CX_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;                       // operand / accumulator lane: row or column r, half hh
    const int tg = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;   // transposed read: 16-lane group, the block row and 4-column piece this lane supplies
    // work item: (block of A rows — late blocks first, request, row set)
    const int per = a.batch * a.NY;
    const int blk = a.nblk - 1 - (int)blockIdx.x / per, rest = (int)blockIdx.x % per;
    const int y = rest % a.NY, b = rest / a.NY;
    const int G = 1 << a.gshift, R = a.T << a.gshift;              // A rows of this (request, row set): token-major (token, head) pairs
    const int pg0 = a.indptr[b], pg1 = a.indptr[b + 1];
    const int L = (pg1 - pg0 - 1) * a.page_size + a.last_page_offset[b];
    const int base = L - a.T;                                      // token t sees rows 0 .. base + t
    const int aw0 = CX_QB * blk + 32 * wave, arow = aw0 + r;        // this wave's first A row, this lane's
    const bool active = aw0 < R;                                   // (wave-uniform)
    const int ac = arow < R ? arow : R - 1;                        // (A rows past R: the last one's token, zero queries, never written)
    const int tok = ac >> a.gshift, h = y * G + (ac & (G - 1));
    const int qlim = base + tok;                                   // the last row this lane's query sees
    const int lim0 = base + ((aw0 < R ? aw0 : R - 1) >> a.gshift);  // ... the wave's first query, ... its last (wave-uniform)
    const int lim1 = base + ((aw0 + 31 < R ? aw0 + 31 : R - 1) >> a.gshift);

    // Q^T as the B operand: lane (r, hh) holds Q[A row r][16 ks + 8 hh ..+7] of K-step ks
    f16x8 qf[8];
    {
        const f16* qrow = a.q + (((size_t)b * a.T + tok) * a.QH + h) * CX_HD;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            uint4 w = make_uint4(0u, 0u, 0u, 0u);
            if (arow < R) w = *reinterpret_cast<const uint4*>(qrow + 16 * ks + 8 * hh);
            qf[ks] = __builtin_bit_cast(f16x8, w);
        }
    }
    if constexpr (QT) {
        // q'^T = T^T . q^T on the matrix pipe (fq_prefill_attn.hip): T in the swizzled image (first stage of the ring), its columns read
        // transposed as the A operand; the fp32 sums rounded to fp16 once, through a wave-private [32][128] image (second stage)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = tid + CX_THREADS * i, row = c >> 4, ch = c & 15;
            *reinterpret_cast<uint4*>(cx_smem + cx_off(row, ch)) = *reinterpret_cast<const uint4*>(a.qt + row * CX_HD + ch * 8);
        }
        __syncthreads();
        unsigned char* qs = cx_smem + CX_STAGE + wave * (32 * 256);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            f32x16 c = {0};
            const int c0 = 4 * nb + 2 * (tg & 1) + (tp >> 1);
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int row = 16 * ks + 8 * (tg >> 1) + tq;
                const f16x4 t0 = cx_tr(cx_smem + cx_off(row, c0) + 8 * (tp & 1));
                const f16x4 t1 = cx_tr(cx_smem + cx_off(row + 4, c0) + 8 * (tp & 1));
                c = mfma32(cx_cat(t0, t1), qf[ks], c);
            }
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {                       // registers 4 gg ..+3: columns 32 nb + 8 gg + 4 hh ..+3 of row r
                const f16x4 w = {(f16)c[4 * gg], (f16)c[4 * gg + 1], (f16)c[4 * gg + 2], (f16)c[4 * gg + 3]};
                *reinterpret_cast<f16x4*>(qs + r * 256 + 2 * (32 * nb + 8 * gg + 4 * hh)) = w;
            }
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const f16x8*>(qs + r * 256 + 2 * (16 * ks + 8 * hh));
        __syncthreads();                                           // the ring takes both images' place
    }
    float qsum = 0.0f;                                             // INT4: the sum over all features of this lane's query, fp32
    if constexpr (!F16) {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) qsum += (float)qf[ks][e];
        qsum += __shfl_xor(qsum, 32, 64);
    }

    const int tlast = ((CX_QB * blk + CX_QB - 1 < R ? CX_QB * blk + CX_QB - 1 : R - 1) >> a.gshift);
    const int kv_end = base + tlast + 1;                           // rows 0 .. kv_end - 1 are seen by some A row of the block (kv_end <= L)
    const int nt = kv_end > 0 ? (kv_end + CX_KT - 1) / CX_KT : 0;
    // LDS addresses: the swizzle's XOR commutes with the XOR of a compile-time chunk, so one lane base per kind of read serves every read of a tile
    // (K: cx_off(r, 2 ks + hh) = kl ^ 32 ks; V: cx_off(16 kk + rl, 4 db + c) + 8 (tp & 1) = 4096 kk + (vl ^ 64 db), row + 8: 2048 + (vl ^ 32 ^ 64 db);
    // commit: cx_off(sr, 4 sc + i) = cl ^ 16 i). Forty loop-invariant addresses held in registers spilled.
    const int kl = cx_off(r, hh), vl = cx_off(4 * (tg >> 1) + tq, 2 * (tg & 1) + (tp >> 1)) + 8 * (tp & 1), cl = cx_off(tid >> 2, 4 * (tid & 3));
    const float sm_scale = 1.44269504088896340736f / __builtin_sqrtf((float)CX_HD);   // exp2 takes pre-scaled scores

    // register staging of a tile: thread (sr, sc) -> quarter sc of cached row 64 t + sr of K and of V (INT4: 16 bytes each, fp16 pages: 64),
    // and with sc = 0 / 1 the row's K / V parameters. The row is found through the page table; rows at or beyond L are zeros, never loaded.
    constexpr int ROWB = F16 ? CX_HD * 2 : CX_HD / 2, NQ = F16 ? 4 : 1;
    const int sr = tid >> 2, sc = tid & 3;
    const size_t page_stride = (size_t)a.num_layers * 2 * a.num_heads * a.page_size;
    const size_t k_off = ((size_t)a.layer_idx * 2 * a.num_heads + (size_t)y * a.copies) * a.page_size, kv_off = (size_t)a.num_heads * a.page_size;
    uint4 kst[NQ], vst[NQ];
    uint32_t par = 0;
    bool live = false;
    auto request = [&](int t) {
        const int kv = CX_KT * t + sr;
        live = kv < L;
        par = 0;
#pragma unroll
        for (int i = 0; i < NQ; ++i) kst[i] = vst[i] = make_uint4(0u, 0u, 0u, 0u);
        if (live) {
            const int pit = a.pshift >= 0 ? kv >> a.pshift : kv / a.page_size, ent = kv - pit * a.page_size;
            const size_t e = (size_t)a.indices[pg0 + pit] * page_stride + k_off + (size_t)ent;
            const uint4* kp = reinterpret_cast<const uint4*>(a.data + e * ROWB + sc * (ROWB / 4));
            const uint4* vp = reinterpret_cast<const uint4*>(a.data + (e + kv_off) * ROWB + sc * (ROWB / 4));
#pragma unroll
            for (int i = 0; i < NQ; ++i) kst[i] = kp[i];
#pragma unroll
            for (int i = 0; i < NQ; ++i) vst[i] = vp[i];
            if constexpr (!F16) {
                if (sc < 2) par = a.param[e + (sc ? kv_off : 0)];
            }
        }
    };
    uint32_t ebits = 0x4C004C00u;   // (16.0, 16.0): kept in a VGPR (kv_unpack8)
    asm volatile("" : "+v"(ebits));
    auto commit = [&](int buf) {
        unsigned char* st = cx_smem + buf * CX_STAGE;
        if constexpr (F16) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int off = cl ^ (16 * i);
                *reinterpret_cast<uint4*>(st + off) = kst[i];
                *reinterpret_cast<uint4*>(st + CX_TILE + off) = vst[i];
            }
        } else {
            const uint32_t kw[4] = {kst[0].x, kst[0].y, kst[0].z, kst[0].w}, vw[4] = {vst[0].x, vst[0].y, vst[0].z, vst[0].w};
            // K as n; V as n - 8, or (n - 8) 2^11 where the row's scale (held by the row's thread sc = 1) is >= 128
            const uint32_t vpar = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)par, 0x55, 0xF, 0xF, false);   // quad_perm [1, 1, 1, 1]: one VALU move
            const bool big = (vpar & 0x7FFFu) >= 0x5800u && (vpar & 0x7FFFu) < 0x7C00u;
            const f16x2 one = {(f16)1.0f, (f16)1.0f}, koff = {(f16)-16.0f, (f16)-16.0f};
            const f16x2 vmul = big ? f16x2{(f16)2048.0f, (f16)2048.0f} : one, voff = big ? f16x2{(f16)-49152.0f, (f16)-49152.0f} : f16x2{(f16)-24.0f, (f16)-24.0f};
#pragma unroll
            for (int i = 0; i < 4; ++i) {                          // dword i: features 32 sc + 8 i ..+7 = chunk 4 sc + i
                const int off = cl ^ (16 * i);
                const uint4 z = make_uint4(0u, 0u, 0u, 0u);
                *reinterpret_cast<uint4*>(st + off) = live ? cx_unpack(kw[i], ebits, one, koff) : z;
                *reinterpret_cast<uint4*>(st + CX_TILE + off) = live ? cx_unpack(vw[i], ebits, vmul, voff) : z;
            }
            if (sc < 2) {                                          // (a dead row: par = 0, all four values 0)
                float* pp = reinterpret_cast<float*>(st + 2 * CX_TILE);
                const float s = (float)__builtin_bit_cast(f16, (unsigned short)(par & 0xFFFF)), z = (float)__builtin_bit_cast(f16, (unsigned short)(par >> 16));
                if (sc == 0) {
                    pp[sr] = s * sm_scale;
                    pp[CX_KT + sr] = z * sm_scale;
                } else {
                    pp[2 * CX_KT + sr] = s * (big ? CX_PSCALE * 0.00048828125f : CX_PSCALE);
                    pp[3 * CX_KT + sr] = 8.0f * s - z;
                }
            }
        }
    };

    float m = -INFINITY, l = 0.0f, zacc = 0.0f;                    // the row's running maximum (both lanes of the pair), THIS lane's part of its sums
    f32x16 oacc[4];                                                // O^T: feature 32 db + (reg & 3) + 8 (reg >> 2) + 4 hh of A row r
#pragma unroll
    for (int db = 0; db < 4; ++db) oacc[db] = f32x16{0};

    if (nt > 0) {
        request(0);
        commit(0);
    }
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        const unsigned char* kb = cx_smem + (t & 1) * CX_STAGE;
        const int klt = kl + (t & 1) * CX_STAGE, vlt = vl + (t & 1) * CX_STAGE + CX_TILE;
        const float* pp = reinterpret_cast<const float*>(kb + 2 * CX_TILE) + 4 * hh;
        if (t + 1 < nt) request(t + 1);
        if (active && CX_KT * t <= lim1) {                          // (wave-uniform: tiles wholly above the wave's last visible row are skipped)
            // S^T = K . Q^T: lane (r, hh) holds K row r (and 32 + r) as the A operand; s0 / s1[i] = score of A row r with cached row
            // 64 t + (i & 3) + 8 (i >> 2) + 4 hh (+ 32)
            f32x16 s0 = {0}, s1 = {0};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int off = klt ^ (32 * ks);
                const f16x8 k0 = *reinterpret_cast<const f16x8*>(cx_smem + off);
                const f16x8 k1 = *reinterpret_cast<const f16x8*>(cx_smem + off + 32 * 256);
                s0 = mfma32(k0, qf[ks], s0);
                s1 = mfma32(k1, qf[ks], s1);
            }
            float x[32];
            if constexpr (F16) {
#pragma unroll
                for (int i = 0; i < 16; ++i) x[i] = s0[i] * sm_scale, x[16 + i] = s1[i] * sm_scale;
            } else {
#pragma unroll
                for (int g4 = 0; g4 < 8; ++g4) {                   // registers 4 g4 ..+3: cached rows 32 (g4 >> 2) + 8 (g4 & 3) + 4 hh ..+3
                    const int row = 32 * (g4 >> 2) + 8 * (g4 & 3);
                    // (volatile reads, each group's results pinned: the sixteen parameter reads of a tile hoisted together hold 64 VGPRs — a spill)
                    const f32x4 ks4 = *reinterpret_cast<const volatile f32x4*>(pp + row), kz4 = *reinterpret_cast<const volatile f32x4*>(pp + CX_KT + row);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float c = g4 < 4 ? s0[4 * g4 + j] : s1[4 * (g4 - 4) + j];
                        x[4 * g4 + j] = __builtin_fmaf(ks4[j], c, -(kz4[j] * qsum));
                    }
                    asm volatile("" : "+v"(x[4 * g4]), "+v"(x[4 * g4 + 1]), "+v"(x[4 * g4 + 2]), "+v"(x[4 * g4 + 3]));
                }
            }
            if (CX_KT * t + CX_KT - 1 > lim0) {                    // (wave-uniform) the tile touches a diagonal (every row at or beyond L lies above all of them)
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const int kv = CX_KT * t + 32 * (i >> 4) + (i & 3) + 8 * ((i & 15) >> 2) + 4 * hh;
                    if (kv > qlim) x[i] = -INFINITY;
                }
            }
            // (tile 0 holds row 0, which every query sees: m is finite from the first tile on, a tile masked whole for a row leaves it alone)
            float mx = x[0];
#pragma unroll
            for (int i = 1; i < 32; ++i) mx = fmaxf(mx, x[i]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m, mx);
            if (__builtin_amdgcn_ballot_w64(m_new > m) != 0) {     // (wave-uniform; a factor of 1 would change nothing)
                const float alpha = __builtin_amdgcn_exp2f(m - m_new);
                l *= alpha;
                zacc *= alpha;
#pragma unroll
                for (int db = 0; db < 4; ++db) oacc[db] *= alpha;
                m = m_new;
            }
            float ps = 0.0f;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                x[i] = __builtin_amdgcn_exp2f(x[i] - m);
                ps += x[i];
            }
            l += ps;
            f16x8 pf[4];                                           // P^T as the B operand of K-step kk = 2 (sub-tile) + s: registers 8 s ..+7 of that sub-tile
            if constexpr (F16) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int e = 0; e < 8; ++e) pf[kk][e] = (f16)(x[8 * kk + e] * CX_PSCALE);
            } else {
#pragma unroll
                for (int g4 = 0; g4 < 8; ++g4) {
                    const int row = 32 * (g4 >> 2) + 8 * (g4 & 3);
                    const f32x4 vs4 = *reinterpret_cast<const volatile f32x4*>(pp + 2 * CX_KT + row), vz4 = *reinterpret_cast<const volatile f32x4*>(pp + 3 * CX_KT + row);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = 4 * g4 + j;
                        pf[i >> 3][i & 7] = (f16)(x[i] * vs4[j]);
                        zacc = __builtin_fmaf(x[i], vz4[j], zacc);
                    }
                    asm volatile("" : "+v"(zacc));
                }
            }
            // O^T += V^T . P^T: the A operand of K-step kk is V[rows 16 kk + 4 hh ..+3 and + 8][feature 32 db + r], two transposed reads
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const int o0 = vlt ^ (64 * db), o1 = vlt ^ (32 + 64 * db);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const f16x4 v0 = cx_tr(cx_smem + o0 + 4096 * kk);
                    const f16x4 v1 = cx_tr(cx_smem + o1 + 4096 * kk + 2048);
                    oacc[db] = mfma32(cx_cat(v0, v1), pf[kk], oacc[db]);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);                         // (the unpack stays behind the arithmetic: hoisted, its 32 dwords spill)
        if (t + 1 < nt) commit((t + 1) & 1);
        __syncthreads();
    }

    const float lt = l + __shfl_xor(l, 32, 64), zt = zacc + __shfl_xor(zacc, 32, 64);
    if (active && arow < R) {
        const float inv = lt > 0.0f ? 1.0f / lt : 0.0f;            // (an empty request: zeros)
        constexpr float back = 1.0f / CX_PSCALE;
        if (!a.transpose_out) {
            f16* orow = a.o + (((size_t)b * a.T + tok) * a.QH + h) * CX_HD;
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) {
                    f16x4 w;
#pragma unroll
                    for (int j = 0; j < 4; ++j) w[j] = (f16)((oacc[db][4 * gg + j] * back + zt) * inv);
                    *reinterpret_cast<f16x4*>(orow + 32 * db + 8 * gg + 4 * hh) = w;
                }
        } else {
            f16* ocol = a.o + ((size_t)b * a.T + tok) * CX_HD * a.QH + h;
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int f = 32 * db + 8 * (i >> 2) + 4 * hh + (i & 3);
                    ocol[(size_t)f * a.QH] = (f16)((oacc[db][i] * back + zt) * inv);
                }
        }
    }
}

}  // namespace

int fq_launch_kv_chunk_extend(const FqKvView& c, const FqKvAttn& at, int q_len, hipStream_t stream) {
    const int num_cache_heads = c.num_heads, q_group = at.share, copies = at.copies, page_size = c.page_size, head_dim = c.head_dim, batch = c.batch;
    const bool f16_cache = c.f16_pages;
    const f16* const qt = at.qt;
    if (head_dim != CX_HD || q_len < 1 || copies < 1 || q_group % copies || num_cache_heads % copies || page_size < 1 || batch < 1) return FQ_LAUNCH_NO_KERNEL;
    int gshift = 0;
    while (gshift < 4 && (1 << gshift) != q_group) ++gshift;
    if (gshift > 3) return FQ_LAUNCH_NO_KERNEL;                     // q_group 1 / 2 / 4 / 8
    const int NY = num_cache_heads / copies;
    const int64_t nblk = ((int64_t)q_len * q_group + CX_QB - 1) / CX_QB, wgs = (int64_t)batch * NY * nblk;
    if ((int64_t)q_len * q_group > 0x7FFFFFFF - CX_QB || wgs > 0x7FFFFFFF) return FQ_LAUNCH_NO_KERNEL;
    int pshift = -1;
    if ((page_size & (page_size - 1)) == 0) pshift = __builtin_ctz((unsigned)page_size);
    CxArgs a = {at.o, at.q, qt, (const uint8_t*)c.pages, (const uint32_t*)c.params, c.indptr, c.indices, c.last_page_offset, c.num_layers, c.layer_idx,
                num_cache_heads, page_size, copies, q_len, NY * q_group, gshift, NY, batch, (int)nblk, at.transpose_out, pshift};
    // (the ring is a static array: the compiler's resource report then states the kernel's LDS, and the launch needs no raised cap)
#define FQ_CX(QT_, F16_) hipLaunchKernelGGL((fq_kv_chunk_extend_kernel<QT_, F16_>), dim3((unsigned)wgs), dim3(CX_THREADS), 0, stream, a);
    if (qt != nullptr) {
        if (f16_cache) { FQ_CX(true, true) } else { FQ_CX(true, false) }
    } else {
        if (f16_cache) { FQ_CX(false, true) } else { FQ_CX(false, false) }
    }
#undef FQ_CX
    return (int)hipGetLastError();
}
