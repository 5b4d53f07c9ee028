// fq_kvextend.hip — causal attention of T NEW tokens per request over the paged KV cache (fq_kv_batch_extend): the step after the prompt
// that carries more than one token — a speculative verify of T draft tokens, a follow-up prompt that extends the cache, a prompt fed in
// pieces. FlashInfer covers it with its append / prefill attention over a paged cache (include/flashinfer/prefill.cuh); the reference
// binds only the decode kernel, so its cache class takes one token per request (kv_cache.py:150,344).
//
// What it computes: request b has length L_b after the step's rows were appended (kv_indptr / last_page_offset, as the decode reads it);
// its T new tokens sit at positions L_b - T .. L_b - 1 and query token t attends cached rows 0 .. L_b - T + t (causal, the mask aligned
// bottom-right as prefill.cuh's). Everything else is the decode launch's arithmetic (fq_kvcache.hip): k / v de-quantised as n * scale -
// zero (or fp16 rows), scores / sqrt(head_dim), fp32 throughout, fp16 out; the optional query transform q' = fp16(q . q_trans) inside the
// launch; the optional [.., head_dim, heads] output. Query head h reads cache head (h / q_group) * copies (the decode's conventions: the
// replicated layout read one copy, a cache that holds the KV heads once, plain multi-head attention).
//
// How: the merged decode launch (fq_kv_decode_kernel<.., QG = 4>) gives a workgroup to a (request, KV head) pair and runs q . k as
// v_mfma_f32_16x16x32_f16 with the query heads in the A rows — four distinct queries in sixteen rows. Here the A rows are (token, head)
// pairs of ONE set of cached rows: R = T * q_group rows, sixteen per tile (blockIdx.z; T * G > 16 adds tiles). A lane (part, slot) holds
// cached row `slot` and receives the scores of A rows 4 part .. 4 part + 3 for it: four DISTINCT rows where the decode had copies, for the
// same instructions. The rows are loaded and their nibbles unpacked once for all T tokens; p . v goes through the LDS transpose
// (ds_read_b64_tr_b16) as in the decode, now with all sixteen columns of the weight tile used. One softmax state per A row: its reference
// maximum is uniform over the 16 lanes that hold the row's weights (a four-step reduction when it moves, rare). The causal mask only
// touches rows >= L_b - T + 1: the steady-state loop stops there and stays free of conditions, the tail steps mask per A row.
// With few workgroups the rows of a request are split over several of them (SPLIT: the decode's relaxed-atomic + vmcnt hand-over).
// LIMIT (INT4 pages): a16 = fp16(256 p s_v) is finite while p s_v < 256. The reference sits 2^8 above the score that last moved it, so a
// dominant row alone has p = 2^-8; a row that arrives in a later step of the same wave within 8 log2 units above the reference's row has p up
// to 1 and overflows from p s_v >= 256 (tests/test_gpu_attn_closed_form.py: the marked riser cases). A wave-uniform slow path for rows with
// s_v >= 128 (values times 2^11, weight times 2^-11) was built and measured: 442 -> 506 us at 8 x 2048 rows, T = 512
// (profiles/attn_closed_form.txt); not kept.
#include "fq_kv_common.hpp"
#include "fq_launch.hpp"
#include <type_traits>

namespace {

using namespace fqkv;

struct ExtKv {
    uint8_t* data;
    const f16* param;        // half2 (scale, zero) per entry
    const int* indptr;
    const int* indices;
    const int* last_page_offset;
    int num_layers, layer_idx, num_heads, page_size, copies;
};

struct ExtArgs {
    f16* o;                  // [batch, T, QH, HD] or [batch, T, HD, QH] (transpose_out)
    const f16* q;            // [batch, T, QH, HD]
    const f16* qt;           // [HD, HD] or nullptr
    float* ws;               // SPLIT: counters [KX_WS_COUNTERS], then the states [workgroup][split][16][HD + 2]
    int T, QH, qgroup, ntiles, transpose_out;
};

constexpr int KX_HD = 128;
constexpr int KX_WS_COUNTERS = 128;   // a split launch has at most 128 workgroups per split (kv_extend_splits)
constexpr float KX_OFF = 16.0f;
// p . v of an INT4 row as sum_i a_i (n_i - KX_MID) + sum_i p_i (KX_MID s_i - z_i) with a_i = fp16(p_i s_i) the one rounded quantity: the MFMA
// sums a_i (16 + n_i), the zero-point sum takes a_i (16 + KX_MID) and p_i (z_i - KX_MID s_i). The rounding of a_i then multiplies n_i - 8
// (|.| <= 8) instead of n_i (<= 15): half the error of the decode's form where the zero point cancels most of the sum (flat scores, small V).
constexpr float KX_MID = 8.0f;
constexpr float KX_MARGIN = 8.0f;     // the decode's KV_MARGIN: a row's reference lies 2^8 above the largest score seen when it last moved

__device__ __forceinline__ float kx_max16(float v) {   // maximum over the 16 lanes of a row group (lane bits 0..3)
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float kx_sum16(float v) {
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int NW, bool UNI, bool F16, bool SPLIT>
__global__ __launch_bounds__(NW * 64, 2) void fq_kv_extend_kernel(ExtKv p, ExtArgs a) {
    constexpr int HD = KX_HD, RPW = 16, NS = NW * RPW, THREADS = NW * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char kx_smem[];
    const int b = blockIdx.x, y = blockIdx.y;
    const int S = SPLIT ? (int)gridDim.z / a.ntiles : 1;
    const int tile = SPLIT ? (int)blockIdx.z / S : (int)blockIdx.z, zs = SPLIT ? (int)blockIdx.z - tile * S : 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int part = lane >> 4, slot = lane & 15;
    const int R = a.T * a.qgroup;                  // A rows of this (request, row set): token-major (token, head) pairs
    const int chead = y * p.copies;                // = (h / qgroup) * copies for the qgroup query heads y * qgroup ..
    const float sm_scale = 1.44269504088896340736f / __builtin_sqrtf((float)HD);
    const int pg0 = p.indptr[b], pg1 = p.indptr[b + 1];
    const int64_t seq_len = (int64_t)(pg1 - pg0 - 1) * p.page_size + p.last_page_offset[b];
    auto arow = [&](int m) { const int r = tile * 16 + m; return r < R ? r : R - 1; };   // (rows past R repeat the last: finite, never written)

    // the tile's sixteen queries as fp16 values in LDS (fp32 words), transformed by qt where given: the decode's sums in the decode's order
    float* s_q = reinterpret_cast<float*>(kx_smem);                 // [16][HD]
    for (int i = tid; i < 16 * HD; i += THREADS) {
        const int m = i / HD, f = i - m * HD, r = arow(m), t = r / a.qgroup;
        s_q[i] = (float)a.q[(((size_t)b * a.T + t) * a.QH + (size_t)y * a.qgroup + (r - t * a.qgroup)) * HD + f];
    }
    __syncthreads();
    if (a.qt != nullptr) {
        constexpr int NCHQ = THREADS / HD, CHQ = HD / NCHQ;
        float* s_part = s_q + 16 * HD;                              // [NCHQ][16][HD]
        const int j = tid % HD, c = tid / HD;
        float acc[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) acc[m] = 0.0f;
        for (int i = c * CHQ; i < (c + 1) * CHQ; i += 4) {
            float t4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) t4[u] = (float)a.qt[(i + u) * HD + j];
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const float4 q4 = *reinterpret_cast<const float4*>(s_q + m * HD + i);   // (a wave's threads share c: one broadcast read)
                acc[m] = __builtin_fmaf(q4.x, t4[0], acc[m]);
                acc[m] = __builtin_fmaf(q4.y, t4[1], acc[m]);
                acc[m] = __builtin_fmaf(q4.z, t4[2], acc[m]);
                acc[m] = __builtin_fmaf(q4.w, t4[3], acc[m]);
            }
        }
#pragma unroll
        for (int m = 0; m < 16; ++m) s_part[(c * 16 + m) * HD + j] = acc[m];
        __syncthreads();
        for (int i = tid; i < 16 * HD; i += THREADS) {
            float t = 0.0f;
#pragma unroll
            for (int cc = 0; cc < NCHQ; ++cc) t += s_part[cc * 16 * HD + i];
            s_q[i] = (float)(f16)t;
        }
        __syncthreads();
    }
    // A operand of K-step w: lane (part, slot) carries A row `slot`, features 32 part + 8 w + feat(e) (INT4: the order kv_unpack8 leaves)
    auto feat = [](int e) { return F16 ? e : KV_PERM[e]; };
    f16x8 qa[4];
    float qsum[4], qoff[4];
    int tk[4];                                     // the token of A row 4 part + i: it sees rows up to L - T + tk
    {
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = s_q[slot * HD + part * 32 + w * 8 + feat(e)];
                qa[w][e] = (f16)v;
                t += v;
            }
        t += __shfl_xor(t, 16, 64);
        t += __shfl_xor(t, 32, 64);                // the sum over all features of A row `slot`
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            qsum[i] = __shfl(t, 4 * part + i, 64);
            qoff[i] = KX_OFF * qsum[i];
            tk[i] = arow(4 * part + i) / a.qgroup;
        }
    }
    uint32_t ebits = 0x4C004C00u;   // (16.0, 16.0): kept in a VGPR
    asm volatile("" : "+v"(ebits));

    float m[4], d[4], zacc[4];
    f32x4 oacc[8];                  // O[A row 4 part + i][feature of column `slot` of tile t]
#pragma unroll
    for (int i = 0; i < 4; ++i) m[i] = -INFINITY, d[i] = 0.0f, zacc[i] = 0.0f;
#pragma unroll
    for (int t = 0; t < 8; ++t) oacc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    typedef __fp16 h4 __attribute__((__vector_size__(8)));
    typedef __attribute__((address_space(3))) h4 lds_h4;
    __syncthreads();                                                    // s_q is read: the tiles take its place
    unsigned char* pv_vt = kx_smem + (size_t)wave * 4096;               // [8 tiles][16 rows][16 features] fp16
    unsigned char* pv_pt = kx_smem + (size_t)NW * 4096 + (size_t)wave * 512;   // [16 rows][16 A rows] fp16 weights

    const size_t page_stride = (size_t)p.num_layers * 2 * p.num_heads * p.page_size;
    const size_t k_off = ((size_t)p.layer_idx * 2 * p.num_heads + chead) * p.page_size, kv_off = (size_t)p.num_heads * p.page_size;
    // the decode's row walk (fq_kv_decode_kernel): UNI — a wave's 16 rows never straddle a page, one scalar page index per step; otherwise a
    // (page, entry) per lane, rows beyond the sequence read entry 0 of the last page
    const int vwave = SPLIT ? zs * NW + wave : wave;
    const int STRIDE = SPLIT ? S * NS : NS;
    int pit, ent;
    if (UNI) {
        pit = (vwave * RPW) / p.page_size;
        ent = vwave * RPW - pit * p.page_size;
    } else {
        pit = 0, ent = vwave * RPW + slot;
        while (ent >= p.page_size) {
            ent -= p.page_size;
            ++pit;
        }
    }
    struct Rows {
        uint4 kq[F16 ? 4 : 1], vq[F16 ? 4 : 1];
        uint32_t kpar, vpar;
    };
    constexpr int ROWB = F16 ? HD * 2 : HD / 2;
    const unsigned lane_row = (unsigned)slot * ROWB + (unsigned)part * (F16 ? 64 : 16);
    auto request = [&](int64_t base, Rows& r) {
        const uint8_t *kp_, *vp_;
        const uint32_t *kpar_, *vpar_;
        if (UNI) {
            const size_t page = (size_t)reinterpret_cast<kv_const_int*>(reinterpret_cast<uintptr_t>(p.indices))[pg0 + pit];
            const size_t e0 = kv_uniform64(page * page_stride + k_off + (size_t)ent);
            const uint8_t* kb = p.data + e0 * ROWB;
            kp_ = kb + lane_row;
            vp_ = kb + kv_off * ROWB + lane_row;
            kpar_ = reinterpret_cast<const uint32_t*>(p.param) + e0 + slot;
            vpar_ = kpar_ + kv_off;
        } else {
            const bool valid = base + slot < seq_len;
            const size_t page = (size_t)p.indices[valid ? pg0 + pit : pg1 - 1];
            const size_t ke = page * page_stride + k_off + (valid ? (size_t)ent : 0), ve = ke + kv_off;
            kp_ = p.data + ke * ROWB + part * (F16 ? 64 : 16);
            vp_ = p.data + ve * ROWB + part * (F16 ? 64 : 16);
            kpar_ = reinterpret_cast<const uint32_t*>(p.param) + ke;
            vpar_ = reinterpret_cast<const uint32_t*>(p.param) + ve;
        }
        ent += STRIDE;
        while (ent >= p.page_size) {
            ent -= p.page_size;
            ++pit;
        }
        if constexpr (F16) {
#pragma unroll
            for (int w = 0; w < 4; ++w) r.kq[w] = reinterpret_cast<const uint4*>(kp_)[w];
#pragma unroll
            for (int w = 0; w < 4; ++w) r.vq[w] = reinterpret_cast<const uint4*>(vp_)[w];
        } else {
            r.kq[0] = *reinterpret_cast<const uint4*>(kp_);
            r.vq[0] = *reinterpret_cast<const uint4*>(vp_);
            r.kpar = *kpar_;
            r.vpar = *vpar_;
        }
    };
    const int64_t first_masked = seq_len - a.T + 1;   // rows below it are seen by every token of the step
    // ALLV: every row of the step is seen by every A row (the steady-state loop); otherwise row `base + slot` is seen by A row i where
    // base + slot <= L - T + tk[i] (which also keeps every row at or beyond L out)
    auto step = [&](int64_t base, const Rows& r, auto allv) {
        constexpr bool ALLV = decltype(allv)::value;
        const int rel = ALLV ? 0 : (int)(base - (seq_len - a.T)) + slot;    // (tail only: a few strides around L - T)
        bool valid[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) valid[i] = ALLV || rel <= tk[i];
        const bool inseq = ALLV || rel < a.T;
        float x[4], vs = 1.0f, vz = 0.0f;
        f16x8 kb[4];
        if constexpr (F16) {
#pragma unroll
            for (int w = 0; w < 4; ++w) kb[w] = __builtin_bit_cast(f16x8, r.kq[w]);
        } else {
            const uint32_t kw[4] = {r.kq[0].x, r.kq[0].y, r.kq[0].z, r.kq[0].w};
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                uint32_t u[4];
                kv_unpack8(kw[w], ebits, u);
                kb[w] = __builtin_bit_cast(f16x8, u32x4{u[0], u[1], u[2], u[3]});
            }
        }
        const f32x4 c4 = kv_qk_mfma4(qa, kb);
        if constexpr (F16) {
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = valid[i] ? c4[i] * sm_scale : -INFINITY;
        } else {
            const float ks = (float)__builtin_bit_cast(f16, (unsigned short)(r.kpar & 0xFFFF)), kz = (float)__builtin_bit_cast(f16, (unsigned short)(r.kpar >> 16));
            vs = (float)__builtin_bit_cast(f16, (unsigned short)(r.vpar & 0xFFFF)), vz = (float)__builtin_bit_cast(f16, (unsigned short)(r.vpar >> 16));
            vz = __builtin_fmaf(-KX_MID, vs, vz);          // z - 8 s (see KX_MID)
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = valid[i] ? (ks * (c4[i] - qoff[i]) - kz * qsum[i]) * sm_scale : -INFINITY;
        }
        f16x4 ah;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (__builtin_amdgcn_ballot_w64(x[i] > m[i]) != 0) {     // (wave-uniform branch; the reference of A row 4 part + i is uniform over its 16 lanes)
                const float gm = kx_max16(x[i]);
                const bool up = gm > m[i];
                const float m_new = up ? gm + KX_MARGIN : m[i];
                const float alpha = up ? __builtin_amdgcn_exp2f(m[i] - m_new) : 1.0f;
                d[i] *= alpha;
                zacc[i] *= alpha;
#pragma unroll
                for (int t = 0; t < 8; ++t) oacc[t][i] *= alpha;
                m[i] = m_new;
            }
            const float pg = valid[i] ? __builtin_amdgcn_exp2f(x[i] - m[i]) : 0.0f;
            d[i] += pg;
            if constexpr (F16) {
                ah[i] = (f16)(pg * 256.0f);
            } else {
                const f16 a16 = (f16)((valid[i] ? pg * vs : 0.0f) * 256.0f);   // (a masked row's parameters may be anything: never multiplied)
                ah[i] = a16;
                zacc[i] += __builtin_fmaf((float)a16 * 0.00390625f, KX_OFF + KX_MID, valid[i] ? pg * vz : 0.0f);
            }
        }
        *reinterpret_cast<f16x4*>(pv_pt + slot * 32 + part * 8) = ah;      // row `slot`, A rows 4 part .. 4 part + 3
        if constexpr (F16) {
            // (a row beyond the sequence holds whatever the page holds, maybe NaN: it must not meet its zero weight in the MFMA)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint4 v = inseq ? r.vq[w] : make_uint4(0u, 0u, 0u, 0u);
                *reinterpret_cast<uint4*>(pv_vt + (2 * part + (w >> 1)) * 512 + slot * 32 + (w & 1) * 16) = v;
            }
        } else {
            const uint32_t vw[4] = {r.vq[0].x, r.vq[0].y, r.vq[0].z, r.vq[0].w};
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                uint32_t u[4];
                kv_unpack8(vw[w], ebits, u);
                *reinterpret_cast<u32x4*>(pv_vt + (2 * part + (w >> 1)) * 512 + slot * 32 + (w & 1) * 16) = u32x4{u[0], u[1], u[2], u[3]};
            }
        }
        const f16x4 pa = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4*)(pv_pt + 8 * lane)));
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const f16x4 vb = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4*)(pv_vt + t * 512 + 8 * lane)));
            oacc[t] = __builtin_amdgcn_mfma_f32_16x16x16f16(pa, vb, oacc[t], 0, 0, 0);
        }
    };
    // the decode's pipeline (one step of rows in flight under a step's arithmetic), its steady-state loop bounded by the first masked row
    // instead of the length; the tail (the last strides before the first masked row, the masked rows, the end of the sequence) is a loop
    // here: T new rows can span several strides
    Rows buf[2];
    int64_t base = (int64_t)vwave * RPW;
    if (base + (int64_t)2 * STRIDE < first_masked) {
        request(base, buf[0]);
        for (; base + (int64_t)2 * STRIDE < first_masked; base += (int64_t)2 * STRIDE) {
            request(base + STRIDE, buf[1]);
            step(base, buf[0], std::true_type{});
            request(base + (int64_t)2 * STRIDE, buf[0]);
            step(base + STRIDE, buf[1], std::true_type{});
        }
    } else if (base < seq_len) {
        request(base, buf[0]);
    }
    for (; base < seq_len; base += (int64_t)2 * STRIDE) {
        if (base + STRIDE < seq_len) request(base + STRIDE, buf[1]);
        step(base, buf[0], std::false_type{});
        if (base + STRIDE < seq_len) {
            if (base + (int64_t)2 * STRIDE < seq_len) request(base + (int64_t)2 * STRIDE, buf[0]);
            step(base + STRIDE, buf[1], std::false_type{});
        }
    }

    // the wave's state per A row: m (uniform over the row's 16 lanes), the denominators and zero-point sums of those lanes, O
    float dt[4], zt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        dt[i] = kx_sum16(d[i]);
        zt[i] = kx_sum16(zacc[i]);
    }
    __syncthreads();                                                    // every wave is done with its tiles
    float* st_m = reinterpret_cast<float*>(kx_smem);                   // [NW][16]
    float* st_d = st_m + NW * 16;                                       // [NW][16]
    float* st_o = st_d + NW * 16;                                       // [NW][16][HD]
    if (slot == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) st_m[wave * 16 + 4 * part + i] = m[i], st_d[wave * 16 + 4 * part + i] = dt[i];
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int f = 32 * (t >> 1) + 8 * (2 * (t & 1) + (slot >> 3)) + (F16 ? (slot & 7) : KV_PERM[slot & 7]);   // column `slot` of tile t
#pragma unroll
        for (int i = 0; i < 4; ++i) st_o[(wave * 16 + 4 * part + i) * HD + f] = oacc[t][i] * 0.00390625f - zt[i];
    }
    __syncthreads();
    auto out_index = [&](int r, int f) {           // A row r of the tile, feature f -> o
        const int rg = tile * 16 + r, t = rg / a.qgroup, h = y * a.qgroup + (rg - t * a.qgroup);
        return a.transpose_out ? (((size_t)b * a.T + t) * HD + f) * a.QH + h : (((size_t)b * a.T + t) * a.QH + h) * HD + f;
    };
    const int rows_here = R - tile * 16 < 16 ? R - tile * 16 : 16;
    const size_t wi = ((size_t)b * gridDim.y + y) * a.ntiles + tile;    // this (request, row set, tile): its counter, its states
    float* states = a.ws + KX_WS_COUNTERS;
    for (int idx = tid; idx < rows_here * HD; idx += THREADS) {
        const int r = idx / HD, f = idx - r * HD;
        float mm = st_m[r];
#pragma unroll
        for (int w = 1; w < NW; ++w) mm = fmaxf(mm, st_m[w * 16 + r]);
        float oo = 0.0f, dd = 0.0f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float mw = st_m[w * 16 + r];
            const float wt = mw == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(mw - mm);
            oo = __builtin_fmaf(st_o[(w * 16 + r) * HD + f], wt, oo);
            dd = __builtin_fmaf(st_d[w * 16 + r], wt, dd);
        }
        if constexpr (!SPLIT) {
            a.o[out_index(r, f)] = dd > 0.0f ? (f16)(oo / dd) : (f16)0.0f;
        } else {      // agent-scope stores: written through to memory for the last arriver (see the decode's hand-over)
            float* mine = states + ((wi * S + zs) * 16 + r) * (HD + 2);
            if (f == 0) {
                __hip_atomic_store(mine, mm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(mine + 1, dd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __hip_atomic_store(mine + 2 + f, oo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if constexpr (SPLIT) {
        // fq_kv_decode_kernel's hand-over: no release / acquire pair — gfx9 counts stores in vmcnt and the agent-scope stores write through to
        // the memory the merging workgroup's agent-scope loads read. A target where stores retire on another counter needs the fences back.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "fq_kv_extend_kernel<SPLIT>: the vmcnt-based hand-over is only valid on gfx942 / gfx950"
#endif
        unsigned* cnt = reinterpret_cast<unsigned*>(a.ws) + wi;
        __shared__ unsigned s_last;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this workgroup's states have reached memory ...
        __syncthreads();
        if (tid == 0) s_last = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(S - 1);   // ... before they are counted
        __syncthreads();
        if (s_last) {
            // the last arriver merges the S states of its rows: every row's weights once (thread (row, split)), then every output element's S partial
            // numerators, four elements per thread with all their loads in flight at once (one round trip per four elements, not per element)
            auto ld = [](const float* ptr) { return __hip_atomic_load(ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };   // (sc1: not this XCD's L2)
            float* s_w = st_o;                     // [16 rows][16 splits] (the workgroup's own states are merged: free)
            float* s_den = st_o + 256;             // [16 rows]
            if (tid < 256) {
                const int r = tid >> 4, z = tid & 15;
                const float* st = states + ((wi * S + (z < S ? z : 0)) * 16 + r) * (HD + 2);
                const float mz = z < S ? ld(st) : -INFINITY, dz = z < S ? ld(st + 1) : 0.0f;
                const float mm = kx_max16(mz);
                const float wt = mz == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(mz - mm);
                const float den = kx_sum16(dz * wt);
                s_w[tid] = wt;
                if (z == 0) s_den[r] = den;
            }
            __syncthreads();
            constexpr int ITEMS = 16 * HD / THREADS;          // 4: split launches run eight-wave workgroups only (see the launcher)
            static_assert(ITEMS == 4, "the split form is built for eight waves");
#pragma unroll
            for (int k0 = 0; k0 < ITEMS; k0 += 4) {
                float oz[4][16];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int idx = tid + (k0 + k) * THREADS, r = idx / HD, f = idx - r * HD;
#pragma unroll
                    for (int z = 0; z < 16; ++z) oz[k][z] = ld(states + ((wi * S + (z < S ? z : 0)) * 16 + r) * (HD + 2) + 2 + f);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int idx = tid + (k0 + k) * THREADS, r = idx / HD, f = idx - r * HD;
                    float oo = 0.0f;
#pragma unroll
                    for (int z = 0; z < 16; ++z) oo += oz[k][z] * s_w[r * 16 + z];     // (weight 0 beyond S and for empty splits)
                    const float dd = s_den[r];
                    if (r < rows_here) a.o[out_index(r, f)] = dd > 0.0f ? (f16)(oo / dd) : (f16)0.0f;
                }
            }
            if (tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch finds the counter as this one did
        }
    }
}

}  // namespace

// How many workgroups share a (request, row set, tile): the decode's rule (fq_kv_decode_splits: up to ~256 workgroups, at most 16 splits, none
// above 128 workgroups) with splits down to 128 rows — a workgroup here serves T * q_group rows of A, and one request of a Llama-3-8B model is
// only 8 of them: with 256-row splits a 2048-token request ran on 64 CUs (T = 4: 16.4 us against 8.4 for the 256-workgroup decode launch).
static int kv_extend_splits(int64_t wgs, int seq_hint) {
    if (wgs <= 0 || wgs > 128) return 1;
    int s = (int)(256 / wgs);
    if (s > 16) s = 16;
    if (seq_hint > 0 && s > seq_hint / 128) s = seq_hint / 128;
    return s < 2 ? 1 : s;
}

// A split launch has at most 128 workgroups per split and at most 256 (workgroup, split) states of 16 A rows (kv_extend_splits: 256 / workgroups
// splits, at most 16): one bound for every geometry of (batch, query heads, q_len) — 0 where no geometry of it can be split.
int64_t fq_kv_extend_ws_bytes(int batch, int num_q_heads, int q_len, int head_dim) {
    const int64_t min_wgs = (int64_t)batch * (((int64_t)q_len * num_q_heads + 15) / 16);   // (request, row set, tile) workgroups of the fewest tiles
    if (head_dim != KX_HD || min_wgs <= 0 || min_wgs > 128) return 0;
    return (int64_t)KX_WS_COUNTERS * (int64_t)sizeof(unsigned) + 256 * 16 * (int64_t)(head_dim + 2) * (int64_t)sizeof(float);
}

int fq_launch_kv_extend(const FqKvView& c, const FqKvAttn& at, int q_len, int seq_hint, int64_t ws_bytes, hipStream_t stream) {
    const int num_cache_heads = c.num_heads, q_group = at.share, copies = at.copies, page_size = c.page_size, head_dim = c.head_dim, batch = c.batch;
    const bool f16_cache = c.f16_pages;
    float* const ws = at.ws;
    if (head_dim != KX_HD || q_len < 1 || q_group < 1 || copies < 1 || q_group % copies || num_cache_heads % copies) return FQ_LAUNCH_NO_KERNEL;
    const int QH = num_cache_heads / copies * q_group, NY = num_cache_heads / copies;
    const int ntiles = (q_len * q_group + 15) / 16;
    const int64_t wgs = (int64_t)batch * NY * ntiles;
    const int64_t need = fq_kv_extend_ws_bytes(batch, QH, q_len, head_dim);
    const int splits = (ws != nullptr && need > 0 && ws_bytes >= need) ? kv_extend_splits(wgs, seq_hint) : 1;
    const bool split = splits > 1;
    // eight-wave workgroups up to two per CU (the decode's choice); beyond, four waves. A split launch has at most 256 workgroups
    // (kv_extend_splits): always eight waves, so the four-wave kernels are built unsplit only.
    const bool wide = wgs * splits <= 512;
    if (split && !wide) return FQ_LAUNCH_NO_KERNEL;
    ExtKv p = {(uint8_t*)c.pages, (const f16*)c.params, c.indptr, c.indices, c.last_page_offset, c.num_layers, c.layer_idx, num_cache_heads, page_size, copies};
    ExtArgs a = {at.o, at.q, at.qt, ws, q_len, QH, q_group, ntiles, at.transpose_out};
    const dim3 grid((unsigned)batch, (unsigned)NY, (unsigned)(ntiles * splits));
#define FQ_EXT4(NW_, UNI_, F16_, SP_)                                                                                  \
    {                                                                                                                 \
        constexpr size_t lds_q = sizeof(float) * 16 * KX_HD * (1 + NW_ * 64 / KX_HD), lds_pv = (size_t)NW_ * 4608;    \
        constexpr size_t lds_st = sizeof(float) * NW_ * 16 * (2 + KX_HD);                                            \
        constexpr size_t lds = lds_q > lds_pv ? (lds_q > lds_st ? lds_q : lds_st) : (lds_pv > lds_st ? lds_pv : lds_st); \
        FQ_RAISE_LDS_CAP((fq_kv_extend_kernel<NW_, UNI_, F16_, SP_>), lds);                                           \
        hipLaunchKernelGGL((fq_kv_extend_kernel<NW_, UNI_, F16_, SP_>), grid, dim3(NW_ * 64), lds, stream, p, a);     \
    }
#define FQ_EXT3(NW_, UNI_, F16_)                                                                                       \
    {                                                                                                                 \
        if constexpr (NW_ == 8) {                                                                                     \
            if (split) FQ_EXT4(NW_, UNI_, F16_, true) else FQ_EXT4(NW_, UNI_, F16_, false)                            \
        } else FQ_EXT4(NW_, UNI_, F16_, false)                                                                        \
    }
#define FQ_EXT2(NW_, UNI_)                                                                                             \
    {                                                                                                                 \
        if (f16_cache) FQ_EXT3(NW_, UNI_, true) else FQ_EXT3(NW_, UNI_, false)                                        \
    }
#define FQ_EXT(NW_)                                                                                                    \
    {                                                                                                                 \
        if (page_size % 16 == 0) FQ_EXT2(NW_, true) else FQ_EXT2(NW_, false)                                          \
    }
    if (wide) FQ_EXT(8) else FQ_EXT(4)
#undef FQ_EXT
#undef FQ_EXT2
#undef FQ_EXT3
#undef FQ_EXT4
    return (int)hipGetLastError();
}
