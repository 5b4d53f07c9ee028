// fq_prefill_attn.hip — causal self-attention of a PROMPT (fq_prefill_attention_f16): the one launch of a prefill layer the library did not
// own. The reference hands the un-quantised (transformed) states its cache returns on the first call per layer to flash-attn's CUDA kernel
// (deploy/transformers/modeling_llama.py:125-137, transformers' _flash_attention_forward(.., is_causal=True)), after query_states @
// trans_matrix_k_inv_t. fq_kv_batch_extend cannot stand in: it reads the QUANTISED cache and has the decode launch's shape.
//
// What it computes: q, o [batch, seq, q_heads, 128], k, v [batch, seq, kv_heads, 128] fp16; query head h reads KV head h / (q_heads /
// kv_heads) (repeat_kv's order); position t of a request attends positions 0 .. t of it; scores q . k / sqrt(128), softmax and sums in fp32,
// o rounded to fp16 once. Optional q_trans: q' = fp16(q . q_trans) inside the launch (fp32 sums, one rounding). Optional per-request range
// (seq_start, seq_len): the request's tokens are positions start .. start + len - 1, everything is relative to start, positions outside the
// range are written as zeros and never read in a way that changes a result (their K / V rows are replaced by zeros on the way into LDS, their
// Q rows too). One launch, no workspace, no atomics; the order of every sum depends on (relative position, head) alone, so two runs are
// bit-identical and a ranged request equals the same tokens launched alone.
// Inputs INSIDE a range are assumed finite: a key above the diagonal gets the weight 0, but its V row still goes through the matrix pipe with
// the rest of its 64-row tile, so a NaN / Inf in V (or K) at a later position of the range reaches the earlier rows that share the tile (0 . NaN).
//
// How (the flash-style forward of the CDNA guides, in plain HIP): a workgroup of four waves owns a block of 128 query rows of one (request,
// query head), a wave 32 of them with its Q fragments in registers. K / V tiles of 64 rows go through LDS by register staging (requested
// before a tile's arithmetic, written behind it into the other half of a two-deep ring: one barrier per tile), both in the XOR-swizzled
// 256-byte-row image that serves ds_read_b128 row reads (K) and ds_read_b64_tr_b16 transposed reads (V). The SWAPPED product S^T = K . Q^T
// (v_mfma_f32_32x32x16_f16, K the A operand) leaves a query row's scores on one lane pair: the row maximum is 31 fmax and one exchange with
// lane ^ 32, the row sum stays per lane until the end. The accumulator tile S^T is the B operand of O^T += V^T . P^T as it stands — registers
// 8 s .. 8 s + 7 rounded to fp16 are the fragment of K-step s, in the permuted row order 16 s + 8 (j >> 2) + 4 h + (j & 3) that the V reads
// follow — so no lane exchange and no LDS round trip for P, and O^T keeps the query row on the lane: every softmax rescale is lane-local.
// Causal: tiles wholly above a wave's diagonal are skipped, only tiles that touch the diagonal (or the end of the range) pay for the mask,
// late (long) blocks are scheduled first, and where the unit count allows it the q_group heads of a KV head run back to back on one XCD
// (workgroup ids are dealt round-robin over the 8 XCDs): the expectation, not measured, is that their K / V tiles then meet in that XCD's L2.
#include "fq_kv_common.hpp"
#include "fq_launch.hpp"

namespace {

using namespace fqkv;

constexpr int PA_HD = 128, PA_QB = 128, PA_KT = 64, PA_THREADS = 256;
constexpr int PA_TILE = PA_KT * PA_HD * 2;        // one K or V tile: 16 KB
constexpr int PA_STAGE = 2 * PA_TILE;             // K + V
constexpr int PA_LDS = 2 * PA_STAGE;              // the two-deep ring: 64 KB, two workgroups per CU

struct PaArgs {
    f16* o;
    const f16* q;
    const f16* qt;           // [128, 128] or nullptr
    const f16* k;
    const f16* v;
    const int* seq_start;    // [batch] or nullptr (with seq_len)
    const int* seq_len;
    int batch, seq, QH, KVH, nblk, swz;
};

// byte offset of 16-byte chunk ch (0..15) of row `row` in a [rows][128 x fp16] image: the XOR keeps both the row reads of a 32x32x16 operand
// and its transposed reads off each other's banks
__device__ __forceinline__ int pa_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

typedef __fp16 pa_h4 __attribute__((__vector_size__(8)));
typedef __attribute__((address_space(3))) pa_h4 pa_lds_h4;
__device__ __forceinline__ f16x4 pa_tr(const unsigned char* p) {
    return __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((pa_lds_h4*)(p)));
}
__device__ __forceinline__ f16x8 pa_cat(f16x4 a, f16x4 b) { return f16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; }

template <bool QT>
__global__ __launch_bounds__(PA_THREADS, 2) void fq_prefill_attn_kernel(PaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pa_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;                       // operand / accumulator lane: row or column r, half hh
    const int tg = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;   // transposed read: 16-lane group, the block row and 4-column piece this lane supplies
    const int G = a.QH / a.KVH;
    // work item: (block of query rows — late blocks first, request, KV head, head of the group)
    int u, hg;
    {
        const int x = blockIdx.x;
        if (a.swz) {         // the G heads of a unit back to back on XCD x % 8
            const int t = x >> 3;
            hg = t % G;
            u = (t / G) * 8 + (x & 7);
        } else {
            u = x / G;
            hg = x - u * G;
        }
    }
    const int kvh = u % a.KVH, ub = u / a.KVH;
    const int b = ub % a.batch, blk = a.nblk - 1 - ub / a.batch;
    const int h = kvh * G + hg;
    int start = 0, len = a.seq;
    if (a.seq_start != nullptr) {
        start = a.seq_start[b];
        len = a.seq_len[b];
        start = start < 0 ? 0 : (start > a.seq ? a.seq : start);       // (a range never leaves the tensors)
        len = len < 0 ? 0 : (len > a.seq - start ? a.seq - start : len);
    }
    const size_t tok0 = (size_t)b * a.seq;
    // positions outside the range are zeros: this workgroup writes those among the ABSOLUTE positions 128 blk .. 128 blk + 127 of its head
    if (len < a.seq) {
        for (int i = tid; i < PA_QB * 16; i += PA_THREADS) {
            const int p = PA_QB * blk + (i >> 4);
            if (p < a.seq && (p < start || p >= start + len))
                *reinterpret_cast<uint4*>(a.o + ((tok0 + p) * a.QH + h) * PA_HD + (i & 15) * 8) = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    const int q0 = PA_QB * blk;                                    // everything below is relative to `start`
    if (q0 >= len) return;
    const size_t qstride = (size_t)a.QH * PA_HD, kstride = (size_t)a.KVH * PA_HD;
    const f16* qbase = a.q + (tok0 + start) * qstride + (size_t)h * PA_HD;
    const f16* kbase = a.k + (tok0 + start) * kstride + (size_t)kvh * PA_HD;
    const f16* vbase = a.v + (tok0 + start) * kstride + (size_t)kvh * PA_HD;
    f16* obase = a.o + (tok0 + start) * qstride + (size_t)h * PA_HD;

    const int qw0 = q0 + 32 * wave, qrel = qw0 + r;                // this wave's first row, this lane's row
    const bool active = qw0 < len;                                 // (wave-uniform)
    // Q^T as the B operand: lane (r, hh) holds Q[row r][16 ks + 8 hh ..+7] of K-step ks (rows beyond the range: zeros)
    f16x8 qf[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (qrel < len) w = *reinterpret_cast<const uint4*>(qbase + (size_t)qrel * qstride + 16 * ks + 8 * hh);
        qf[ks] = __builtin_bit_cast(f16x8, w);
    }
    if constexpr (QT) {
        // q'^T = T^T . q^T on the matrix pipe: T in the swizzled image (first half of the ring), its columns read transposed as the A operand;
        // the fp32 sums rounded to fp16 once, passed through a wave-private [32][128] image (second half) into the B-operand order
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = tid + PA_THREADS * i, row = c >> 4, ch = c & 15;
            *reinterpret_cast<uint4*>(pa_smem + pa_off(row, ch)) = *reinterpret_cast<const uint4*>(a.qt + row * PA_HD + ch * 8);
        }
        __syncthreads();
        unsigned char* qs = pa_smem + PA_STAGE + wave * (32 * 256);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            f32x16 c = {0};
            const int c0 = 4 * nb + 2 * (tg & 1) + (tp >> 1);
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int row = 16 * ks + 8 * (tg >> 1) + tq;
                const f16x4 t0 = pa_tr(pa_smem + pa_off(row, c0) + 8 * (tp & 1));
                const f16x4 t1 = pa_tr(pa_smem + pa_off(row + 4, c0) + 8 * (tp & 1));
                c = mfma32(pa_cat(t0, t1), qf[ks], c);
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

    const int kv_end = q0 + PA_QB < len ? q0 + PA_QB : len;        // rows 0 .. kv_end - 1 are seen by some row of the block
    const int nt = (kv_end + PA_KT - 1) / PA_KT;
    // register staging of a tile: thread -> four 16-byte chunks of K and of V (a 16-lane group reads one whole 256-byte row); rows at or
    // beyond the range's end are zeros (never loaded: they may lie outside the tensors, and 0 . NaN would reach O through the matrix pipe)
    uint4 kst[4], vst[4];
    auto request = [&](int t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + PA_THREADS * i, kv = PA_KT * t + (c >> 4), ch = c & 15;
            kst[i] = vst[i] = make_uint4(0u, 0u, 0u, 0u);
            if (kv < len) {
                kst[i] = *reinterpret_cast<const uint4*>(kbase + (size_t)kv * kstride + ch * 8);
                vst[i] = *reinterpret_cast<const uint4*>(vbase + (size_t)kv * kstride + ch * 8);
            }
        }
    };
    auto commit = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + PA_THREADS * i, off = pa_off(c >> 4, c & 15);
            *reinterpret_cast<uint4*>(pa_smem + buf * PA_STAGE + off) = kst[i];
            *reinterpret_cast<uint4*>(pa_smem + buf * PA_STAGE + PA_TILE + off) = vst[i];
        }
    };

    const float sm_scale = 1.44269504088896340736f / __builtin_sqrtf((float)PA_HD);   // exp2 takes pre-scaled scores
    float m = -INFINITY, l = 0.0f;                                 // the row's running maximum (both lanes of the pair), THIS lane's part of its sum
    f32x16 oacc[4];                                                // O^T: feature 32 db + (reg & 3) + 8 (reg >> 2) + 4 hh of row r
#pragma unroll
    for (int db = 0; db < 4; ++db) oacc[db] = f32x16{0};

    request(0);
    commit(0);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        const unsigned char* kb = pa_smem + (t & 1) * PA_STAGE;
        const unsigned char* vb = kb + PA_TILE;
        if (t + 1 < nt) request(t + 1);
        if (active && PA_KT * t <= qw0 + 31) {                      // (wave-uniform: tiles wholly above the wave's diagonal are skipped)
            // S^T = K . Q^T: lane (r, hh) holds K row r (and 32 + r) as the A operand; s0 / s1[i] = score of query row r with K row
            // 64 t + (i & 3) + 8 (i >> 2) + 4 hh (+ 32)
            f32x16 s0 = {0}, s1 = {0};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int off = pa_off(r, 2 * ks + hh);
                const f16x8 k0 = *reinterpret_cast<const f16x8*>(kb + off);
                const f16x8 k1 = *reinterpret_cast<const f16x8*>(kb + off + 32 * 256);
                s0 = mfma32(k0, qf[ks], s0);
                s1 = mfma32(k1, qf[ks], s1);
            }
            float x[32];
#pragma unroll
            for (int i = 0; i < 16; ++i) x[i] = s0[i] * sm_scale, x[16 + i] = s1[i] * sm_scale;
            if (PA_KT * t + PA_KT - 1 > qw0 || PA_KT * t + PA_KT > len) {   // (wave-uniform) the tile touches the diagonal or the range's end
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const int kv = PA_KT * t + 32 * (i >> 4) + (i & 3) + 8 * ((i & 15) >> 2) + 4 * hh;
                    if (kv > qrel || kv >= len) x[i] = -INFINITY;
                }
            }
            // (tile 0 holds row 0, which every query row sees: m is finite from the first tile on, a tile masked whole for a row leaves it alone)
            float mx = x[0];
#pragma unroll
            for (int i = 1; i < 32; ++i) mx = fmaxf(mx, x[i]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m, mx);
            if (__builtin_amdgcn_ballot_w64(m_new > m) != 0) {     // (wave-uniform; a factor of 1 would change nothing)
                const float alpha = __builtin_amdgcn_exp2f(m - m_new);
                l *= alpha;
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
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int e = 0; e < 8; ++e) pf[kk][e] = (f16)x[8 * kk + e];
            // O^T += V^T . P^T: the A operand of K-step kk is V[rows 16 kk + 4 hh ..+3 and + 8][feature 32 db + r], two transposed reads
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const int c0 = 4 * db + 2 * (tg & 1) + (tp >> 1);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int row = 16 * kk + 4 * (tg >> 1) + tq;
                    const f16x4 v0 = pa_tr(vb + pa_off(row, c0) + 8 * (tp & 1));
                    const f16x4 v1 = pa_tr(vb + pa_off(row + 8, c0) + 8 * (tp & 1));
                    oacc[db] = mfma32(pa_cat(v0, v1), pf[kk], oacc[db]);
                }
            }
        }
        if (t + 1 < nt) commit((t + 1) & 1);
        __syncthreads();
    }

    const float lt = l + __shfl_xor(l, 32, 64);
    if (active && qrel < len) {
        const float inv = 1.0f / lt;
        f16* orow = obase + (size_t)qrel * qstride;
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                const f16x4 w = {(f16)(oacc[db][4 * gg] * inv), (f16)(oacc[db][4 * gg + 1] * inv), (f16)(oacc[db][4 * gg + 2] * inv),
                                 (f16)(oacc[db][4 * gg + 3] * inv)};
                *reinterpret_cast<f16x4*>(orow + 32 * db + 8 * gg + 4 * hh) = w;
            }
    }
}

}  // namespace

int fq_launch_prefill_attn(f16* o, const f16* q, const f16* qt, const f16* k, const f16* v, const int* seq_start, const int* seq_len, int batch,
                           int seq, int q_heads, int kv_heads, hipStream_t stream) {
    if (batch < 1 || seq < 1 || kv_heads < 1 || q_heads < 1 || q_heads % kv_heads) return FQ_LAUNCH_NO_KERNEL;
    const int nblk = (seq + PA_QB - 1) / PA_QB;
    const int64_t units = (int64_t)batch * nblk * kv_heads, wgs = units * (q_heads / kv_heads);
    if (wgs > 0x7FFFFFFF) return FQ_LAUNCH_NO_KERNEL;
    PaArgs a = {o, q, qt, k, v, seq_start, seq_len, batch, seq, q_heads, kv_heads, nblk, units % 8 == 0 ? 1 : 0};
    if (qt != nullptr) {
        FQ_RAISE_LDS_CAP((fq_prefill_attn_kernel<true>), PA_LDS);
        hipLaunchKernelGGL((fq_prefill_attn_kernel<true>), dim3((unsigned)wgs), dim3(PA_THREADS), PA_LDS, stream, a);
    } else {
        FQ_RAISE_LDS_CAP((fq_prefill_attn_kernel<false>), PA_LDS);
        hipLaunchKernelGGL((fq_prefill_attn_kernel<false>), dim3((unsigned)wgs), dim3(PA_THREADS), PA_LDS, stream, a);
    }
    return (int)hipGetLastError();
}
