// fq_rope.hip — rotary position embedding of the queries and keys of `tokens` tokens in ONE launch (fq_rope_f16): what transformers'
// apply_rotary_pos_emb(q, k, cos, sin, unsqueeze_dim=2) computes on fp16 tensors of the layout the attention here uses,
//   q [tokens, q_heads, head_dim], k [tokens, k_heads, head_dim], cos / sin [tokens, head_dim]:
//   out[j] = rn16(rn16(x[j] cos[j]) + rn16(r[j] sin[j])),  r[j] = -x[j + hd / 2] (j < hd / 2), x[j - hd / 2] otherwise
// — about ten element-wise torch launches per layer and step (slice, negate, concatenate, two multiplies and an add, for q and again for k).
// The three fp16 roundings are the contract (fqkv::kv_rope8: no fused multiply-add); cos / sin are taken as given (their halves need not be
// equal, frequency scaling is the caller's). A streaming kernel: a thread owns eight features j .. j + 7 of one (token, head) row AND their
// partners at + hd / 2 — six 16-byte loads, two 16-byte stores, no traffic between lanes — so an output may be its own input.
#include "fq_kv_common.hpp"
#include "fq_launch.hpp"

namespace {

template <int HD>
__global__ __launch_bounds__(256) void fq_rope_kernel(f16* q_out, f16* k_out, const f16* q, const f16* k, const f16* __restrict__ cs,
                                                      const f16* __restrict__ sn, int q_heads, int k_heads) {
    constexpr int CPH = HD / 16;     // threads per (token, head) row
    // blockIdx.x: the token; blockIdx.y * 256 + threadIdx.x: (head, chunk) of it — no division anywhere (CPH is a power of two)
    const int i = (int)blockIdx.y * 256 + (int)threadIdx.x;
    if (i >= (q_heads + k_heads) * CPH) return;
    const int c = i % CPH, head = i / CPH;
    const size_t tok = blockIdx.x;
    const bool is_q = head < q_heads;
    const size_t row = is_q ? ((size_t)tok * q_heads + head) * HD : ((size_t)tok * k_heads + (head - q_heads)) * HD;
    const f16* x = (is_q ? q : k) + row;
    f16* y = (is_q ? q_out : k_out) + row;
    const f16x8 lo = __builtin_bit_cast(f16x8, reinterpret_cast<const uint4*>(x)[c]);
    const f16x8 hi = __builtin_bit_cast(f16x8, reinterpret_cast<const uint4*>(x + HD / 2)[c]);
    const size_t t0 = (size_t)tok * HD;
    const f16x8 c_lo = __builtin_bit_cast(f16x8, reinterpret_cast<const uint4*>(cs + t0)[c]);
    const f16x8 c_hi = __builtin_bit_cast(f16x8, reinterpret_cast<const uint4*>(cs + t0 + HD / 2)[c]);
    const f16x8 s_lo = __builtin_bit_cast(f16x8, reinterpret_cast<const uint4*>(sn + t0)[c]);
    const f16x8 s_hi = __builtin_bit_cast(f16x8, reinterpret_cast<const uint4*>(sn + t0 + HD / 2)[c]);
    const f16x8 o_lo = fqkv::kv_rope8(lo, -hi, c_lo, s_lo);
    const f16x8 o_hi = fqkv::kv_rope8(hi, lo, c_hi, s_hi);
    reinterpret_cast<uint4*>(y)[c] = __builtin_bit_cast(uint4, o_lo);
    reinterpret_cast<uint4*>(y + HD / 2)[c] = __builtin_bit_cast(uint4, o_hi);
}

}  // namespace

// q_heads / k_heads: 0 for a tensor that is not there (its pointers are then never read)
int fq_launch_rope(f16* q_out, f16* k_out, const f16* q, const f16* k, const f16* cos, const f16* sin, int64_t tokens, int q_heads, int k_heads,
                   int head_dim, hipStream_t stream) {
    if ((head_dim != 64 && head_dim != 128) || q_heads + k_heads < 1) return FQ_LAUNCH_NO_KERNEL;
    if (tokens <= 0) return 0;
    if (tokens > 0x7FFFFFFF) return FQ_LAUNCH_NO_KERNEL;
    const dim3 grid((unsigned)tokens, (unsigned)(((q_heads + k_heads) * (head_dim / 16) + 255) / 256));
    if (head_dim == 128)
        hipLaunchKernelGGL(fq_rope_kernel<128>, grid, dim3(256), 0, stream, q_out, k_out, q, k, cos, sin, q_heads, k_heads);
    else
        hipLaunchKernelGGL(fq_rope_kernel<64>, grid, dim3(256), 0, stream, q_out, k_out, q, k, cos, sin, q_heads, k_heads);
    return (int)hipGetLastError();
}
