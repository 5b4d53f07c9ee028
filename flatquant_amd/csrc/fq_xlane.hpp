// fq_xlane.hpp — the six cross-lane butterfly stages of the register FWHT (partner = lane ^ 2^s, s = 0 .. 5), shared by
// fq_hadamard_reg.hip (the standalone rotation) and fq_kvcache.hip (the 128-point rotation of the decode launch's queries and
// new K row, fq_kv_decode_append_had_i4): one body, so both compute the same fp32 sums in the same order.
//   quad_perm DPP (s = 0, 1), row shifts with masked add / sub (s = 2, 3), v_permlane16_swap / v_permlane32_swap (s = 4, 5).
// A lane whose bit s is set needs partner - own: its own value gets the sign bit flipped first (exact), then both kinds of lane add.
#pragma once
#include "fq_common.hpp"

namespace {

template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float flip(float v, unsigned m) {
    return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) ^ m);
}

// per-lane constants of the six cross-lane stages: sign-bit masks (0x80000000 where bit s of the lane number is set)
// for the stages that flip-and-add, +-1.0f for the two that use an fma
struct XMask {
    unsigned m[2];
    float sgn[2];
    __device__ __forceinline__ explicit XMask(int lane) {
        m[0] = (lane & 1) ? 0x80000000u : 0u;
        m[1] = (lane & 2) ? 0x80000000u : 0u;
        sgn[0] = (lane & 16) ? -1.0f : 1.0f;
        sgn[1] = (lane & 32) ? -1.0f : 1.0f;
    }
};

// the six cross-lane butterfly stages on one register (14 VALU). "s_nop 1": a VALU result needs two wait states
// before a DPP / permlane read of it.
template <int XS = 6>  // XS: how many of the stages (lane ^ 1, 2, 4, 8, 16, 32) to run: vectors of 8 * 2^XS elements
__device__ __forceinline__ float xlane(float v, const XMask& k) {
    v = flip(v, k.m[0]) + dppf<0xB1>(v);  // lane ^ 1: quad_perm [1,0,3,2]; lanes with the bit set need partner - own
    v = flip(v, k.m[1]) + dppf<0x4E>(v);  // lane ^ 2: quad_perm [2,3,0,1]
    if (XS == 3) {  // lane ^ 4 only
        float r;
        asm volatile("s_nop 1\n\t"
                     "v_add_f32_dpp %0, %1, %1 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                     "v_sub_f32_dpp %0, %1, %1 row_shr:4 row_mask:0xf bank_mask:0xa"
                     : "=&v"(r) : "v"(v));
        return r;
    }
    {   // lane ^ 4 and lane ^ 8: the partner sits one / two banks (groups of 4 lanes) away -> row shifts, one masked add
        // for the lower lanes of each pair (own + partner) and one masked sub for the upper ones (partner - own)
        float r;
        asm volatile("s_nop 1\n\t"
                     "v_add_f32_dpp %0, %1, %1 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                     "v_sub_f32_dpp %0, %1, %1 row_shr:4 row_mask:0xf bank_mask:0xa"
                     : "=&v"(r) : "v"(v));
        asm volatile("s_nop 1\n\t"
                     "v_add_f32_dpp %0, %1, %1 row_shl:8 row_mask:0xf bank_mask:0x3\n\t"
                     "v_sub_f32_dpp %0, %1, %1 row_shr:8 row_mask:0xf bank_mask:0xc"
                     : "=&v"(v) : "v"(r));
    }
    if (XS == 4) return v;
    {   // lane ^ 16: after the swap, a = value of the lower lane of the pair, b = of the upper one, in BOTH lanes' view
        // (even rows keep a = own and receive b = partner; odd rows receive a = partner and keep b = own)
        float a = v, b = v;
        asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
        v = __builtin_fmaf(b, k.sgn[0], a);  // a +- b, one rounding
    }
    if (XS == 5) return v;
    {   // lane ^ 32: same with the wave's halves
        float a = v, b = v;
        asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
        v = __builtin_fmaf(b, k.sgn[1], a);
    }
    return v;
}

}  // namespace
