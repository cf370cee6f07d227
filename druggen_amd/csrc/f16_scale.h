// Scale arithmetic and fp16 hi + lo split of the float32 kernels.  All scales are powers of two, built and inverted
// by exponent arithmetic (exact; v_rcp_f32 is a 1-ulp approximation).
#pragma once
#include "mfma_f16.h"

namespace dg {

__device__ __forceinline__ float comp(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// ---- one scale per ROW (activations) or per output COLUMN (packed weights): row_gemm*.hip, ffn_fused_f32.hip ----------
// The scale brings the largest magnitude into [2^14, 2^15); x scale = hi + lo with hi = fp16(x scale), lo = fp16 of the
// (exact) remainder: 22 significand bits of every element within 2^-18 of the maximum.
__device__ __forceinline__ unsigned scale_exponent(float absmax) {   // biased exponent, clamped away from 0
    const unsigned e = __float_as_uint(absmax) >> 23;
    return e < 15u ? 15u : e;
}
__device__ __forceinline__ float scale_of(unsigned e) { return __uint_as_float((268u - e) << 23); }      // 2^(14 - (e - 127))
__device__ __forceinline__ float inv_scale_of(unsigned e) { return __uint_as_float((e - 14u) << 23); }
// packed fp16 pair { fp16(s0 - hi.lo), fp16(s1 - hi.hi) }: the lo plane of two scaled values whose hi plane is `hpk`
__device__ __forceinline__ unsigned lo_pair(unsigned hpk, float s0, float s1) {
    unsigned d;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(hpk), "v"(s0));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(d) : "v"(hpk), "v"(s1));
    return d;
}

// ---- running scales along the contraction (weight gradients: linear_wgrad.hip, wgrad_stream.hip) ----------------------
// 2^(8 - floor(log2 m)) for a finite m > 0: the scale that maps m into [2^8, 2^9).  A column's scale moves again
// only when a later value is 64-128 times larger than the one that set it (fp16 holds 2^16): on real gradients a
// tighter window (2^12: 4-8 times) had some column of nearly every 16-row step of a wave moving, and every move
// costs the wave ~2 steps.  Elements more than 2^11 below their column's running maximum lose relative (not
// absolute) accuracy: absolute error 2^-25 scaled units = 2^-33 of that maximum.
__device__ __forceinline__ float scale_for(float m) {
    const int e = static_cast<int>((__float_as_uint(m) >> 23) & 255u);      // biased exponent (0 for denormals)
    int be = 127 + 8 - (e - 127);
    be = be > 253 ? 253 : (be < 1 ? 1 : be);
    return __uint_as_float(static_cast<unsigned>(be) << 23);
}
__device__ __forceinline__ float pow2_ratio(float num, float den) {      // num <= den, both powers of two
    const int d = static_cast<int>(__float_as_uint(num) >> 23) - static_cast<int>(__float_as_uint(den) >> 23) + 127;
    return d < 1 ? 0.f : __uint_as_float(static_cast<unsigned>(d) << 23);
}
__device__ __forceinline__ float pow2_inv(float p) {                      // p in [2^-126, 2^126]
    return __uint_as_float((254u - (__float_as_uint(p) >> 23)) << 23);
}
// the pair (v0, v1) * sc as packed hi and lo words: hi = s rounded toward zero to fp16 (11 significant bits), lo = s - hi
// (exact in fp32) rounded toward zero; hi_a hi_b + hi_a lo_b + lo_a hi_b leaves a relative error of 2^-22 per product
__device__ __forceinline__ void split2_f16(float v0, float v1, float sc, unsigned& hw, unsigned& lw) {
    const float s0 = v0 * sc, s1 = v1 * sc;
    hw = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(s0, s1));
    // v_fma_mix_f32 reads the fp16 halves of `hw` directly (hipcc emits cvt + sub)
    float l0, l1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(hw), "v"(s0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(hw), "v"(s1));
    lw = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(l0, l1));
}

}  // namespace dg
