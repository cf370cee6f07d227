// DPP lane reductions of the float32 kernels: one step moves a value inside a 16-lane DPP row and combines it; four steps
// (quad xor 1, quad xor 2, half-row mirror, row mirror) leave the row's total in every lane.  No LDS-crossbar round trips
// (a __shfl_xor butterfly is five dependent ds_bpermute).
#pragma once
#include "common.h"

namespace dg {

// CTRL: 0xB1 quad_perm [1,0,3,2], 0x4E quad_perm [2,3,0,1], 0x141 row_half_mirror, 0x140 row_mirror
// unsigned max (the ordering of |float| bit patterns): 0 is the identity, so the DPP move folds into v_max_u32
template <int CTRL>
__device__ __forceinline__ unsigned umax_dpp(unsigned x) {
    const unsigned moved = static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), CTRL, 0xF, 0xF, true));
    return x > moved ? x : moved;
}
template <int CTRL>
__device__ __forceinline__ float sum_dpp(float x) {
    return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ float max_dpp(float x) {
    return fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true)));
}
// over the 16 lanes of a DPP row, result in every lane
__device__ __forceinline__ float row16_sum(float x) {
    x = sum_dpp<0xB1>(x);
    x = sum_dpp<0x4E>(x);
    x = sum_dpp<0x141>(x);
    return sum_dpp<0x140>(x);
}
__device__ __forceinline__ float row16_max(float x) {
    x = max_dpp<0xB1>(x);
    x = max_dpp<0x4E>(x);
    x = max_dpp<0x141>(x);
    return max_dpp<0x140>(x);
}
// Sum over the 32 lanes of a half-wave, result in every lane.  Two forms that compile differently; each kernel keeps the
// one it was measured with.
//   _readlane: the four 16-lane row totals are read as scalars (four v_readlane + their wait states), `upper` selects
//              the half-wave's pair (row_gemm.hip, row_gemm_k384.hip);
//   _swap:     the two row totals of the half-wave meet through one v_permlane16_swap (attn_half_f32*.hip).
__device__ __forceinline__ float half_wave_total_readlane(float x, bool upper) {
    x = row16_sum(x);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 48));
    return upper ? r2 + r3 : r0 + r1;
}
__device__ __forceinline__ float half_wave_total_swap(float x) {
    x = row16_sum(x);
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// Integer sum over the 64 lanes of a wave, result in every lane (mol_desc.hip): the four row steps above, then the rows meet
// through v_permlane16_swap / v_permlane32_swap of the value with itself, as in common.h's xor_step.  Every lane of the wave
// must be active.
template <int CTRL>
__device__ __forceinline__ unsigned usum_dpp(unsigned x) {
    return x + static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ unsigned wave_usum(unsigned x) {
    x = usum_dpp<0xB1>(x);
    x = usum_dpp<0x4E>(x);
    x = usum_dpp<0x141>(x);
    x = usum_dpp<0x140>(x);
    auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    x = r[0] + r[1];
    r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return r[0] + r[1];
}

}  // namespace dg
