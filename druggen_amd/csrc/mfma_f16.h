// The fp16 MFMA wrappers of the float32 (fp16 hi + lo) kernels and the vector types they work on: row_gemm_k384.hip,
// row_gemm_n384.hip, attn_half_f32.hip, attn_half_f32_bwd.hip, ffn_fused_f32.hip.
//
// The gfx950 hazard they work around.  acc += A . B on v_mfma_f32_16x16x32_f16 is ALWAYS issued in place
// (result registers = accumulator input), through inline asm.  Through the builtin hipcc renamed the destination of some
// MFMAs and put them one slot behind the MFMA that produced their accumulator input; lanes 48..63 of that input were then
// still being written (a few wrong columns per launch, never the same ones: the result latency of this gfx950 opcode is
// longer than the hazard tables assume).  In-place chains are interlocked by the hardware; what the compiler no longer
// sees -- a vector read of a result -- is fenced by mfma_results_ready().  A fix to this workaround is made HERE, once.
#pragma once
#include "common.h"

namespace dg {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void mfma16(f32x4& acc, const f16x8& a, const f16x8& b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
// first MFMA of a chain: accumulator input = the constant 0 (no vector write of the accumulator in front of the chain)
__device__ __forceinline__ void mfma16_first(f32x4& acc, const f16x8& a, const f16x8& b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
}
// in front of the first vector read of a chain's results
__device__ __forceinline__ void mfma_results_ready() { asm volatile("s_nop 15\n\ts_nop 15" ::: "memory"); }
// the same fence in the middle of an MFMA stream, for three finished chains only: tied to their accumulators, so that no
// vector read of them is moved in front of it while the MFMAs of other chains go on behind it
__device__ __forceinline__ void mfma_results_ready(f32x4& a0, f32x4& a1, f32x4& a2) {
    asm volatile("s_nop 15\n\ts_nop 15" : "+v"(a0), "+v"(a1), "+v"(a2)::"memory");
}

}  // namespace dg
