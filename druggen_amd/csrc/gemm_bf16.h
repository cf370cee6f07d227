// Device-side building blocks of the bf16 row kernels (gemm_bf16.hip, ffn_bf16.hip).
//
// Activation tiles: 64 rows x K channels of bf16, row-major with a 2K-byte pitch; inside every
// 256-byte segment of a row the 16-byte chunk index is XOR-ed with (row & 15).  Tiles arrive by
// LDS-DMA (destination lane-linear, the permutation is applied to the per-lane SOURCE address) or
// are written by an MFMA epilogue with the same permutation.  A ds_read_b128 of one MFMA operand
// fragment -- lane = (row, 8-channel group) -- is then bank-conflict free for both bf16 MFMA shapes.
//
// Weights: fp32 nn.Linear parameters are converted once per weight version into bf16 MFMA
// *fragment order*; a wave keeps its fragments in VGPRs for the whole (persistent) kernel.
//   P32[(mb * KS + ks) * 64 + lane] = { W'[32 mb + (lane & 31)][16 ks + 8 (lane >> 5) + j] } j < 8   (32x32x16)
//   P16[(mb * KS + ks) * 64 + lane] = { W'[16 mb + (lane & 15)][32 ks + 8 (lane >> 4) + j] } j < 8   (16x16x32)
// with y = x . W'^T: W' = W (mode 0, forward) or W^T (mode 1, input gradient).  The same fragment
// serves as the A operand ("swapped" product W' . x^T: a lane ends up with 4 consecutive output
// channels of one row) or as the B operand (x . W'^T: 4 consecutive rows of one output channel).
#pragma once

#include "bf16.h"
#include "lane_reduce.h"

namespace dg {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRowsPerTile = 64;

// byte offset of channel `ch` (multiple of 8 for a 16-byte chunk) of tile row `row`, K channels per row
__device__ __forceinline__ unsigned tile_off(int row, int ch, int K) {
    const int chunk = ch >> 3;
    const int sw = (chunk & ~15) | ((chunk & 15) ^ (row & 15));
    return static_cast<unsigned>(row * (K * 2) + sw * 16 + (ch & 7) * 2);
}

// Start the LDS-DMA of one 64 x K bf16 tile (rows r0.. of a [R, K] matrix) into `lds_dst`; all
// `WAVES` waves of the workgroup take part.  Rows >= R are not fetched (the tile keeps stale bytes
// there; nothing computed from them is ever stored).  The caller waits (vmcnt) and synchronises.
template <int K, int WAVES>
__device__ __forceinline__ void dma_tile_bf16(const bf16_t* __restrict__ a, int64_t r0, int64_t R, char* lds_dst,
                                              int wave, int lane) {
    constexpr int CPR = K / 8;                       // 16-byte chunks per row
    constexpr int INSTR = kRowsPerTile * CPR / 64;   // wave-instructions per tile
    const unsigned dst = lds_byte_address(lds_dst);
    static_assert(INSTR % WAVES == 0, "tile must split evenly over the waves");
#pragma unroll
    for (int t = 0; t < INSTR / WAVES; ++t) {
        const int ii = wave + t * WAVES;
        const int L = ii * 64 + lane;
        const int row = L / CPR, cpos = L % CPR;
        const int src = (cpos & ~15) | ((cpos & 15) ^ (row & 15));
        if (r0 + row < R)
            dma16_async(reinterpret_cast<const float*>(a + (r0 + row) * K + src * 8), dst + ii * 1024);
    }
}

// sum over the 32 lanes of a half-wave, result in every lane (lane_reduce.h)
__device__ __forceinline__ float half_wave_sum(float x) { return half_wave_total_readlane(x, threadIdx.x & 32); }

// ---- the bf16 MFMA, operand concatenation and LDS-only barrier of attn_half.hip, embed_bf16.hip, ffn_bf16.hip ----------
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 cat8(u32x2_t lo, u32x2_t hi) {
    const u32x4_t t = {lo[0], lo[1], hi[0], hi[1]};
    return __builtin_bit_cast(bf16x8, t);
}
// Workgroup barrier that orders LDS traffic only: the kernels below wait for their LDS-DMA BEFORE issuing a tile's
// global stores (the DMA of the next tile was issued a whole tile earlier, so that wait is free), and must not sit on
// `vmcnt(0)` at the next barrier until those stores have been acknowledged (PMC: waves parked > 50 % of their cycles).
// (The two empty asm statements are COMPILER barriers: s_barrier is IntrNoMem for LLVM, which is otherwise free to move
// LDS loads / stores across it.)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xC07F);      // lgkmcnt(0); vmcnt / expcnt untouched
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// ---- fp32 exchange tile [64][N]: accumulators (a lane owns 4 consecutive channels of a row) go in
// as 16-byte slots XOR-ed with (row & 7) (conflict-free ds_write_b128 / ds_read_b128), whole rows
// come out: lane `col` of a half-wave reads channels [4 col, 4 col + 4) of each 128-channel chunk.
__device__ __forceinline__ unsigned xch_off(int row, int ch, int N) {
    const int slot = ch >> 2;
    return static_cast<unsigned>(row * (N * 4) + (((slot & ~7) | ((slot & 7) ^ (row & 7))) << 4));
}

}  // namespace dg
