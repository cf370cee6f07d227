// "Row GEMM" for the per-edge / per-node dense layers of DrugGEN's encoder (reference src/model/layers.py: MHA
// projections :111-116,127,135 and MLP.fc1/fc2 :50-53), float32 activations, with the elementwise neighbours of
// those GEMMs fused in:
//
//     Y[R,N] = epilogue( prologue(A)[R,K] . B )        R = B*N*N rows (518 400 at configs[1])
//
//   forward   B[k][n] = W[n][k]    (y = x W^T + b)          -> pack mode 0
//   dgrad     B[k][n] = W[k][n]    (dx = dy W)              -> pack mode 1
//   epilogue: + bias, ReLU, + residual, LayerNorm(gamma, beta) -> y (+ mean, rstd), or a LayerNorm backward
//
// This file: the host entry points (declared in row_gemm.h), the weight pack (fp16 hi + lo planes in MFMA fragment order,
// never through LDS) and two kernels:
//   row_gemm_h3_kernel       the four 128 -> 128 forms (direct, exchange, LayerNorm backward out / in) and the node-level
//                            three-output q / k / v launch (dg_row_gemm_lin3);
//   row_gemm_h3_sum3_kernel  the input gradient of those three Linears: three [R,128] operands, optional residual
//                            (dg_row_gemm_sum3).
// Every 128 -> 384 and 384 -> 128 launch of dg_row_gemm, ReLU bit masks included, is row_gemm_n384.hip / row_gemm_k384.hip.
// The fp32-MFMA and bf16 x 6 kernels of rounds 1 - 2 are gone.
#include "common.h"
#include "f16_scale.h"
#include "lane_reduce.h"
#include "row_gemm.h"
#include "row_gemm_n384.h"
#include "row_gemm_k384.h"
#include "traversal.h"

#include <cstring>
#include <type_traits>

namespace dg {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTR = 64;          // rows per workgroup tile

struct Epilogue {
    const float* bias = nullptr;      // [N] or null
    // Three Linears in one launch (NG = 3 kernel; q / k / v of an attention block, reference layers.py:111-113): column
    // groups 1 / 2 go to y_alt[0] / y_alt[1] (row pitch 128, like y), their bias comes from bias_alt[0] / bias_alt[1].
    // (y_alt sits here, where the ReLU bit-mask pointers used to be: the fields below keep their kernel-argument offsets,
    // and hipcc groups the scalar loads of the 128 -> 128 instances as it always has)
    float* y_alt[2] = {nullptr, nullptr};
    const float* residual = nullptr;  // [R,N] or null
    const float* gamma = nullptr;     // LayerNorm (needs N == 128) or null
    const float* beta = nullptr;
    float* mean = nullptr;
    float* rstd = nullptr;
    float* pre = nullptr;             // optional [R,N]: the pre-LayerNorm sum, saved for the backward
    float eps = 0.f;
    int relu = 0;
    // LayerNorm-BACKWARD epilogue (LNB kernels): v = a B + residual is the gradient of a LayerNorm output; the row
    // leaves as dz = rstd (v gamma - mean(v gamma) - xhat mean(v gamma xhat)), xhat = (lnb_pre - mean) rstd, with
    // `gamma`, `mean`, `rstd` above read as that LayerNorm's saved parameters / statistics.  Per half-wave partial sums
    // of dgamma = sum_rows v xhat and dbeta = sum_rows v go to lnb_part[(block * 8 + half-wave)][2][128].
    const float* lnb_pre = nullptr;
    float* lnb_part = nullptr;
    // LayerNorm-backward PROLOGUE (LNA kernel): the A operand is dz = LayerNormBackward(a; lna_pre, mean, rstd, gamma),
    // computed by the producer waves on the rows they stream (a is that LayerNorm's OUTPUT gradient); dz is also
    // written to lna_dz [R,128] (the residual path and the weight gradient read it later), dgamma / dbeta partials go
    // to lnb_part in the layout above (half-waves of the four producer waves).
    const float* lna_pre = nullptr;
    float* lna_dz = nullptr;
    const float* bias_alt[2] = {nullptr, nullptr};
    int reverse = 0;      // 128 -> 128 kernels without LayerNorm-backward stages: tiles in descending order (traversal.h)
};

// sum over the 32 lanes of a half-wave, result in every lane (lane_reduce.h)
__device__ __forceinline__ float half_sum(float x) { return half_wave_total_readlane(x, threadIdx.x & 32); }

constexpr int kH3Pitch = 272;                 // bytes per LDS row of one fp16 plane (128 k): conflict-free b128 reads
// LDS image of a 64-row chunk: two fp16 planes (hi, lo), then the 64 inverse row scales of the chunk
constexpr int kH3Plane = kTR * kH3Pitch;
constexpr int kH3Rs = 2 * kH3Plane;           // byte offset of float inv_row_scale[64] (past the 32 KiB exchange tile)
constexpr int kH3Buf = kH3Rs + kTR * 4;
constexpr int kH3Lds = 2 * kH3Buf;
static_assert(kH3Rs >= kTR * 128 * 4, "the fp32 exchange tile must not reach the row scales");

// ---- fp16 x 3: power-of-two scaled two-plane split -------------------------------------------------------
// A row a (and a weight column w) is multiplied by a power of two that brings its largest magnitude into
// [2^14, 2^15) -- exact -- and split as hi = fp16(x), lo = fp16(x - hi): the residual is exact in fp32 and
// hi + lo carries 22 significand bits of every element that is within 2^-18 of the row maximum (smaller
// elements lose bits only below 2^-39 of the maximum).  a.w ~= hi.hi + hi.lo + lo.hi with fp32
// accumulation (the dropped lo.lo term is 2^-22 relative): three MFMAs per product instead of the six of
// the bf16 three-plane split, two LDS planes instead of three, and the same fp32-class error (measured
// against fp64 in tests/test_hip_kernels.py).  The epilogue multiplies by the inverse scales
// (f16_scale.h).

// Producer side of the fp16x3 kernels: thread `pt` holds PFN float4s, the i-th belonging to tile row (pt + STRIDE i) >> 5
// at float4 column (pt & 31) (the 32 lanes of a half-wave hold one 128-wide row).  Row maximum -> power-of-two scale
// -> hi / lo fp16 planes + the inverse scale, written to the LDS image `pl`.  The work is staged across groups of
// eight float4s so that the eight independent dependency chains (DPP reduction, conversions) interleave instead of
// running one after the other: the producers' VALU latency is the critical path of these kernels.
template <int PFN, int STRIDE>
__device__ __forceinline__ void split_write_h3(const float4 (&set)[PFN], char* pl, int pt) {
    constexpr int G = PFN > 8 ? 2 : 4;   // the 16-float4 producers (two waves) are short of registers
    static_assert(PFN % G == 0 && STRIDE % 32 == 0, "whole groups, whole rows");
    char* const prow = pl + (pt >> 5) * kH3Pitch + (pt & 31) * 8;
    char* const prs = pl + kH3Rs + (pt >> 5) * 4;
#pragma unroll
    for (int g0 = 0; g0 < PFN; g0 += G) {
        unsigned m[G];
#pragma unroll
        for (int j = 0; j < G; ++j) {   // |.| maximum of the four components: two VOP3 instructions with abs modifiers
            const float4& v = set[g0 + j];
            float t, u;
            asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(t) : "v"(v.x), "v"(v.y), "v"(v.z));
            asm("v_max_f32_e64 %0, |%1|, %2" : "=v"(u) : "v"(v.w), "v"(t));
            m[j] = __float_as_uint(u);
        }
#pragma unroll
        for (int j = 0; j < G; ++j) m[j] = umax_dpp<0xB1>(m[j]);
#pragma unroll
        for (int j = 0; j < G; ++j) m[j] = umax_dpp<0x4E>(m[j]);
#pragma unroll
        for (int j = 0; j < G; ++j) m[j] = umax_dpp<0x141>(m[j]);
#pragma unroll
        for (int j = 0; j < G; ++j) m[j] = umax_dpp<0x140>(m[j]);
        float sc[G];
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const auto r = __builtin_amdgcn_permlane16_swap(m[j], m[j], false, false);
            const unsigned x = r[0] > r[1] ? r[0] : r[1];
            const unsigned e = max(x >> 23, 15u);
            m[j] = e;
            sc[j] = scale_of(e);
        }
        f32x2 xa[G], xb[G];
        f16x2 ha[G], hb[G];
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const float4& v = set[g0 + j];
            xa[j] = f32x2{v.x, v.y} * sc[j];
            xb[j] = f32x2{v.z, v.w} * sc[j];
        }
#pragma unroll
        for (int j = 0; j < G; ++j) {
            ha[j] = __builtin_convertvector(xa[j], f16x2);
            hb[j] = __builtin_convertvector(xb[j], f16x2);
        }
#pragma unroll
        for (int j = 0; j < G; ++j) {
            xa[j] -= __builtin_convertvector(ha[j], f32x2);
            xb[j] -= __builtin_convertvector(hb[j], f32x2);
        }
#pragma unroll
        for (int j = 0; j < G; ++j) {
            // row (pt >> 5) + (STRIDE / 32) (g0 + j): one base address per call, the rest are store-offset immediates
            const f16x2 la = __builtin_convertvector(xa[j], f16x2), lb = __builtin_convertvector(xb[j], f16x2);
            const u32x2 h = {__builtin_bit_cast(unsigned, ha[j]), __builtin_bit_cast(unsigned, hb[j])};
            const u32x2 l = {__builtin_bit_cast(unsigned, la), __builtin_bit_cast(unsigned, lb)};
            *reinterpret_cast<u32x2*>(prow + 0 * kH3Plane + (STRIDE / 32) * (g0 + j) * kH3Pitch) = h;
            *reinterpret_cast<u32x2*>(prow + 1 * kH3Plane + (STRIDE / 32) * (g0 + j) * kH3Pitch) = l;
        }
        if ((pt & 31) == 0) {   // one divergent block per group (branches between the stages would serialise the chains)
#pragma unroll
            for (int j = 0; j < G; ++j)
                *reinterpret_cast<float*>(prs + (STRIDE / 32) * (g0 + j) * 4) = inv_scale_of(m[j]);
        }
    }
}

// packed fp16x3 weights: [slab][k-step][plane 0/1][lane] x 8 fp16, then float inv_col_scale[32 * slabs] (one scale
// per output column over the whole contraction).  One 512-thread workgroup per (32-column slab, 128-wide k
// chunk): thread = (k-step, lane) keeps its 8 values in registers while the column maxima are reduced through LDS.
// (w1, w2 non-null: the matrix is the vertical stack [w; w1; w2] of three [128, cols] weights -- q / k / v of an
// attention block packed as ONE 128 -> 384 forward operand or ONE 384 -> 128 input-gradient operand)
__device__ __forceinline__ void pack_weight_h3_block(const float* __restrict__ w, const float* __restrict__ w1,
                                                     const float* __restrict__ w2, f16x8* __restrict__ p, int rows, int cols,
                                                     int mode, int n_tiles, int t, int kcb, int kchunks) {
    __shared__ unsigned part[16][32];
    const int k_steps = 8 * kchunks;
    const int lane = threadIdx.x & 63, ks = threadIdx.x >> 6;
    const int c = lane & 31, n = 32 * t + c;
    const int n_out = mode == 0 ? rows : cols, kdim = mode == 0 ? cols : rows;
    auto at = [&](int k) -> float {
        if (n >= n_out || k >= kdim) return 0.f;
        int r = mode == 0 ? n : k;
        const int c = mode == 0 ? k : n;
        const float* ws = w;
        if (w1) {
            ws = r < 128 ? w : (r < 256 ? w1 : w2);
            r &= 127;
        }
        return ws[static_cast<size_t>(r) * cols + c];
    };
    float v[8];
    unsigned mx = 0;
    for (int kc = 0; kc < kchunks; ++kc)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = at(kc * 128 + ks * 16 + 8 * (lane >> 5) + j);
            if (kc == kcb) v[j] = x;
            mx = max(mx, __float_as_uint(x) & 0x7FFFFFFFu);
        }
    part[2 * ks + (lane >> 5)][c] = mx;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) mx = max(mx, part[i][c]);
    const unsigned e = scale_exponent(__uint_as_float(mx));
    const float sc = scale_of(e);
    f16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float xs = v[j] * sc;
        hi[j] = static_cast<_Float16>(xs);
        lo[j] = static_cast<_Float16>(xs - static_cast<float>(hi[j]));
    }
    const size_t slot = static_cast<size_t>(t) * k_steps + 8 * kcb + ks;
    p[(slot * 2 + 0) * 64 + lane] = hi;
    p[(slot * 2 + 1) * 64 + lane] = lo;
    if (kcb == 0 && ks == 0 && lane < 32)
        reinterpret_cast<float*>(p + static_cast<size_t>(n_tiles) * k_steps * 2 * 64)[n] = inv_scale_of(e);
}
__global__ __launch_bounds__(512) void pack_weight_h3_kernel(const float* __restrict__ w, const float* __restrict__ w1,
                                                             const float* __restrict__ w2, f16x8* __restrict__ p, int rows,
                                                             int cols, int mode, int n_tiles) {
    pack_weight_h3_block(w, w1, w2, p, rows, cols, mode, n_tiles, blockIdx.x, blockIdx.y, gridDim.y);
}
// Every weight of a network in ONE launch (after an optimizer step): blockIdx.z walks a device table of
// { w, packed, rows, cols, mode, w1, w2 } (int64 x 7; w1 = w2 = 0 unless the entry is a stack of three weights); blocks
// outside an entry's (slab, k-chunk) grid leave at once.
__global__ __launch_bounds__(512) void pack_weight_h3_batch_kernel(const long long* __restrict__ table) {
    const long long* e = table + 7 * static_cast<size_t>(blockIdx.z);
    const float* w = reinterpret_cast<const float*>(e[0]);
    f16x8* p = reinterpret_cast<f16x8*>(e[1]);
    const int rows = static_cast<int>(e[2]), cols = static_cast<int>(e[3]), mode = static_cast<int>(e[4]);
    const int n_out = mode == 0 ? rows : cols, k = mode == 0 ? cols : rows;
    const int nt = (n_out + 31) / 32, kc = (k + 127) / 128;
    if (static_cast<int>(blockIdx.x) >= nt || static_cast<int>(blockIdx.y) >= kc) return;      // block-uniform
    pack_weight_h3_block(w, reinterpret_cast<const float*>(e[5]), reinterpret_cast<const float*>(e[6]), p, rows, cols, mode,
                         nt, blockIdx.x, blockIdx.y, kc);
}

// Workgroup program: 8 waves, one workgroup per CU, persistent over 64-row tiles.
//   waves 4..7  producers: stream A chunks (64 rows x 128 k fp32) HBM -> registers (three chunks deep,
//               96 KiB in flight per CU) -> split -> fp16 hi / lo planes in LDS (double-buffered);
//   waves 0..3  consumers: wave w = 32-column slab w of the current 128-column group: 3 MFMAs per
//               (k-step, 32-row block) on fragments read from the planes, then the epilogue.
// One barrier per chunk separates "planes[c] written" from "planes[c] read".  K = 128: one chunk per tile.
// NG = 1, the four 128 -> 128 forms: direct epilogue (bias, ReLU), exchange epilogue (EXCH: + residual, LayerNorm),
// LayerNorm backward as the epilogue (LNB) or on the way in (LNA); the B fragments stay resident.
// NG = 3, the node-level q / k / v launch: three [R,128] outputs, one column group per Linear.  The three groups of a
// tile run back to back on the same planes, and the B fragments of a group (64 VGPRs, two halves) are double-buffered:
// the next group's arrive from L2 during this group's MFMAs.
template <int NG, bool EXCH, bool LNB = false, bool LNA = false>
__global__ __launch_bounds__(512, 2) void row_gemm_h3_kernel(const float* __restrict__ a, const f16x8* __restrict__ packed,
                                                             float* __restrict__ y, int64_t R, Epilogue ep) {
    // K = 128: one chunk per tile, the row scale covers the whole contraction
    constexpr int NC = 4, NM = 8 - NC, PFN = 2048 / (64 * NM);   // consumer / producer waves, float4 per producer thread and chunk
    constexpr int K = 128, KS = 8;
    static_assert(!LNB || (EXCH && NG == 1), "LayerNorm-backward epilogue: 128 -> 128 exchange kernel");
    static_assert(!LNA || (!EXCH && !LNB && NG == 1), "LayerNorm-backward prologue: plain 128 -> 128 kernel");
    static_assert(NG == 1 || (NG == 3 && !EXCH && !LNB && !LNA), "three outputs: direct epilogue, one column group per Linear");
    constexpr int DEPTH = LNA ? 2 : 3;      // register sets of A chunks the producers keep in flight
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* lds = smem_raw;                              // 2 x { planes[2][64 rows][272 B], inv_row_scale[64] }
    float* xb = reinterpret_cast<float*>(smem_raw + kH3Lds);   // direct epilogue: one 32 x 32 fp32 tile per consumer wave
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, col = lane & 31;
    const int64_t tiles = (R + kTR - 1) / kTR;
    if (static_cast<int64_t>(blockIdx.x) >= tiles) return;
    const int64_t my_tiles = (tiles - blockIdx.x + gridDim.x - 1) / gridDim.x;
    const int64_t nchunks = my_tiles;      // one 128-wide chunk per tile
    // Workgroups walk the three column groups of a tile in rotated orders (blockIdx % 3): at any
    // moment a third of the CUs streams each group's B fragments from L2 instead of all CUs the same 96 KiB.
    const int rot = static_cast<int>(blockIdx.x % 3);
    const int64_t padded = (nchunks + DEPTH - 1) / DEPTH * DEPTH;      // the producers run whole groups of DEPTH iterations
    // tiles round-robin over the workgroups, ascending or (ep.reverse, traversal.h) descending
    auto tile_at = [&](int64_t ti) {
        const int64_t t = blockIdx.x + ti * gridDim.x;
        if constexpr (LNB || LNA || NG == 3) return t;      // (partial sums per workgroup / node-level kernels: always ascending)
        else return ep.reverse ? tiles - 1 - t : t;
    };

    if (w >= NC) {
        // ------------------------------------------------------------------ producers
        const int pt = threadIdx.x - 64 * NC;
        if constexpr (LNA) {
            // ---- LayerNorm backward on the way in.  Thread pt holds float4 column (pt & 31) of tile rows
            // (pt >> 5) + 8 i: the 32 lanes of a half-wave own whole rows, so both row means are DPP sums.  Two register
            // sets of dy rows; ONE set of pre-LayerNorm rows and row statistics, requested as soon as the previous
            // chunk's rows are finished (a chunk period ahead of their use: with four [R,128] streams per tile that
            // period is ~2x the plain kernel's).  Addresses past the end (last tile, padded iterations) are CLAMPED,
            // never branched around: a clamped row recomputes the dz of the row it was clamped to and stores the same
            // values again; only the dgamma / dbeta sums are masked.
            constexpr int K_ = 128;
            float4 dyr[2][PFN], prr[PFN];
            float st;      // lane c < 8: mean of this half-wave's row c ; 8 <= c < 16: rstd of row c - 8
            const float4 gam = ld4(ep.gamma + (pt & 31) * 4);
            float4 dgam = f4(0.f), dbet = f4(0.f);
            const unsigned voff0 = static_cast<unsigned>(pt >> 5) * (K_ * 4) + static_cast<unsigned>(pt & 31) * 16;
            auto offsets = [&](int64_t chunk, int64_t& r0, unsigned& lim) {
                r0 = tile_at(chunk) * kTR;
                const int64_t last = R - 1 - r0;   // >= 0
                lim = last >= kTR - 1 ? 0xFFFFFFFFu
                                      : static_cast<unsigned>(last) * (K_ * 4) + static_cast<unsigned>(pt & 31) * 16;
            };
            auto fetch_dy = [&](auto s_tag, int64_t chunk) {
                constexpr int s = decltype(s_tag)::value;
                if (chunk > nchunks - 1) chunk = nchunks - 1;
                int64_t r0;
                unsigned lim;
                offsets(chunk, r0, lim);
                const char* ba = reinterpret_cast<const char*>(a) + r0 * (K_ * 4);
#pragma unroll
                for (int i = 0; i < PFN; ++i) {
                    unsigned off = voff0 + i * (2 * NM * K_ * 4);
                    off = off < lim ? off : lim;
                    dyr[s][i] = ld4(reinterpret_cast<const float*>(ba + off));
                }
            };
            auto fetch_pre = [&](int64_t chunk) {
                if (chunk > nchunks - 1) chunk = nchunks - 1;
                int64_t r0;
                unsigned lim;
                offsets(chunk, r0, lim);
                const char* bp = reinterpret_cast<const char*>(ep.lna_pre) + r0 * (K_ * 4);
#pragma unroll
                for (int i = 0; i < PFN; ++i) {
                    unsigned off = voff0 + i * (2 * NM * K_ * 4);
                    off = off < lim ? off : lim;
                    prr[i] = ld4(reinterpret_cast<const float*>(bp + off));
                }
                int64_t row = r0 + (pt >> 5) + 8 * (pt & 7);
                if (row > R - 1) row = R - 1;
                st = (pt & 8) ? ep.rstd[row] : ep.mean[row];
            };
            auto write2 = [&](auto s_tag, int64_t chunk) {
                constexpr int s = decltype(s_tag)::value;
                const float live = chunk < nchunks ? 1.f : 0.f;
                const int buf = static_cast<int>(chunk & 1);
                if (chunk > nchunks - 1) chunk = nchunks - 1;
                int64_t r0;
                unsigned lim;
                offsets(chunk, r0, lim);
                char* bz = reinterpret_cast<char*>(ep.lna_dz) + r0 * (K_ * 4);
                const int64_t last = R - 1 - r0;
                // 32-bit row test from a lane term that is opaque per chunk (as loop invariants the eight 64-bit row
                // numbers of a thread are hoisted and spilled)
                const unsigned lastu = static_cast<unsigned>(last < kTR - 1 ? last : kTR - 1);
                unsigned rowt = static_cast<unsigned>(pt) >> 5;
                asm volatile("" : "+v"(rowt));
                const int sti = __float_as_int(st);
                // four rows at a time -- LayerNorm backward, dz store, split into the LDS planes -- fenced: left alone,
                // the scheduler interleaves all eight rows' chains and spills
#pragma unroll
                for (int i0 = 0; i0 < PFN; i0 += 4) {
                    float4 dzs[4];
#pragma unroll
                    for (int i = i0; i < i0 + 4; ++i) {
                        // statistics of row i of this half-wave: scalar reads of both half-waves' lanes, then a select
                        const int mu0 = __builtin_amdgcn_readlane(sti, i), mu1 = __builtin_amdgcn_readlane(sti, 32 + i);
                        const int rs0 = __builtin_amdgcn_readlane(sti, 8 + i), rs1 = __builtin_amdgcn_readlane(sti, 40 + i);
                        const float mu = __int_as_float(half ? mu1 : mu0), rs = __int_as_float(half ? rs1 : rs0);
                        const float4 v = dyr[s][i];
                        const float4 xh = rs * (prr[i] - f4(mu));
                        const float4 u = v * gam;
                        const float c1 = half_sum((u.x + u.y) + (u.z + u.w)) * (1.0f / 128.0f);
                        const float c2 = half_sum((u.x * xh.x + u.y * xh.y) + (u.z * xh.z + u.w * xh.w)) * (1.0f / 128.0f);
                        const float4 dz = rs * (u - f4(c1) - c2 * xh);
                        const float ok = rowt + 8u * i <= lastu ? live : 0.f;
                        const float4 vm = ok * v;
                        dgam = fma4(vm, xh, dgam);
                        dbet += vm;
                        dzs[i - i0] = dz;
                        unsigned off = voff0 + i * (2 * NM * K_ * 4);
                        off = off < lim ? off : lim;
                        st4(reinterpret_cast<float*>(bz + off), dz);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    split_write_h3<4, 64 * NM>(dzs, lds + buf * kH3Buf, pt + i0 * (64 * NM));
                    __builtin_amdgcn_sched_barrier(0);
                }
                fetch_pre(chunk + 1);      // the pre rows / statistics of the next chunk
            };
            constexpr std::integral_constant<int, 0> S0{};
            constexpr std::integral_constant<int, 1> S1{};
            fetch_dy(S0, 0);
            fetch_pre(0);
            fetch_dy(S1, 1);
            write2(S0, 0);
            fetch_dy(S0, 2);
            __syncthreads();
            for (int64_t c = 0; c < padded; c += 2) {
                write2(S1, c + 1);
                fetch_dy(S1, c + 3);
                __syncthreads();
                write2(S0, c + 2);
                fetch_dy(S0, c + 4);
                __syncthreads();
            }
            float* pp = ep.lnb_part + (static_cast<size_t>(blockIdx.x) * 8 + 2 * (w - NC) + half) * 256 + (pt & 31) * 4;
            st4(pp, dgam);
            st4(pp + 128, dbet);
            return;
        }
        float4 pf[3][PFN];
        // Straight-line on purpose (chunk indices are clamped instead of guarded): with branches around
        // the loads hipcc can no longer count how many younger loads may stay in flight and drains
        // the whole queue (vmcnt(0)) before every split, which serialises the stream with HBM latency.
        // uniform 64-bit tile base + a 32-bit per-lane byte offset; rows past the end of a partial tile are clamped
        // on the offset (row-major: the row term dominates the comparison)
        const unsigned voff0 = static_cast<unsigned>(pt >> 5) * (K * 4) + static_cast<unsigned>(pt & 31) * 16;
        auto fetch = [&](float4 (&set)[PFN], int64_t chunk) {
            if (chunk > nchunks - 1) chunk = nchunks - 1;
            const int64_t r0 = tile_at(chunk) * kTR;
            const char* base = reinterpret_cast<const char*>(a) + r0 * (K * 4);
            const int64_t last = R - 1 - r0;   // >= 0
            const unsigned lim = last >= kTR - 1 ? 0xFFFFFFFFu
                                                 : static_cast<unsigned>(last) * (K * 4) + static_cast<unsigned>(pt & 31) * 16;
#pragma unroll
            for (int i = 0; i < PFN; ++i) {
                unsigned off = voff0 + i * (2 * NM * K * 4);   // 64 NM threads = 2 NM rows per step
                off = off < lim ? off : lim;
                set[i] = ld4(reinterpret_cast<const float*>(base + off));
            }
        };
        auto write = [&](const float4 (&set)[PFN], int64_t chunk) {   // chunks past the end land in the idle buffer
            split_write_h3<PFN, 64 * NM>(set, lds + (chunk & 1) * kH3Buf, pt);
        };
        auto end_of_iteration = [&](int64_t c) {
            if (EXCH && c < nchunks) {   // the consumers' exchange epilogue: two more barriers
                __syncthreads();
                __syncthreads();
            }
            __syncthreads();
        };
        fetch(pf[0], 0);
        fetch(pf[1], 1);
        fetch(pf[2], 2);
        write(pf[0], 0);
        fetch(pf[0], 3);
        __syncthreads();
        for (int64_t c = 0; c < padded; c += 3) {
            // iteration c writes chunk c + 1 (the consumers are on chunk c) and refills its register set
            write(pf[1], c + 1);
            fetch(pf[1], c + 4);
            end_of_iteration(c);
            write(pf[2], c + 2);
            fetch(pf[2], c + 5);
            end_of_iteration(c + 1);
            write(pf[0], c + 3);
            fetch(pf[0], c + 6);
            end_of_iteration(c + 2);
        }
        return;
    }

    // ---------------------------------------------------------------------- consumers
    // B fragments of the current unit in two halves (k-steps 0-3 and 4-7, 32 VGPRs each).  When the unit changes
    // (NG = 3) the halves form a ring: half 1 of this unit is requested from L2 at the start of the unit, half 0 of
    // the next unit after the first four k-steps.
    f16x8 bset[2][2][4];
    auto slab_of = [&](int g) { return 4 * g + w; };      // the wave's 32-column slab of column group g
    auto load_b = [&](f16x8 (&bfr)[2][4], int g, int h) {
        const f16x8* wp = packed + static_cast<size_t>(slab_of(g)) * KS * 2 * 64 + lane;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int p = 0; p < 2; ++p) bfr[p][ks] = wp[((4 * h + ks) * 2 + p) * 64];
    };
    const float* inv_cs = reinterpret_cast<const float*>(packed + static_cast<size_t>(4 * NG) * KS * 2 * 64);
    float bias_g[NG], cs_g[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int n = 32 * slab_of(g) + col;
        if (NG == 3) {      // the column group selects the Linear, n & 127 its output channel
            const float* bp = n < 128 ? ep.bias : ep.bias_alt[(n >> 7) - 1];
            bias_g[g] = bp ? bp[n & 127] : 0.f;
        } else {
            bias_g[g] = ep.bias ? ep.bias[n] : 0.f;
        }
        cs_g[g] = inv_cs[n];
    }
    float4 res[8];   // EXCH: residual rows of the tile, requested before its MFMAs
    float4 lpre[LNB ? 4 : 1];      // LNB: rows of the saved pre-LayerNorm sum (four at a time)
    float4 dgam = f4(0.f), dbet = f4(0.f);      // LNB: this lane's four columns, summed over every row it finishes
    f32x16 acc[2];
    // one unit = one (tile, column group): MFMAs on planes[chunk & 1] with the two halves of `bset`, then the epilogue;
    // NG = 3: each half is refilled with the following unit's fragments as soon as its MFMAs are issued
    auto unit = [&](int64_t ti, int pos_g) {   // positions within the tile; values are rotated
        const int g = NG > 1 ? (pos_g + rot) % NG : 0;
        const int64_t chunk = ti;
        const int64_t tix = tile_at(ti);
        const int64_t r0 = tix * kTR;
        if (NG > 1) load_b(bset[1], g, 1);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
        // rows of this wave in the exchange epilogue: w * 16 + it * 2 + half, clamped to the last row of a partial tile
        // in 32 bits: uniform 64-bit tile base + a per-lane byte offset derived HERE from lane terms that are opaque per
        // tile (as loop invariants the per-row pointers are hoisted out of the tile loop and spilled)
        unsigned colv = static_cast<unsigned>(col), halfv = static_cast<unsigned>(half);
        if (EXCH) asm volatile("" : "+v"(colv), "+v"(halfv));
        const unsigned lastr = static_cast<unsigned>(R - 1 - r0 < kTR - 1 ? R - 1 - r0 : kTR - 1);
        auto row_off = [&](int it) {
            unsigned rr = static_cast<unsigned>(w * 16 + it * 2) + halfv;
            rr = rr < lastr ? rr : lastr;
            return rr * 512u + colv * 16u;
        };
        if (EXCH && ep.residual) {
            const char* rbase = reinterpret_cast<const char*>(ep.residual) + r0 * 512;
#pragma unroll
            for (int it = 0; it < 8; ++it) res[it] = ld4(reinterpret_cast<const float*>(rbase + row_off(it)));
        }
        const char* pl = lds + (chunk & 1) * kH3Buf;
        // fragments of step ks + 1 are requested before the MFMAs of step ks; consecutive MFMAs alternate
        // between the two row blocks (independent accumulators)
        f16x8 af[2][2][2];
        auto frags = [&](int ks, f16x8 (&dst)[2][2]) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int p = 0; p < 2; ++p)
                    dst[m][p] = *reinterpret_cast<const f16x8*>(pl + p * kH3Plane + (32 * m + col) * kH3Pitch +
                                                                (ks * 16 + 8 * half) * 2);
        };
        // inverse scales of this lane's accumulator rows: 32 m + 8 q + 4 half + (0..3), times the column's
        auto row_scales = [&](float4 (&rs)[4], int m, float cs) {
            const float* rsp = reinterpret_cast<const float*>(pl + kH3Rs);
#pragma unroll
            for (int q = 0; q < 4; ++q) rs[q] = cs * ld4(rsp + 32 * m + 8 * q + 4 * half);
        };
        frags(0, af[0]);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            if (ks + 1 < 8) frags(ks + 1, af[(ks + 1) & 1]);
            if (NG > 1 && ks == 4) {   // half 0 is consumed: request the next unit's (same tile or next)
                const int un = (pos_g + 1) % NG;   // next position: same tile, or the next tile's first
                load_b(bset[0], (un + rot) % NG, 0);
            }
            const f16x8(&f)[2][2] = af[ks & 1];
            const f16x8(&bfr)[2][4] = bset[ks >> 2];
            constexpr int TA[3] = {1, 0, 0}, TB[3] = {0, 1, 0};   // lo.hi, hi.lo, hi.hi: smallest terms first
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int m = 0; m < 2; ++m)
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[m][TA[t]], bfr[TB[t]][ks & 3], acc[m], 0, 0, 0);
        }
        if (!EXCH) {
            // direct epilogue from the accumulator layout, one 32-row block at a time; y and its two siblings (NG = 3:
            // the column group selects the output) all have row pitch 128
            const bool full = r0 + kTR <= R;
            const float bias = bias_g[g];
            float* yb = y;
            if constexpr (NG == 3) {
                if (g > 0) yb = ep.y_alt[g - 1];
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                float out[16];
                float4 rs[4];
                row_scales(rs, m, cs_g[g]);
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    float v = fmaf(acc[m][reg], comp(rs[reg >> 2], reg & 3), bias);
                    if (ep.relu) v = fmaxf(v, 0.f);
                    out[reg] = v;
                }
                // Leave as whole 128-byte row segments: the 32 x 32 block goes through a wave-private 4 KiB LDS tile
                // (no barrier: one wave, LDS operations stay in order) and out as four 16-byte-per-lane stores, each
                // covering 8 rows -- instead of sixteen 4-byte-per-lane stores, which cost the consumers as much
                // time as their MFMAs (profiles/r02_gemm_n384_phases.txt).
                float* xw = xb + w * (32 * 32);
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) xw[((reg & 3) + 8 * (reg >> 2) + 4 * half) * 32 + col] = out[reg];
                __builtin_amdgcn_wave_barrier();   // compiler-level ordering only: other lanes' writes are read below
                float4 rowv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) rowv[i] = ld4(xw + (8 * i + (lane >> 3)) * 32 + 4 * (lane & 7));
                __builtin_amdgcn_wave_barrier();
                float* yr = yb + (r0 + 32 * m + (lane >> 3)) * 128 + 32 * w + 4 * (lane & 7);
                if (full) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) st4(yr + static_cast<size_t>(8 * i) * 128, rowv[i]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (r0 + 32 * m + 8 * i + (lane >> 3) < R) st4(yr + static_cast<size_t>(8 * i) * 128, rowv[i]);
                }
            }
        }
        if (EXCH) {
            // exchange through the consumed planes so that each half-wave finalises whole 512-byte rows
            float* ex = reinterpret_cast<float*>(lds + (chunk & 1) * kH3Buf);
            const float bias = bias_g[0];
            float4 rs[2][4];
            row_scales(rs[0], 0, cs_g[0]);
            row_scales(rs[1], 1, cs_g[0]);
            if (LNB) {      // rows of the saved pre-LayerNorm sum: requested here (the fragment registers are free now),
                            // they arrive during the exchange
                const char* pbase = reinterpret_cast<const char*>(ep.lnb_pre) + r0 * 512;
#pragma unroll
                for (int it = 0; it < 4; ++it) lpre[LNB ? it : 0] = ld4(reinterpret_cast<const float*>(pbase + row_off(it)));
            }
            __syncthreads();   // every consumer has finished its fragment reads
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int rr = 32 * m + (reg & 3) + 8 * (reg >> 2) + 4 * half;
                    float v = fmaf(acc[m][reg], comp(rs[m][reg >> 2], reg & 3), bias);
                    if (ep.relu) v = fmaxf(v, 0.f);
                    ex[rr * 128 + 32 * w + col] = v;
                }
            __syncthreads();
            // rows of this wave: w * 16 + it * 2 + half.  `CHECK` only for the tail tile (uniform branch)
            auto finish_rows_lnb = [&](auto check_tag) {
                constexpr bool CHECK = decltype(check_tag)::value;
                float* yrow = reinterpret_cast<float*>(reinterpret_cast<char*>(y + r0 * 128) + ((w * 16 + halfv) * 512u + colv * 16u));
                const float4 gam = ld4(reinterpret_cast<const float*>(reinterpret_cast<const char*>(ep.gamma) + colv * 16u));
                // two groups of four rows (register budget): the second group's rows of the saved pre-LayerNorm sum are
                // requested before the first group is finished
#pragma unroll
                for (int hg = 0; hg < 2; ++hg) {
                    float4 pn[4];
                    if (hg == 0) {
                        const char* pbase = reinterpret_cast<const char*>(ep.lnb_pre) + r0 * 512;
#pragma unroll
                        for (int j = 0; j < 4; ++j) pn[j] = ld4(reinterpret_cast<const float*>(pbase + row_off(4 + j)));
                    }
                    float mu4[4], rs4[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {      // one address per half-wave: broadcast loads
                        unsigned rr = static_cast<unsigned>(w * 16 + (4 * hg + j) * 2) + halfv;
                        rr = rr < lastr ? rr : lastr;
                        mu4[j] = ep.mean[r0 + rr];
                        rs4[j] = ep.rstd[r0 + rr];
                    }
                    float4 yv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int it = 4 * hg + j, rr = w * 16 + it * 2 + half;
                        float4 v = ld4(reinterpret_cast<const float*>(reinterpret_cast<const char*>(ex) + ((w * 16 + it * 2 + halfv) * 512u + colv * 16u)));
                        if (ep.residual) v += res[it];
                        if (CHECK && static_cast<unsigned>(w * 16 + it * 2) + halfv > lastr) v = f4(0.f);
                        const float4 xh = rs4[j] * (lpre[LNB ? j : 0] - f4(mu4[j]));
                        const float4 u = v * gam;
                        const float c1 = half_sum((u.x + u.y) + (u.z + u.w)) * (1.0f / 128.0f);
                        const float c2 = half_sum((u.x * xh.x + u.y * xh.y) + (u.z * xh.z + u.w * xh.w)) * (1.0f / 128.0f);
                        yv[j] = rs4[j] * (u - f4(c1) - c2 * xh);
                        dgam = fma4(v, xh, dgam);
                        dbet += v;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int it = 4 * hg + j, rr = w * 16 + it * 2 + half;
                        if (!CHECK || static_cast<unsigned>(w * 16 + it * 2) + halfv <= lastr) st4(yrow + it * 256, yv[j]);
                        if (hg == 0) lpre[LNB ? j : 0] = pn[j];
                    }
                }
            };
            auto finish_rows = [&](auto check_tag) {
                constexpr bool CHECK = decltype(check_tag)::value;
                float* yrow = y + (r0 + w * 16 + half) * 128 + col * 4;
                float* prow = ep.pre ? ep.pre + (r0 + w * 16 + half) * 128 + col * 4 : nullptr;
                float4 gam = f4(0.f), bet = f4(0.f);
                if (ep.gamma) {
                    gam = ld4(ep.gamma + col * 4);
                    bet = ld4(ep.beta + col * 4);
                }
                // all results of the tile are computed into distinct registers first and stored afterwards:
                // a store-data register that is rewritten while its store is in flight costs a vmcnt(0)
                float4 yv[8], pv[8];
                float mu8[8], rs8[8];
#pragma unroll
                for (int it = 0; it < 8; ++it) {
                    const int rr = w * 16 + it * 2 + half;
                    float4 v = ld4(ex + rr * 128 + col * 4);
                    if (ep.residual) v += res[it];
                    pv[it] = v;
                    if (ep.gamma) {
                        const float mu = half_sum((v.x + v.y) + (v.z + v.w)) * (1.0f / 128.0f);
                        const float4 d = v - f4(mu);
                        const float var = half_sum((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) * (1.0f / 128.0f);
                        const float rs = rsqrtf(var + ep.eps);
                        v = fma4(rs * d, gam, bet);
                        mu8[it] = mu;
                        rs8[it] = rs;
                    }
                    yv[it] = v;
                }
#pragma unroll
                for (int it = 0; it < 8; ++it) {
                    const int rr = w * 16 + it * 2 + half;
                    if (!CHECK || r0 + rr < R) {
                        st4(yrow + it * 256, yv[it]);
                        if (prow && ep.gamma) st4(prow + it * 256, pv[it]);
                    }
                }
                if (ep.gamma && col == 0) {   // one divergent block per tile for the row statistics
#pragma unroll
                    for (int it = 0; it < 8; ++it) {
                        const int rr = w * 16 + it * 2 + half;
                        if (!CHECK || r0 + rr < R) {
                            ep.mean[r0 + rr] = mu8[it];
                            ep.rstd[r0 + rr] = rs8[it];
                        }
                    }
                }
            };
            if constexpr (LNB) {
                if (r0 + kTR <= R) finish_rows_lnb(std::false_type{});
                else finish_rows_lnb(std::true_type{});
            } else {
                if (r0 + kTR <= R) finish_rows(std::false_type{});
                else finish_rows(std::true_type{});
            }
        }
        if (pos_g == NG - 1) __syncthreads();   // end of this chunk's iteration
    };
    load_b(bset[0], NG > 1 ? rot : 0, 0);
    if (NG == 1) load_b(bset[1], 0, 1);
    __syncthreads();   // chunk 0 is in planes[0]
    for (int64_t ti = 0; ti < my_tiles; ++ti) {
        if constexpr (NG == 1) {
            unit(ti, 0);
        } else {   // rolled on purpose: three inlined copies let hipcc hoist loads across units and spill
#pragma unroll 1
            for (int u = 0; u < NG; ++u) unit(ti, u);
        }
    }
    for (int64_t c = nchunks; c < padded; ++c) __syncthreads();   // match the producers' padded iterations
    if (LNB) {      // per half-wave partials of dgamma / dbeta (reduced in a fixed order by ln_finish)
        float* pp = ep.lnb_part + (static_cast<size_t>(blockIdx.x) * 8 + 2 * w + half) * 256 + col * 4;
        st4(pp, dgam);
        st4(pp + 128, dbet);
    }
}


// ------------------------------------------------------------------------------------------------------
// sum3: y = a0 B0 + a1 B1 + a2 B2 (+ residual), the input gradient of the q / k / v Linears of an attention block.
// A 384 -> 128 contraction whose three 128-wide chunks are three separate [R,128] matrices.  The B fragments of
// the chunks cannot all be resident (3 x 96 VGPRs), and re-reading 96 KiB from L2 for every 64-row unit bounds the
// MFMA phase (every CU pulls the same bytes: ~15-19 TB/s in aggregate).  This program
//   * walks two tiles at a time, position major -- (t0,0) (t1,0) (t0,1) (t1,1) (t0,2) (t1,2) -- so one set
//     of B fragments serves two units (two accumulator sets);
//   * refills the fragments by hand: the load of a k-step's registers is issued right after their last
//     MFMA in the second unit of a position, the first unit of the next position waits per k-step with the
//     exact in-order count (3 (7 - ks) younger loads) -- the consumers issue no other VMEM operation;
//   * keeps every global access in waves 4..7: A chunks HBM -> registers (three deep) -> split -> fp16
//     planes, and the finished tile's epilogue (exchange tile in LDS -> + residual -> 512-byte row stores).
//     Their loop is one straight line per tile pair so that hipcc can count loads in flight.
// Barriers: B(c) ends every chunk; A(c) precedes the exchange-tile write of a chunk that completes a tile.
__device__ __forceinline__ void load_b128_async(f16x8& dst, const f16x8* p) {
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_b_refill(f16x8& b0, f16x8& b1) {
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(b0), "+v"(b1) : "n"(N));
}

struct Sum3Operands {
    const float* a[3];          // the three [R,128] operands: k-chunk kc of the contraction is a[kc]
    const float* residual;      // [R,128] or null
};

template <bool RES>      // RES: in.residual is non-null
__global__ __launch_bounds__(512, 2) void row_gemm_h3_sum3_kernel(Sum3Operands in, const f16x8* __restrict__ packed,
                                                                  float* __restrict__ y, int64_t R) {
    constexpr int KC = 3, KS = 24;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* lds = smem_raw;                                          // 2 x { planes[2][64 rows][272 B], inv_row_scale[64] }
    float* ex = reinterpret_cast<float*>(smem_raw + 2 * kH3Buf);   // exchange tile [64][128] fp32
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, col = lane & 31;
    const int64_t tiles = (R + kTR - 1) / kTR;
    if (static_cast<int64_t>(blockIdx.x) >= tiles) return;
    const int ntl = static_cast<int>((tiles - blockIdx.x + gridDim.x - 1) / gridDim.x);
    const int npairs = ntl / 2, nchunks = 3 * ntl;
    const int rot = static_cast<int>(blockIdx.x % 3);   // rotated chunk order per workgroup (spreads the L2 stream)
    auto tile_row0 = [&](int ti) { return (blockIdx.x + static_cast<int64_t>(ti) * gridDim.x) * kTR; };
    auto chunk_map = [&](int c, int& ti, int& pos) {
        if (c < 6 * npairs) {
            const int p = c / 6, r = c - 6 * p;
            pos = r >> 1;
            ti = 2 * p + (r & 1);
        } else {
            pos = c - 6 * npairs;
            ti = ntl - 1;
        }
    };

    if (w >= 4) {
        // ---------------------------------------------------------------------- movers
        // (they are the critical path: their VALU work wins the issue arbitration against the consumer on the SIMD)
        __builtin_amdgcn_s_setprio(3);
        const int pw = w - 4, pt = threadIdx.x - 256;
        float4 pf[3][8];
        // loads of a chunk: uniform 64-bit base (tile, operand) + a 32-bit per-lane byte offset; rows past the end
        // of a partial tile are clamped on the offset (row-major, so the row term dominates the comparison)
        const unsigned voff0 = static_cast<unsigned>(pt >> 5) * 512 + static_cast<unsigned>(pt & 31) * 16;
        auto fetch = [&](float4 (&set)[8], int c) {
            if (c > nchunks - 1) c = nchunks - 1;
            int ti, pos;
            chunk_map(c, ti, pos);
            const int64_t r0 = tile_row0(ti);
            const int kc = (pos + rot) % KC;
            const char* base = reinterpret_cast<const char*>(in.a[kc]) + r0 * 512;
            const int64_t last = R - 1 - r0;   // >= 0
            const unsigned lim = last >= kTR - 1 ? 0xFFFFFFFFu : static_cast<unsigned>(last) * 512 + static_cast<unsigned>(pt & 31) * 16;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                unsigned off = voff0 + i * (8 * 512);
                off = off < lim ? off : lim;
                set[i] = ld4(reinterpret_cast<const float*>(base + off));
            }
        };
        auto write = [&](const float4 (&set)[8], int c) {   // chunks past the end land in the idle buffer
            // the scale of a row is per 128-wide chunk: each chunk has its own accumulation
            split_write_h3<8, 256>(set, lds + (c & 1) * kH3Buf, pt);
        };
        float4 res[8];   // residual rows of the tile being finished: pw * 16 + it * 2 + half
        auto fetch_residual = [&](int ti) {
            if (!RES) return;
            const int64_t r0 = tile_row0(ti);
            const char* base = reinterpret_cast<const char*>(in.residual) + r0 * 512;
            const int64_t last = R - 1 - r0;
            const unsigned lim = last >= kTR - 1 ? 0xFFFFFFFFu : static_cast<unsigned>(last) * 512 + col * 16;
            const unsigned roff0 = static_cast<unsigned>(pw * 16 + half) * 512 + col * 16;
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                unsigned off = roff0 + it * 1024;
                off = off < lim ? off : lim;
                res[it] = ld4(reinterpret_cast<const float*>(base + off));
            }
        };
        auto store_tile = [&](int ti) {   // exchange tile (+ residual) -> global rows
            const int64_t r0 = tile_row0(ti);
            const bool full = r0 + kTR <= R;
            float* yrow = y + (r0 + pw * 16 + half) * 128 + col * 4;
            // two groups of four rows; inside a group every result has its own registers and the stores follow
            // the arithmetic
#pragma unroll
            for (int hg = 0; hg < 2; ++hg) {
                float4 yv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int it = 4 * hg + j, rr = pw * 16 + it * 2 + half;
                    yv[j] = ld4(ex + rr * 128 + col * 4);
                    if (RES) yv[j] += res[it];
                }
                if (full) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) st4(yrow + (4 * hg + j) * 256, yv[j]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int it = 4 * hg + j, rr = pw * 16 + it * 2 + half;
                        if (r0 + rr < R) st4(yrow + it * 256, yv[j]);
                    }
                }
            }
        };
        fetch(pf[0], 0);
        fetch(pf[1], 1);
        fetch(pf[2], 2);
        write(pf[0], 0);
        fetch(pf[0], 3);
        __syncthreads();   // chunk 0 is in planes[0]
        int c = 0;
        for (int p = 0; p < npairs; ++p, c += 6) {
            const int t0 = 2 * p, t1 = 2 * p + 1;
            write(pf[1], c + 1); fetch(pf[1], c + 4); __syncthreads();                              // (t0, 0)
            write(pf[2], c + 2); fetch(pf[2], c + 5); __syncthreads();                              // (t1, 0)
            write(pf[0], c + 3); fetch(pf[0], c + 6); __syncthreads();                              // (t0, 1)
            write(pf[1], c + 4); fetch(pf[1], c + 7); fetch_residual(t0); __syncthreads();          // (t1, 1)
            write(pf[2], c + 5); fetch(pf[2], c + 8); __syncthreads(); __syncthreads();             // (t0, 2): A, B
            store_tile(t0);
            fetch_residual(t1);
            write(pf[0], c + 6); fetch(pf[0], c + 9); __syncthreads(); __syncthreads();             // (t1, 2): A, B
            store_tile(t1);
        }
        if (ntl & 1) {
            const int t = ntl - 1;
            write(pf[1], c + 1); fetch(pf[1], c + 4); __syncthreads();                              // (t, 0)
            write(pf[2], c + 2); fetch(pf[2], c + 5); fetch_residual(t); __syncthreads();           // (t, 1)
            write(pf[0], c + 3); __syncthreads(); __syncthreads();                                  // (t, 2): A, B
            store_tile(t);
        }
        return;
    }

    // -------------------------------------------------------------------------- consumers
    f16x8 bfr[2][8];
    auto b_ptr = [&](int pos) { return packed + (static_cast<size_t>(w) * KS + ((pos + rot) % KC) * 8) * 2 * 64 + lane; };
    {
        const f16x8* b0 = b_ptr(0);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int p = 0; p < 2; ++p) bfr[p][ks] = b0[(ks * 2 + p) * 64];
    }
    const float cs = reinterpret_cast<const float*>(packed + static_cast<size_t>(4) * KS * 2 * 64)[32 * w + col];
    f32x16 accs[2][2];
    int chunk = 0;
    __syncthreads();   // chunk 0 is in planes[0]
    auto body = [&](int pos, f32x16 (&acc)[2], auto second_tag) {
        constexpr bool SECOND = decltype(second_tag)::value;
        if (pos == 0) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
        }
        const f16x8* bnext = b_ptr((pos + 1) % KC);
        const char* pl = lds + (chunk & 1) * kH3Buf;
        f16x8 af[2][2][2];
        auto frags = [&](int ks, f16x8 (&dst)[2][2]) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int p = 0; p < 2; ++p)
                    dst[m][p] = *reinterpret_cast<const f16x8*>(pl + p * kH3Plane + (32 * m + col) * kH3Pitch +
                                                                (ks * 16 + 8 * half) * 2);
        };
        f32x16 part[2];   // this chunk's products; folded into `acc` with the chunk's inverse row scales
        frags(0, af[0]);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            if (ks + 1 < 8) frags(ks + 1, af[(ks + 1) & 1]);
            if (!SECOND) {
                switch (ks) {
                    case 0: wait_b_refill<14>(bfr[0][ks], bfr[1][ks]); break;
                    case 1: wait_b_refill<12>(bfr[0][ks], bfr[1][ks]); break;
                    case 2: wait_b_refill<10>(bfr[0][ks], bfr[1][ks]); break;
                    case 3: wait_b_refill<8>(bfr[0][ks], bfr[1][ks]); break;
                    case 4: wait_b_refill<6>(bfr[0][ks], bfr[1][ks]); break;
                    case 5: wait_b_refill<4>(bfr[0][ks], bfr[1][ks]); break;
                    case 6: wait_b_refill<2>(bfr[0][ks], bfr[1][ks]); break;
                    default: wait_b_refill<0>(bfr[0][ks], bfr[1][ks]); break;
                }
            }
            const f16x8(&f)[2][2] = af[ks & 1];
            constexpr int TA[3] = {1, 0, 0}, TB[3] = {0, 1, 0};   // lo.hi, hi.lo, hi.hi: smallest terms first
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    if (ks == 0 && t == 0) {
                        const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                        part[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[m][TA[t]], bfr[TB[t]][ks], zero, 0, 0, 0);
                    } else {
                        part[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[m][TA[t]], bfr[TB[t]][ks], part[m], 0, 0, 0);
                    }
                }
            if (SECOND) {
#pragma unroll
                for (int p = 0; p < 2; ++p) load_b128_async(bfr[p][ks], bnext + (ks * 2 + p) * 64);
            }
        }
        {
            const float* rsp = reinterpret_cast<const float*>(pl + kH3Rs);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    // inverse row scale of the chunk TIMES this lane's inverse column scale: folding with the row scale alone
                    // overflows for rows above ~2^90 although the result is representable (tests: max 2^120 row)
                    const float4 r4 = cs * ld4(rsp + 32 * m + 8 * q + 4 * half);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[m][4 * q + i] = fmaf(part[m][4 * q + i], comp(r4, i), acc[m][4 * q + i]);
                }
        }
        if (pos == KC - 1) {
            __syncthreads();   // A: the movers have finished with the previous exchange tile
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int rr = 32 * m + (reg & 3) + 8 * (reg >> 2) + 4 * half;
                    ex[rr * 128 + 32 * w + col] = acc[m][reg];
                }
        }
        __syncthreads();   // B
        ++chunk;
    };
    for (int p = 0; p < npairs; ++p) {
#pragma unroll 1
        for (int pos = 0; pos < KC; ++pos) {
            body(pos, accs[0], std::false_type{});
            body(pos, accs[1], std::true_type{});
        }
    }
    if (ntl & 1) {
#pragma unroll 1
        for (int pos = 0; pos < KC; ++pos) {
            body(pos, accs[0], std::false_type{});
            if (pos + 1 < KC) {   // no partner tile: refill between the units
                const f16x8* bnext = b_ptr(pos + 1);
#pragma unroll
                for (int ks = 0; ks < 8; ++ks)
#pragma unroll
                    for (int q = 0; q < 2; ++q) load_b128_async(bfr[q][ks], bnext + (ks * 2 + q) * 64);
            }
        }
    }
}

}  // namespace
}  // namespace dg

namespace dg {

size_t row_gemm_f32_packed_floats(int n_out, int k_contract) {
    if (n_out < 1 || k_contract < 1) return 0;
    const size_t nt = (n_out + 31) / 32, kc = (k_contract + 127) / 128;
    return nt * kc * 8 * 2 * 64 * 4 + nt * 32;   // fp16x3: [slab][k-step][plane][lane] x 8 fp16, inv_col_scale
}

int row_gemm_f32_pack(const float* w, float* packed, int rows, int cols, int mode, dg_stream_t stream_,
                      const float* w1, const float* w2) {
    if (!w || !packed) return fail(DG_E_ARG, "dg_row_gemm_pack: null pointer");
    if ((w1 || w2) && (!w1 || !w2 || rows != 384))
        return fail(DG_E_ARG, "dg_row_gemm_pack3: needs three [128, cols] weights");
    if (mode != 0 && mode != 1) return fail(DG_E_ARG, "dg_row_gemm_pack: mode must be 0 (forward) or 1 (dgrad)");
    const int n_out = mode == 0 ? rows : cols, k = mode == 0 ? cols : rows;
    const int nt = (n_out + 31) / 32, kc = (k + 127) / 128;
    hipLaunchKernelGGL(pack_weight_h3_kernel, dim3(nt, kc), dim3(512), 0, static_cast<hipStream_t>(stream_), w, w1, w2,
                       reinterpret_cast<f16x8*>(packed), rows, cols, mode, nt);
    return check_launch("dg_row_gemm_pack");
}

int row_gemm_f32_pack_batch(const void* table, int n, int max_rows_cols, dg_stream_t stream_) {
    if (!table) return fail(DG_E_ARG, "dg_row_gemm_pack_batch: null pointer");
    if (n < 1) return 0;
    const int nt = (max_rows_cols + 31) / 32, kc = (max_rows_cols + 127) / 128;
    hipLaunchKernelGGL(pack_weight_h3_batch_kernel, dim3(nt, kc, n), dim3(512), 0, static_cast<hipStream_t>(stream_),
                       static_cast<const long long*>(table));
    return check_launch("dg_row_gemm_pack_batch");
}

size_t row_gemm_f32_mask_words(int64_t R, int K, int N) {
    // geometry of the direct-epilogue kernels (see the launch table in dg_row_gemm)
    if (K == 128 && N == 384) return static_cast<size_t>((R + 31) / 32) * 12 * 64;      // (>= row_gemm_n384_mask_words(R))
    if (K == 128 && N == 128) return static_cast<size_t>((R + 63) / 64) * 8 * 64;   // upper bound over variants
    return 0;
}

int row_gemm_f32(const float* a, const float* packed, float* y, int64_t R, int K, int N, const float* bias,
                           int relu, unsigned* relu_bits_out, const unsigned* mask_bits, const float* residual,
                           const float* gamma, const float* beta, float* mean, float* rstd, float* pre_ln,
                           float eps, dg_stream_t stream_, const float* ascale, float* yscale, int afmt, int yfmt,
                           const void* alo, void* ylo) {
    if (!a || !packed || !y) return fail(DG_E_ARG, "dg_row_gemm: null pointer");
    if ((afmt && K != 384) || (yfmt && N != 384)) return fail(DG_E_ARG, "dg_row_gemm: narrow hidden operands are the 384-wide ones");
    if (R < 0 || !((K == 128 && (N == 128 || N == 384)) || (K == 384 && N == 128)))
        return fail(DG_E_SHAPE, "dg_row_gemm: unsupported K=%d N=%d (supported: 128x128, 128x384, 384x128)", K, N);
    if (gamma && (N != 128 || !beta || !mean || !rstd))
        return fail(DG_E_ARG, "dg_row_gemm: LayerNorm epilogue needs N == 128, beta, mean and rstd");
    const bool exch = gamma || residual;
    if (exch && (mask_bits || relu_bits_out))
        return fail(DG_E_ARG, "dg_row_gemm: bit masks cannot be combined with residual / LayerNorm epilogues");
    if ((mask_bits || relu_bits_out) && K != 128)
        return fail(DG_E_ARG, "dg_row_gemm: bit masks need K == 128");
    if (exch && N != 128) return fail(DG_E_ARG, "dg_row_gemm: residual / LayerNorm epilogues need N == 128");
    if ((mask_bits || relu_bits_out) && N != 384)
        return fail(DG_E_ARG, "dg_row_gemm: bit masks need the 128 -> 384 shape");
    if (R == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Epilogue ep;
    ep.bias = bias;
    ep.residual = residual;
    ep.gamma = gamma;
    ep.beta = beta;
    ep.mean = mean;
    ep.rstd = rstd;
    ep.pre = pre_ln;
    ep.eps = eps;
    ep.relu = relu;
    ProfScope prof(R < edge_rows() ? DG_K_ROW_GEMM : (K == 384 ? DG_K_ROW_GEMM_E_K384 : (N == 384 ? DG_K_ROW_GEMM_E_N384 : DG_K_ROW_GEMM_E_128)), stream);
    // 128 -> 384: the producer / consumer kernel (row_gemm_n384.hip)
    if (K == 128 && N == 384) {
        if (int st = launch_row_gemm_n384(a, packed, y, yscale, R, bias, relu, relu_bits_out, mask_bits, stream, yfmt, ylo)) return st;
        return check_launch("dg_row_gemm");
    }
    // 384 -> 128: the producer / consumer kernel (row_gemm_k384.hip)
    if (K == 384) {
        if (int st = launch_row_gemm_k384(a, ascale, packed, y, R, bias, relu, residual, gamma, beta, mean, rstd, pre_ln, eps, stream, afmt, alo))
            return st;
        return check_launch("dg_row_gemm");
    }
    const int64_t tiles = (R + kTR - 1) / kTR;
    const int seqs = static_cast<int>(tiles < 256 ? tiles : 256);      // one 8-wave workgroup per CU
    ep.reverse = take_direction(R);
#define LAUNCH_H3(EX_)                                                                                         \
    {                                                                                                          \
        constexpr int lds_ = kH3Lds + (EX_ ? 0 : 4 * 32 * 32 * 4);                                            \
        DG_OPT_IN_LDS((&row_gemm_h3_kernel<1, EX_>), lds_);                                                    \
        hipLaunchKernelGGL((row_gemm_h3_kernel<1, EX_>), dim3(seqs), dim3(512), lds_, stream, a,               \
                           reinterpret_cast<const f16x8*>(packed), y, R, ep);                                  \
    }
    if (exch) LAUNCH_H3(true)
    else LAUNCH_H3(false)
#undef LAUNCH_H3
    return check_launch("dg_row_gemm");
}


size_t row_gemm_f32_ln_bwd_workspace_bytes() { return static_cast<size_t>(256) * 8 * 256 * sizeof(float); }

// dz = LayerNormBackward(a B + residual; pre, mean, rstd, gamma), dgamma, dbeta: see Epilogue::lnb_pre
int row_gemm_f32_ln_bwd(const float* a, const float* packed, float* dz, int64_t R, int K, const float* residual,
                        const float* pre, const float* mean, const float* rstd, const float* gamma, float* dgamma,
                        float* dbeta, void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (!a || !packed || !dz || !pre || !mean || !rstd || !gamma || !workspace)
        return fail(DG_E_ARG, "dg_row_gemm_ln_bwd: null pointer");
    // (384 -> 128: the epilogue of that kernel runs in its producer waves, which already hold three A chunks in
    // registers: built, 593 us against 302 + 161 us for the two launches at R = 518 400 -- not kept)
    if (R < 0 || K != 128) return fail(DG_E_SHAPE, "dg_row_gemm_ln_bwd: unsupported K=%d (K = N = 128)", K);
    if (workspace_bytes < row_gemm_f32_ln_bwd_workspace_bytes()) return fail(DG_E_WORKSPACE, "dg_row_gemm_ln_bwd: workspace too small");
    if (R == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Epilogue ep;
    ep.residual = residual;
    ep.gamma = gamma;
    ep.mean = const_cast<float*>(mean);
    ep.rstd = const_cast<float*>(rstd);
    ep.lnb_pre = pre;
    ep.lnb_part = static_cast<float*>(workspace);
    const int64_t tiles = (R + kTR - 1) / kTR;
    const int seqs = static_cast<int>(tiles < 256 ? tiles : 256);
    {
        ProfScope prof(R < edge_rows() ? DG_K_ROW_GEMM : DG_K_ROW_GEMM_E_128, stream);
        note_forward(R);      // (dgamma / dbeta partial sums: the order of the rows matters)
        DG_OPT_IN_LDS((&row_gemm_h3_kernel<1, true, true>), kH3Lds);
        hipLaunchKernelGGL((row_gemm_h3_kernel<1, true, true>), dim3(seqs), dim3(512), kH3Lds, stream, a,
                           reinterpret_cast<const f16x8*>(packed), dz, R, ep);
    }
    if (dgamma || dbeta) launch_ln_finish(ep.lnb_part, seqs * 8, 2, 128, dgamma, dbeta, stream);
    return check_launch("dg_row_gemm_ln_bwd");
}

// y = dz B with dz = LayerNormBackward(dy; pre, mean, rstd, gamma) computed (and written) on the way in: see
// Epilogue::lna_pre.  K = N = 128.
int row_gemm_f32_ln_in(const float* dy, const float* pre, const float* mean, const float* rstd, const float* gamma,
                       const float* packed, float* dz, float* y, float* dgamma, float* dbeta, void* workspace,
                       size_t workspace_bytes, int64_t R, dg_stream_t stream_) {
    if (!dy || !pre || !mean || !rstd || !gamma || !packed || !dz || !y || !workspace)
        return fail(DG_E_ARG, "dg_row_gemm_ln_bwd_in: null pointer");
    if (R < 0) return fail(DG_E_SHAPE, "dg_row_gemm_ln_bwd_in: R = %lld", static_cast<long long>(R));
    if (workspace_bytes < row_gemm_f32_ln_bwd_workspace_bytes()) return fail(DG_E_WORKSPACE, "dg_row_gemm_ln_bwd_in: workspace too small");
    if (R == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Epilogue ep;
    ep.gamma = gamma;
    ep.mean = const_cast<float*>(mean);
    ep.rstd = const_cast<float*>(rstd);
    ep.lna_pre = pre;
    ep.lna_dz = dz;
    ep.lnb_part = static_cast<float*>(workspace);
    const int64_t tiles = (R + kTR - 1) / kTR;
    const int seqs = static_cast<int>(tiles < 256 ? tiles : 256);
    {
        ProfScope prof(R < edge_rows() ? DG_K_ROW_GEMM : DG_K_ROW_GEMM_E_128, stream);
        note_forward(R);      // (dgamma / dbeta partial sums: the order of the rows matters)
        constexpr int lds = kH3Lds + 4 * 32 * 32 * 4;
        DG_OPT_IN_LDS((&row_gemm_h3_kernel<1, false, false, true>), lds);
        hipLaunchKernelGGL((row_gemm_h3_kernel<1, false, false, true>), dim3(seqs), dim3(512), lds, stream, dy,
                           reinterpret_cast<const f16x8*>(packed), y, R, ep);
    }
    // inside dg_linear_wgrad_batch_begin / _end the reduction joins that batch's launch (dgamma, dbeta adjacent)
    if ((dgamma || dbeta) && !(dgamma && dbeta == dgamma + 128 && reduce_batch_try_add(ep.lnb_part, seqs * 8, 256, dgamma)))
        launch_ln_finish(ep.lnb_part, seqs * 8, 2, 128, dgamma, dbeta, stream);
    return check_launch("dg_row_gemm_ln_bwd_in");
}


// Three Linears that share their input in ONE launch: y_i = a W_i^T + b_i (q / k / v of an attention block, reference
// layers.py:111-113; also their transposed use in the second order).  `packed`: dg_row_gemm_pack3(mode 0).
int row_gemm_f32_lin3(const float* a, const float* packed, float* y0, float* y1, float* y2, int64_t R, const float* b0,
                      const float* b1, const float* b2, dg_stream_t stream_) {
    if (!a || !packed || !y0 || !y1 || !y2) return fail(DG_E_ARG, "dg_row_gemm_lin3: null pointer");
    if (R < 0) return fail(DG_E_SHAPE, "dg_row_gemm_lin3: negative row count");
    if (R == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Epilogue ep;
    ep.bias = b0;
    ep.y_alt[0] = y1;
    ep.y_alt[1] = y2;
    ep.bias_alt[0] = b1;
    ep.bias_alt[1] = b2;
    const int64_t tiles = (R + kTR - 1) / kTR;
    const int seqs = static_cast<int>(tiles < 256 ? tiles : 256);
    // profiler / roofline: an edge-level launch of this kernel is a 128 -> 384 launch
    ProfScope prof(R < edge_rows() ? DG_K_ROW_GEMM : DG_K_ROW_GEMM_E_N384, stream);
    // the column-group kernel (B fragments streamed per group: these launches are node-level, one or two tiles per
    // workgroup, where residency buys nothing; the resident-B instance with three outputs spills 168 B / lane)
    constexpr int lds3 = kH3Lds + 4 * 32 * 32 * 4;
    DG_OPT_IN_LDS((&row_gemm_h3_kernel<3, false>), lds3);
    hipLaunchKernelGGL((row_gemm_h3_kernel<3, false>), dim3(seqs), dim3(512), lds3, stream, a,
                       reinterpret_cast<const f16x8*>(packed), y0, R, ep);
    return check_launch("dg_row_gemm_lin3");
}

// y = a0 B0 + a1 B1 + a2 B2 (+ residual): the input gradient of those three Linears in ONE launch -- a 384 -> 128
// contraction whose k-chunks are three separate [R,128] matrices.  `packed`: dg_row_gemm_pack3(mode 1).
int row_gemm_f32_sum3(const float* a0, const float* a1, const float* a2, const float* packed, float* y, int64_t R,
                      const float* residual, dg_stream_t stream_) {
    if (!a0 || !a1 || !a2 || !packed || !y) return fail(DG_E_ARG, "dg_row_gemm_sum3: null pointer");
    if (R < 0) return fail(DG_E_SHAPE, "dg_row_gemm_sum3: negative row count");
    if (R == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Sum3Operands in{{a0, a1, a2}, residual};
    const int64_t tiles = (R + kTR - 1) / kTR;
    const int seqs = static_cast<int>(tiles < 256 ? tiles : 256);
    ProfScope prof(R < edge_rows() ? DG_K_ROW_GEMM : DG_K_ROW_GEMM_E_K384, stream);
    constexpr int lds384 = 2 * kH3Buf + kTR * 128 * 4;
    if (residual) {
        DG_OPT_IN_LDS((&row_gemm_h3_sum3_kernel<true>), lds384);
        hipLaunchKernelGGL((row_gemm_h3_sum3_kernel<true>), dim3(seqs), dim3(512), lds384, stream, in,
                           reinterpret_cast<const f16x8*>(packed), y, R);
    } else {
        DG_OPT_IN_LDS((&row_gemm_h3_sum3_kernel<false>), lds384);
        hipLaunchKernelGGL((row_gemm_h3_sum3_kernel<false>), dim3(seqs), dim3(512), lds384, stream, in,
                           reinterpret_cast<const f16x8*>(packed), y, R);
    }
    return check_launch("dg_row_gemm_sum3");
}

}  // namespace dg
